"""WaveGlow.forward (the analysis pass) against infer_from_noise of the same model and shape, and against the same arithmetic in
plain PyTorch ops on the same GPU.

Config "full" (12 flows x 8 layers x 512 channels, synthetic weights), 900 frames, B = 1 and 8.  Arms, alternated in one process
(warm-up first, `--reps` repetitions each), timed with device events on the current stream:

  a  forward:     cookietts_amd.WaveGlow.forward(mel, audio) - z, log_s and the log det list
  b  infer:       cookietts_amd.WaveGlow.infer_from_noise(mel, z) of the same model: the same WN launches in the other direction
  c  torch GPU:   glow.py:267-312 restated below in plain PyTorch ops (matmuls over shifted copies for the dilated and the transposed
                  convolutions, so no convolution library's kernel search enters the timing), fp32

The reference tree is not imported.  A difference is claimed only where it is >= 10 x the larger arm's spread (max - min).

usage: python scripts/debug/waveglow_forward_ab.py [--reps 5] [--frames 900] [--batches 1 8] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from cookietts_amd import WaveGlow, synthetic  # noqa: E402


class PlainForward:
    """glow.py:267-312 (and WN, :188-222) in torch ops, weight norm folded once."""

    def __init__(self, sd, cfg, device):
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in sd.items()}
        self.cfg, self.t = cfg, t

        def conv(prefix):
            if prefix + ".weight" in t:
                return t[prefix + ".weight"]
            v, g = t[prefix + ".weight_v"], t[prefix + ".weight_g"]
            return v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1))
        wn = cfg["WN_config"]
        self.flows = []
        for k in range(cfg["n_flows"]):
            p = f"WN.{k}"
            f = {"W": t[f"convinv.{k}.conv.weight"][:, :, 0], "start": (conv(p + ".start")[:, :, 0], t[p + ".start.bias"]),
                 "end": (t[p + ".end.weight"][:, :, 0], t[p + ".end.bias"]),
                 "cond": [(conv(f"{p}.cond_layers.{j}")[:, :, 0], t[f"{p}.cond_layers.{j}.bias"]) for j in range(3)],
                 "in": [(conv(f"{p}.in_layers.{i}"), t[f"{p}.in_layers.{i}.bias"]) for i in range(wn["n_layers"])],
                 "rs": [(conv(f"{p}.res_skip_layers.{i}")[:, :, 0], t[f"{p}.res_skip_layers.{i}.bias"]) for i in range(wn["n_layers"])]}
            self.flows.append(f)

    @staticmethod
    def _lin(wb, x):
        return torch.matmul(wb[0], x) + wb[1][None, :, None]

    def _wn(self, f, a0, spect):
        C = self.cfg["WN_config"]["n_channels"]
        x = self._lin(f["start"], a0)
        h = self._lin(f["cond"][1], self._lin(f["cond"][0], spect))
        L = x.shape[2]
        out = None
        n = len(f["in"])
        for i in range(n):
            d = 2 ** i
            w, b = f["in"][i]
            sl = slice(2 * C * i, 2 * C * (i + 1))
            u = torch.matmul(f["cond"][2][0][sl], h) + (f["cond"][2][1][sl] + b)[None, :, None]
            xp = torch.nn.functional.pad(x, (d, d))
            for tap in range(3):
                u = u + torch.matmul(w[:, :, tap], xp[:, :, tap * d:tap * d + L])
            act = torch.tanh(u[:, :C]) * torch.sigmoid(u[:, C:])
            r = self._lin(f["rs"][i], act)
            if i < n - 1:
                x = x + r[:, :C]
                out = r[:, C:] if out is None else out + r[:, C:]
            else:
                out = r if out is None else out + r
        e = self._lin(f["end"], out)
        hh = e.shape[1] // 2
        return e[:, :hh], e[:, hh:]

    @torch.no_grad()
    def __call__(self, mel, wave):
        cfg = self.cfg
        G, hop = cfg["n_group"], cfg["hop_length"]
        B, _, F = mel.shape
        w_up, taps = self.t["upsample.weight"], cfg["win_length"] // hop
        y = torch.zeros(B, w_up.shape[1], F + taps - 1, hop, device=mel.device)
        for j in range(taps):                                            # the transposed conv: frame f lands on output frame f + j
            y[:, :, j:j + F] += torch.einsum("bif,iop->bofp", mel, w_up[:, :, j * hop:(j + 1) * hop])
        spect = y[:, :, :F].reshape(B, w_up.shape[1], F * hop) + self.t["upsample.bias"][None, :, None]
        spect = spect.unfold(2, G, G).permute(0, 2, 1, 3).reshape(B, F * hop // G, -1).permute(0, 2, 1).contiguous()
        audio = wave.unfold(1, G, G).permute(0, 2, 1)
        outs, log_s_list, log_det = [], [], []
        for k, f in enumerate(self.flows):
            if k % cfg["n_early_every"] == 0 and k > 0:
                outs.append(audio[:, :cfg["n_early_size"]])
                audio = audio[:, cfg["n_early_size"]:]
            audio = torch.matmul(f["W"], audio)
            log_det.append(B * audio.shape[2] * torch.logdet(f["W"]))
            h = audio.shape[1] // 2
            b, log_s = self._wn(f, audio[:, :h], spect)
            audio = torch.cat([audio[:, :h], torch.exp(log_s) * audio[:, h:] + b], 1)
            log_s_list.append(log_s)
        outs.append(audio)
        return torch.cat(outs, 1), log_s_list, log_det


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=900)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--config", default="full")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = synthetic.WAVEGLOW_CONFIGS[a.config]
    sd = synthetic.waveglow_state_dict(cfg, seed=9)
    dev = torch.device("cuda", 0)
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(sd))
    m = m.cuda().eval()
    plain = PlainForward(sd, cfg, dev)
    lines = []
    for B in a.batches:
        F = a.frames
        mel = torch.from_numpy(synthetic.synthetic_mel(B, F, cfg["n_mel_channels"], seed=3)).to(dev)
        wave = (torch.from_numpy(np.random.default_rng(4).standard_normal((B, F * cfg["hop_length"]), dtype=np.float32)) * 0.3).to(dev)
        z0 = m(mel, wave)[0]
        arms = {"a_forward": lambda: m(mel, wave), "b_infer": lambda: m.infer_from_noise(mel, z0), "c_torch_gpu": lambda: plain(mel, wave)}
        res = {k: fn() for k, fn in arms.items()}                       # warm-up (workspaces, library handles), results compared
        torch.cuda.synchronize()
        back = res["b_infer"]
        rt = float(((back - wave).double().pow(2).mean() / wave.double().pow(2).mean()).sqrt())
        dz = float((res["a_forward"][0] - res["c_torch_gpu"][0]).abs().max())
        dls = float((torch.cat(res["a_forward"][1], 1) - torch.cat(res["c_torch_gpu"][1], 1)).abs().max())
        del res, back
        ev = {k: [] for k in arms}
        for _ in range(a.reps):                                          # arms alternated
            for k, fn in arms.items():
                ev[k].append(timed(fn)[0])
        med = {k: float(np.median(v)) for k, v in ev.items()}
        spread = {k: float(max(v) - min(v)) for k, v in ev.items()}
        line = dict(row="waveglow_forward_ab", config=a.config, batch=B, frames=F, steps=F * cfg["hop_length"] // cfg["n_group"],
                    reps=a.reps, event_ms={k: [round(x, 3) for x in v] for k, v in ev.items()},
                    median_ms={k: round(v, 3) for k, v in med.items()}, spread_ms={k: round(v, 3) for k, v in spread.items()},
                    round_trip_rms_rel=rt, max_abs_diff_z_a_vs_c=dz, max_abs_diff_log_s_a_vs_c=dls)
        for other in ("b_infer", "c_torch_gpu"):
            larger = max(spread["a_forward"], spread[other])
            d = med["a_forward"] - med[other]
            line[f"a_minus_{other}_ms"] = round(d, 3)
            line[f"a_over_{other}"] = round(med["a_forward"] / med[other], 4)
            line[f"a_vs_{other}_difference_exceeds_10x_spread"] = bool(abs(d) >= 10 * larger)
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
