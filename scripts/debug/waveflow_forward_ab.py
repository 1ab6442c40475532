"""WaveFlow analysis pass: the all-rows form against the row-wise form, ``infer_from_noise`` and plain PyTorch ops, config 4.

Model: BASELINE config 4 (``synthetic.WAVEFLOW_CONFIGS["full"]``), an 80 x ``--frames`` mel (+ the zero frame ``infer`` pads), audio of
frames * hop samples, batch ``--batch``.  Arms, alternated in one process (one call each to pack and allocate, ``--warmup`` rounds that run like the
timed ones and are dropped, then ``--reps`` timed repetitions; device events around each call, median and spread = max - min):

  forward            ``WaveFlow.forward`` as it selects its form (all-rows on this model)
  forward_rowwise    the same under CTTS_WF_FWD_ROWWISE=1
  infer_from_noise   the synthesis direction of the same model on the same shape (return_CPU=False)
  torch_conv2d       the same forward arithmetic as F.conv2d / F.interpolate ops of PyTorch-ROCm on the same GPU

The torch arm's z is compared with the device's first (RMS relative), so that the arms are known to compute the same thing.  A
difference is claimed at >= 10 x the larger arm's spread only; the record says ``claimed`` per pair.

usage: python scripts/debug/waveflow_forward_ab.py --batch 1 [--frames 900] [--reps 5] [--out profiles/r24_00_waveflow_forward_ab.jsonl]
(one process per batch size; run each under its own time limit)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from cookietts_amd import WaveFlow, _lib, synthetic  # noqa: E402
from oracle import waveflow_oracle as wf  # noqa: E402
from oracle.waveglow_oracle import fold_weightnorm  # noqa: E402


def dense_weights(sd, cfg, dev):
    wn = cfg["WN_config"]

    def w(name):
        if name + ".weight" in sd:
            return torch.from_numpy(np.asarray(sd[name + ".weight"], np.float32)).to(dev)
        return torch.from_numpy(fold_weightnorm(sd[name + ".weight_g"], sd[name + ".weight_v"]).astype(np.float32)).to(dev)

    def b(name):
        return torch.from_numpy(np.asarray(sd[name + ".bias"], np.float32)).to(dev)
    out = []
    for k in range(cfg["n_flows"]):
        p = f"WN.{k}.WN"
        n = range(wn["n_layers"])
        out.append(dict(start=(w(p + ".start"), b(p + ".start")), cond=(w(p + ".cond_layers.0"), b(p + ".cond_layers.0")),
                        ins=[(w(f"{p}.in_layers.{i}"), b(f"{p}.in_layers.{i}")) for i in n],
                        rs=[(w(f"{p}.res_skip_layers.{i}"), b(f"{p}.res_skip_layers.{i}")) for i in n],
                        end=(w(p + ".end"), b(p + ".end"))))
    return out


@torch.no_grad()
def torch_forward(W, cfg, mel, audio):
    """efficient_model_ax.py:225-277 + efficient_modules.py:28-40 + glow_ax.py:556-635 (no queues) for config 4's options."""
    wn = cfg["WN_config"]
    G, C, nl, kh = cfg["n_group"], wn["n_channels"], wn["n_layers"], wn["kernel_size_h"]
    B, T = audio.shape
    L = T // G
    a = audio.view(B, L, G).transpose(1, 2)
    for k, f in enumerate(W):
        cond = F.interpolate(F.conv1d(mel, *f["cond"]), size=L, mode='linear', align_corners=True)
        x = F.conv2d(a[:, None, :-1], *f["start"])
        out = None
        for i in range(nl):
            d = 2 ** i
            u = F.conv2d(F.pad(x, (0, 0, kh - 1, 0)), *f["ins"][i], dilation=(1, d), padding=(0, d * (wn["kernel_size_w"] // 2)))
            u = u + cond[:, 2 * C * i:2 * C * (i + 1), None, :]
            act = torch.tanh(u[:, :C]) * torch.sigmoid(u[:, C:])
            rs = F.conv2d(act, *f["rs"][i])
            if i < nl - 1:
                x = x + rs[:, :C]
                skip = rs[:, C:]
            else:
                skip = rs
            out = skip if out is None else out + skip
        e = F.conv2d(out, *f["end"])
        a = torch.cat((a[:, :1], a[:, 1:] * e[:, 0].exp() + e[:, 1]), dim=1)
        a = a[:, wf.permutation(k, G)]
    return a.transpose(1, 2).contiguous().view(B, T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, required=True)
    ap.add_argument("--frames", type=int, default=900)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2, help="rounds over all arms, run like the timed ones, whose times are dropped")
    ap.add_argument("--out", default=os.path.join("profiles", "r24_00_waveflow_forward_ab.jsonl"))
    args = ap.parse_args()
    cfg = synthetic.WAVEFLOW_CONFIGS["full"]
    wn = cfg["WN_config"]
    assert cfg["channel_mixing"].lower().startswith("permute") and not cfg["mix_first"] and cfg["n_early_every"] > cfg["n_flows"]
    assert wn.get("gated_unit", "GTU") == "GTU" and not wn.get("seperable_conv") and not cfg.get("preempthasis")
    sd = synthetic.waveflow_state_dict(cfg, seed=1234)
    m = WaveFlow(**cfg)
    m.load_state_dict(synthetic.to_torch(sd))
    m = m.cuda().eval()
    m_inv = WaveFlow(**cfg)               # its own instance: a model keeps ONE workspace geometry live, and the arms alternate
    m_inv.load_state_dict(synthetic.to_torch(sd))
    m_inv = m_inv.cuda().eval()
    dev = torch.device("cuda")
    B, Fr, hop = args.batch, args.frames, cfg["hop_length"]
    mel = torch.from_numpy(synthetic.synthetic_mel(B, Fr, seed=7)).to(dev)
    melp = F.pad(mel, (0, 1))
    audio = (0.3 * torch.from_numpy(np.random.default_rng(11).standard_normal((B, Fr * hop)).astype(np.float32))).to(dev)
    z_in = (0.6 * torch.from_numpy(np.random.default_rng(12).standard_normal((B, Fr * hop)).astype(np.float32))).to(dev)
    W = dense_weights(sd, cfg, dev)
    codes = {}

    def knob(on):
        if on:
            os.environ["CTTS_WF_FWD_ROWWISE"] = "1"
        else:
            os.environ.pop("CTTS_WF_FWD_ROWWISE", None)
        _lib.tuning_reload()
        assert _lib.tuning_active("CTTS_WF_FWD_ROWWISE") == on

    def fwd(rowwise):
        def run():
            knob(rowwise)
            out = m.forward(melp, audio)[0]
            codes["forward_rowwise" if rowwise else "forward"] = _lib.lib().ctts_last_gemm_loop()
            return out
        return run
    arms = {"forward": fwd(False), "forward_rowwise": fwd(True),
            "infer_from_noise": lambda: m_inv.infer_from_noise(mel, z_in, return_CPU=False),
            "torch_conv2d": lambda: torch_forward(W, cfg, melp, audio)}
    first = {name: run() for name, run in arms.items()}                     # warm-up (packs, allocates, tunes)
    torch.cuda.synchronize()
    ref = first["forward"].double()

    def rms_rel(x):
        return float(((x.double() - ref) ** 2).mean().sqrt() / (ref ** 2).mean().sqrt())
    agree = {"forward_rowwise": rms_rel(first["forward_rowwise"]), "torch_conv2d": rms_rel(first["torch_conv2d"])}
    assert codes["forward"] & 256 and not codes["forward_rowwise"] & 256, codes
    del first                                                               # (held every arm's output alive)
    times = {name: [] for name in arms}
    for r in range(args.warmup + args.reps):                                # the warm-up rounds run exactly as the timed ones, and are dropped
        for name, run in arms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            run()
            t1.record()
            t1.synchronize()
            if r >= args.warmup:
                times[name].append(t0.elapsed_time(t1))
    knob(False)
    rec = dict(what="waveflow_forward_ab", config="full", batch=B, frames=Fr, reps=args.reps, warmup_rounds_dropped=args.warmup, loop_codes=codes, z_rms_rel_vs_forward=agree,
               workspace_bytes=dict(forward=int(sum(v.numel() * 4 for v in m._ws.values())),
                                    inverse=int(sum(v.numel() * 4 for v in m_inv._ws.values()))))
    for name, t in times.items():
        rec[name] = dict(median_ms=float(np.median(t)), spread_ms=float(max(t) - min(t)), all_ms=[round(v, 3) for v in t])

    def claim(a, b):
        d = rec[b]["median_ms"] - rec[a]["median_ms"]
        ok = abs(d) >= 10 * max(rec[a]["spread_ms"], rec[b]["spread_ms"])
        return dict(faster=(a if d > 0 else b) if ok else None, claimed=bool(ok), diff_ms=float(d))
    rec["forward_vs_rowwise"] = claim("forward", "forward_rowwise")
    rec["forward_vs_infer"] = claim("forward", "infer_from_noise")
    rec["forward_vs_torch"] = claim("forward", "torch_conv2d")
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
