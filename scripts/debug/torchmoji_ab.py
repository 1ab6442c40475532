"""The torchMoji style vector: this package's device path against the same arithmetic in plain PyTorch, on the host and on the GPU.

Shapes: B = 1 and 4 sentences, T = 20 and 130 tokens (130 is the server's maxlen), V = 50000, synthetic weights
(`synthetic.torchmoji_state_dict`).  Row 0 is T tokens long, the others are ragged.  Arms, alternated in one process (warm-up
first, `--reps` repetitions each):

  a  device:      cookietts_amd.TorchMoji, host tokens in, device features out (2 T + 12 launches and two small copies per call)
  b  host:        the model restated below in plain PyTorch ops on the CPU with the machine's thread setting, plus the
                  `.cuda()` copy of the features - what text2speech.py:497-509 does today with the reference module
  c  torch GPU:   the same plain-PyTorch restatement with its tensors on the GPU (PyTorch-ROCm kernels)

The reference tree is not imported: `PlainTorchMoji` restates model_def.py:169-253 / lstm.py:330-357 / attlayer.py:48-66 (rows
stepped under a mask instead of packed; the same sums).  Device arms are timed with device events on the current stream and
with the wall clock around a device synchronise; the host arm with the wall clock, copy included.

usage: python scripts/debug/torchmoji_ab.py [--reps 5] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from cookietts_amd import TorchMoji, synthetic  # noqa: E402

NB_TOKENS = 50000


def hard_sigmoid(x):
    return torch.clamp(0.2 * x + 0.5, 0.0, 1.0)


class PlainTorchMoji:
    def __init__(self, sd, device):
        self.sd = {k: torch.from_numpy(np.asarray(v)).to(device) for k, v in sd.items()}
        self.device = device

    def _direction(self, x, lens, p, sfx, reverse):
        w_ih, w_hh, b_ih, b_hh = (self.sd[f"{p}.{n}_l0{sfx}"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
        B, T, _ = x.shape
        H = w_hh.shape[1]
        xp = torch.zeros(B, T + 1, 4 * H, device=x.device)              # slot T: where an idle row reads and writes
        xp[:, :T] = x @ w_ih.T + (b_ih + b_hh)
        out = torch.zeros(B, T + 1, H, device=x.device)
        h = torch.zeros(B, H, device=x.device)
        c = torch.zeros(B, H, device=x.device)
        rows = torch.arange(B, device=x.device)
        w_hh_t = w_hh.T.contiguous()
        for step in range(T):
            active = step < lens
            tb = torch.where(active, lens - 1 - step if reverse else torch.full_like(lens, step), torch.full_like(lens, T))
            g = xp[rows, tb] + h @ w_hh_t
            i, f, gg, o = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
            c2 = hard_sigmoid(f) * c + hard_sigmoid(i) * torch.tanh(gg)
            h2 = hard_sigmoid(o) * torch.tanh(c2)
            act = active[:, None]
            c = torch.where(act, c2, c)
            h = torch.where(act, h2, h)
            out[rows, tb] = h2
        return out[:, :T]

    @torch.no_grad()
    def __call__(self, tokens):
        """tokens: numpy [B, T]; lengths and the trim on the host as in the reference; features on ``self.device``."""
        tok = np.asarray(tokens).astype(np.int64)
        nz = tok != 0
        lens_np = tok.shape[1] - np.argmax(nz[:, ::-1], axis=1)
        tok = tok[:, :int(lens_np.max())]
        T = tok.shape[1]
        tok_t = torch.from_numpy(np.ascontiguousarray(tok)).to(self.device)
        lens = torch.from_numpy(lens_np.astype(np.int64)).to(self.device)
        valid = (torch.arange(T, device=self.device)[None, :] < lens[:, None])
        x = torch.tanh(self.sd["embed.weight"][tok_t]) * valid[:, :, None]
        o0 = torch.cat([self._direction(x, lens, "lstm_0", "", False), self._direction(x, lens, "lstm_0", "_reverse", True)], dim=2)
        o0 = o0 * valid[:, :, None]
        o1 = torch.cat([self._direction(o0, lens, "lstm_1", "", False), self._direction(o0, lens, "lstm_1", "_reverse", True)], dim=2)
        feat = torch.cat([o1 * valid[:, :, None], o0, x], dim=2)
        logits = feat @ self.sd["attention_layer.attention_vector"]
        w = (logits - logits.max()).exp() * valid
        att = w / w.sum(dim=1, keepdim=True)
        return (feat * att[:, :, None]).sum(dim=1)


def case_tokens(B, T, seed):
    rng = np.random.default_rng(seed)
    tok = np.zeros((B, T), np.uint16)
    lens = [T] + [int(n) for n in rng.integers(max(1, T // 2), T + 1, size=B - 1)]
    for b, n in enumerate(lens):
        tok[b, :n] = rng.integers(1, NB_TOKENS, size=n)
    return tok, lens


def timed_device(fn):
    """(device-event ms, wall ms around a synchronise, result)."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out


def timed_host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sd = synthetic.torchmoji_state_dict(NB_TOKENS, seed=21)
    ours = TorchMoji(nb_tokens=NB_TOKENS)
    ours.load_state_dict(synthetic.to_torch(sd))
    ours = ours.cuda().eval()
    plain_cpu, plain_gpu = PlainTorchMoji(sd, torch.device("cpu")), PlainTorchMoji(sd, torch.device("cuda", 0))
    lines = []
    for B in (1, 4):
        for T in (20, 130):
            tok, lens = case_tokens(B, T, 1000 * B + T)
            arms = {"a_device": lambda: ours(tok), "b_host": lambda: plain_cpu(tok).cuda(), "c_torch_gpu": lambda: plain_gpu(tok)}
            res = {k: fn() for k, fn in arms.items()}                                       # warm-up, and the results compared
            torch.cuda.synchronize()
            diff_b = float((res["a_device"] - res["b_host"]).abs().max())
            diff_c = float((res["a_device"] - res["c_torch_gpu"]).abs().max())
            ev = {"a_device": [], "c_torch_gpu": []}
            wall = {k: [] for k in arms}
            for _ in range(a.reps):                                                         # arms alternated
                for k, fn in arms.items():
                    if k == "b_host":
                        wall[k].append(timed_host(fn)[0])
                    else:
                        e, w, _ = timed_device(fn)
                        ev[k].append(e)
                        wall[k].append(w)
            # the figure of each arm: device events for the device arms, wall clock (copy included) for the host arm
            fig = {"a_device": np.array(ev["a_device"]), "b_host": np.array(wall["b_host"]), "c_torch_gpu": np.array(ev["c_torch_gpu"])}
            med = {k: float(np.median(v)) for k, v in fig.items()}
            spread = {k: float(v.max() - v.min()) for k, v in fig.items()}
            line = dict(row="torchmoji_ab", batch=B, T=T, lengths=lens, nb_tokens=NB_TOKENS, reps=a.reps,
                        launches_per_call_a=2 * T + 12, torch_threads=torch.get_num_threads(),
                        a_device_event_ms=[round(x, 3) for x in ev["a_device"]], a_device_wall_ms=[round(x, 3) for x in wall["a_device"]],
                        b_host_wall_ms=[round(x, 3) for x in wall["b_host"]],
                        c_torch_gpu_event_ms=[round(x, 3) for x in ev["c_torch_gpu"]],
                        c_torch_gpu_wall_ms=[round(x, 3) for x in wall["c_torch_gpu"]],
                        median_ms={k: round(v, 3) for k, v in med.items()}, spread_ms={k: round(v, 3) for k, v in spread.items()},
                        max_abs_diff_a_vs_b=diff_b, max_abs_diff_a_vs_c=diff_c)
            for other in ("b_host", "c_torch_gpu"):
                larger = max(spread["a_device"], spread[other])
                d = med[other] - med["a_device"]
                line[f"{other}_minus_a_ms"] = round(d, 3)
                line[f"{other}_difference_exceeds_10x_spread"] = bool(abs(d) > 10 * larger)
                line[f"{other}_over_a"] = round(med[other] / med["a_device"], 2)
            lines.append(line)
            print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
