"""DTW: this package's one-launch device path against the reference's shape of code on the same GPU.

Shapes: `validate` - the one of `_4_mtw/waveglow/train.py` validate(): 9 items of up to 240 frames, 160 channels, `(scale_factor, range_) =
(8, 5)`; `gta` - a GTA batch for HiFi-GAN: 16 x 80 x 900, `(5, 3)`.  Arms, alternated in one process (dropped warm-up rounds first,
`--reps` repetitions each, device events around each arm, medians and spreads):

  a  device:     cookietts_amd.DTW(pred, target, s, r, lengths=) - ONE launch for the batch
  b  torch GPU:  `per_item_loop` below, the shape of `mel2samp.py:98-118` restated from its equations: per item pad, `F.interpolate`,
                 `s * r` strided slices, and per slice two `l1_loss(reduction='none').sum(1)` and one `where`.

The reference tree is not imported.  Arm b is the per-item shape of the reference (eager, not scripted or batched): the ratio is against
that shape of code.  A ratio is claimed only where the difference is at least 10 x the larger arm's spread.

usage: python scripts/debug/dtw_ab.py [--reps 5] [--warmup 2] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from cookietts_amd import DTW  # noqa: E402


def make_mels(B, C, T, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    walk = torch.randn(B, C, 1, generator=g, device=dev) + 0.3 * torch.cumsum(torch.randn(B, C, T + 2, generator=g, device=dev), dim=2)
    target = walk[:, :, 1:T + 1].contiguous()
    pred = (0.6 * walk[:, :, 1:T + 1] + 0.4 * walk[:, :, 2:T + 2] + 0.05 * torch.randn(B, C, T, generator=g, device=dev)).contiguous()
    return pred, target


@torch.no_grad()
def per_item_loop(batch_pred, batch_target, scale_factor, range_, lengths):
    out = batch_pred.clone()
    for i, n in enumerate(lengths):
        pred, target = batch_pred[i:i + 1, :, :n], batch_target[i:i + 1, :, :n]
        padded = F.pad(pred, (range_ // 2, range_ // 2))
        expanded = F.interpolate(padded, scale_factor=float(scale_factor), mode='linear', align_corners=False)
        best = pred.clone()
        for j in range(scale_factor * range_):
            cand = expanded[:, :, j::scale_factor][:, :, :n]
            new_l1 = F.l1_loss(cand, target, reduction='none').sum(dim=1, keepdim=True)
            old_l1 = F.l1_loss(best, target, reduction='none').sum(dim=1, keepdim=True)
            best = torch.where(new_l1 < old_l1, cand, best)
        out[i:i + 1, :, :n] = best
    return out


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for name in ("validate", "gta"):
        if name == "validate":
            C, (s, r) = 160, (8, 5)
            lengths = [240, 219, 200, 165, 239, 120, 184, 144, 233]
        else:
            C, (s, r) = 80, (5, 3)
            lengths = [900] * 16
        pred, target = make_mels(len(lengths), C, max(lengths), 32, dev)
        arms = {"a_device": lambda: DTW(pred, target, s, r, lengths=lengths),
                "b_torch_gpu": lambda: per_item_loop(pred, target, s, r, lengths)}
        for _ in range(a.warmup):                                                           # dropped
            res = {k: fn() for k, fn in arms.items()}
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(a.reps):                                                             # arms alternated
            for k, fn in arms.items():
                ms[k].append(timed(fn)[0])
        med = {k: float(np.median(v)) for k, v in ms.items()}
        spread = {k: float(max(v) - min(v)) for k, v in ms.items()}
        d = med["b_torch_gpu"] - med["a_device"]
        claimed = bool(abs(d) >= 10 * max(spread.values()))
        differ = (res["a_device"] != res["b_torch_gpu"]).any(dim=1)
        line = dict(row="dtw_ab", shape=name, batch=len(lengths), channels=C, frames=max(lengths), scale_factor=s, range=r, reps=a.reps,
                    warmup=a.warmup, clock="device events around each arm",
                    a_device_ms=[round(x, 4) for x in ms["a_device"]], b_torch_gpu_ms=[round(x, 3) for x in ms["b_torch_gpu"]],
                    median_ms={k: round(v, 4) for k, v in med.items()}, spread_ms={k: round(v, 4) for k, v in spread.items()},
                    b_minus_a_ms=round(d, 3), difference_at_least_10x_spread=claimed,
                    b_over_a=round(med["b_torch_gpu"] / med["a_device"], 1) if claimed else "no difference claimed",
                    baseline_shape="per-item loop, s * r slices with l1_loss / sum / where each (eager, not batched)",
                    frames_where_the_arms_differ=int(differ.sum()), frames_compared=int(differ.numel()),
                    max_abs_diff_of_the_two_arms=float((res["a_device"] - res["b_torch_gpu"]).abs().max()))
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
