"""Vocoder validation score: this package's one-call device path against the reference's shape of code on the same GPU.

Shapes: `validate` - the one of `_4_mtw/waveglow/train.py` validate(): 9 files of up to 3 s at 48 kHz, windows (1200, 2400), hop 600,
160 mels; `nv_real` - HiFi-GAN's framing, 1024 / 1024 / 256, 80 mels, 22.05 kHz, B = 16, T = 8192.  Arms, alternated in one process
(dropped warm-up rounds first, `--reps` repetitions each, HOST clock around work that ends in a synchronise - the reference arm's cost is
its host reads - medians and spreads):

  a  device:     cookietts_amd.MelSpectrogramError(...)(pred, gt, pred_lengths=, gt_lengths=) - ONE call, ONE device-to-host copy
  b  torch GPU:  `per_file_loop` below, the shape of train.py:258-278: per file and per window this package's
                 `TacotronSTFT.mel_spectrogram` on both signals (the HIP STFT; it carries the reference's two min / max assertions, one
                 host read each), the crop, `MSELoss` / `L1Loss` and two `.item()` reads.  Under "nv" framing this package has no
                 nvSTFT class: arm b is `torch.stft` + matmul + log per item with one `.item()` per item (hifigan/train.py:208-210).

The reference tree is not imported.  Every line also records what leaves the device per call in either arm, COUNTED in one extra call of
each arm under `count_d2h` (every `.cpu()`, `.item()` and `.tolist()` of a device tensor).  Arm b is the per-file shape of the reference,
not a batched rewrite: the ratio is against that shape of code.  A ratio is claimed only where the difference is at least 10 x the larger
arm's spread.

usage: python scripts/debug/mel_error_ab.py [--reps 5] [--warmup 2] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from cookietts_amd import MelSpectrogramError, TacotronSTFT  # noqa: E402
from cookietts_amd.audio import slaney_mel_filterbank  # noqa: E402


class count_d2h:
    """Counts the device-to-host reads made through `Tensor.cpu`, `Tensor.item` and `Tensor.tolist` while it is entered."""

    def __enter__(self):
        self.copies, self.bytes, self._saved = 0, 0, {}
        for name in ("cpu", "item", "tolist"):
            self._saved[name] = orig = getattr(torch.Tensor, name)

            def counted(t, *args, _orig=orig, **kw):
                if t.is_cuda:
                    self.copies += 1
                    self.bytes += t.numel() * t.element_size()
                return _orig(t, *args, **kw)
            setattr(torch.Tensor, name, counted)
        return self

    def __exit__(self, *exc):
        for name, orig in self._saved.items():
            setattr(torch.Tensor, name, orig)
        return False


def make_audio(lengths, sr, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    B, T = len(lengths), max(lengths)
    t = torch.arange(T, device=dev)[None, :] / sr
    f = 100 + 3000 * torch.rand(B, 3, generator=g, device=dev)
    tone = sum(a * torch.sin(2 * np.pi * f[:, i:i + 1] * t) for i, a in enumerate((0.3, 0.2, 0.1)))
    gt = (tone + 0.05 * torch.randn(B, T, generator=g, device=dev)).clamp(-0.95, 0.95)
    pred = (0.9 * tone + 0.08 * torch.randn(B, T, generator=g, device=dev)).clamp(-0.95, 0.95)
    mask = torch.arange(T, device=dev)[None, :] < torch.tensor(lengths, device=dev)[:, None]
    return gt * mask, pred * mask


@torch.no_grad()
def per_file_loop(STFTs, pred, gt, lengths):
    """train.py:258-278, 294-295 -> (average_MSE, average_MAE)."""
    total_MAE = total_MSE = total = 0
    for b, n in enumerate(lengths):
        audio = gt[b, :n].unsqueeze(0)
        audio_waveglow = pred[b, :n].unsqueeze(0).clamp(min=-0.999, max=0.999)
        audio_waveglow = torch.nan_to_num(audio_waveglow, nan=0.0)
        for STFT in STFTs:
            mel_GT = STFT.mel_spectrogram(audio)
            mel_waveglow = STFT.mel_spectrogram(audio_waveglow)[:, :, :mel_GT.shape[-1]]
            MSE = torch.nn.MSELoss()(mel_waveglow, mel_GT).item()
            MAE = torch.nn.L1Loss(reduction='none')(mel_waveglow, mel_GT).mean().item()
            total_MAE += MAE
            total_MSE += MSE
            total += 1
    return total_MSE / total, total_MAE / total


@torch.no_grad()
def nv_loop(fb, window, n_fft, hop, pred, gt, lengths):
    """hifigan/train.py:205-223 per item with the framing of nvSTFT.py:92-101 -> mean l1."""
    def get_mel(y):
        pad = int((n_fft - hop) / 2)
        y = torch.nn.functional.pad(y.unsqueeze(1), (pad, pad), mode='reflect').squeeze(1)
        spec = torch.stft(y, n_fft, hop_length=hop, win_length=n_fft, window=window, center=False, return_complex=True)
        spec = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
        return torch.log(torch.clamp(torch.matmul(fb, spec), min=1e-5))
    val_err_tot = 0
    for b, n in enumerate(lengths):
        y_mel = get_mel(gt[b, :n].unsqueeze(0))
        val_err_tot += torch.nn.functional.l1_loss(y_mel, get_mel(pred[b, :n].unsqueeze(0))).item()
    return val_err_tot / len(lengths)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for name in ("validate", "nv_real"):
        if name == "validate":
            sr, windows, hop, n_mel, fmax = 48000, (1200, 2400), 600, 160, 16000.0
            lengths = [144000, 131237, 120000, 98765, 143999, 72000, 110400, 86431, 139800]      # 9 files of up to 3 s
            metric = MelSpectrogramError(windows, hop, sr, n_mel, 0.0, fmax).to(dev)
            STFTs = [TacotronSTFT(w, hop, w, n_mel, sr, 0.0, fmax).to(dev) for w in windows]
            gt, pred = make_audio(lengths, sr, 28, dev)
            arm_b = lambda: per_file_loop(STFTs, pred, gt, lengths)
            agree = lambda ra, rb: abs(ra["average_MSE"] - rb[0]) / rb[0]
        else:
            sr, windows, hop, n_mel, fmax = 22050, (1024,), 256, 80, 8000.0
            lengths = [8192] * 16
            metric = MelSpectrogramError(windows, hop, sr, n_mel, 0.0, fmax, framing="nv").to(dev)
            fb = torch.from_numpy(slaney_mel_filterbank(sr, 1024, n_mel, 0.0, fmax)).to(dev)
            window = torch.hann_window(1024, device=dev)
            gt, pred = make_audio(lengths, sr, 29, dev)
            arm_b = lambda: nv_loop(fb, window, 1024, hop, pred, gt, lengths)
            agree = lambda ra, rb: abs(ra["l1"][0] - rb) / rb
        arms = {"a_device": lambda: metric(pred, gt, pred_lengths=lengths, gt_lengths=lengths, sanitize=(name == "validate")),
                "b_torch_gpu": arm_b}
        for _ in range(a.warmup):                                                           # dropped
            res = {k: fn() for k, fn in arms.items()}
        torch.cuda.synchronize()
        d2h = {}
        for k, fn in arms.items():                                                          # counted, not timed
            with count_d2h() as c:
                fn()
            d2h[k] = {"copies": c.copies, "bytes": c.bytes}
        wall = {k: [] for k in arms}
        for _ in range(a.reps):                                                             # arms alternated
            for k, fn in arms.items():
                wall[k].append(timed(fn)[0])
        med = {k: float(np.median(v)) for k, v in wall.items()}
        spread = {k: float(max(v) - min(v)) for k, v in wall.items()}
        d = med["b_torch_gpu"] - med["a_device"]
        claimed = bool(abs(d) >= 10 * max(spread.values()))
        line = dict(row="mel_error_ab", shape=name, batch=len(lengths), windows=list(windows), hop=hop, n_mel=n_mel, sampling_rate=sr,
                    reps=a.reps, warmup=a.warmup, clock="host, around work that ends in a synchronise",
                    a_device_wall_ms=[round(x, 3) for x in wall["a_device"]], b_torch_gpu_wall_ms=[round(x, 3) for x in wall["b_torch_gpu"]],
                    median_ms={k: round(v, 3) for k, v in med.items()}, spread_ms={k: round(v, 3) for k, v in spread.items()},
                    b_minus_a_ms=round(d, 3), difference_at_least_10x_spread=claimed,
                    b_over_a=round(med["b_torch_gpu"] / med["a_device"], 2) if claimed else "no difference claimed",
                    d2h_counted_per_call=d2h, baseline_shape="per-file, per-window loop with .item() reads (not batched)",
                    rel_diff_of_the_two_arms=agree(res["a_device"], res["b_torch_gpu"]))
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
