#!/usr/bin/env python3
"""Goldens of the vocoder validation score: the reference's own ``TacotronSTFT`` (utils/audio/stft.py) driven as
``_4_mtw/waveglow/train.py:258-278`` drives it, per file and per window, on the CPU in float32 - ``validate()`` itself reads files
and calls ``.cuda()``, so it cannot be called.  The "nv" cases run the reference's ``hifigan/nvSTFT.py`` ``STFT.get_mel`` and
``F.l1_loss`` as ``hifigan/train.py:208-210`` does, per item (so each item is reflect-padded at its own end).

Run in the build container only (it imports the reference):

    python tests/golden/make_golden_mel_error.py

Data only: per case ``mel_error_<case>.npz`` holds the audio pairs (``gt``, ``pred`` float32, zero beyond the lengths), the lengths, the
reference's float32 per-pair ``mse32`` / ``mae32`` [B, W], ``n_frames`` [B, W], ``average_MSE32`` / ``average_MAE32`` and ``l1_32`` [W]
(sum of the reference's ``L1Loss(reduction='sum')`` over items / sum of the counts).

Stand-ins that live only here: ``make_golden.py``'s librosa modules; empty ``soundfile`` module; ``torch.stft`` wrapped to pass
``return_complex=True`` and hand back the real view the reference's ``spec.pow(2).sum(-1)`` expects.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (puts the repository and the reference on sys.path)
import mel_error_restatement as mr  # noqa: E402


def tacotron_case(c, gt, pred):
    mg._stub_audio_deps()
    from CookieTTS.utils.audio.stft import TacotronSTFT
    wls = c.get("win_lengths", c["windows"])
    STFTs = [TacotronSTFT(filter_length=n, hop_length=c["hop_length"], win_length=wl, n_mel_channels=c["n_mel_channels"],
                          sampling_rate=c["sampling_rate"], mel_fmin=c["mel_fmin"], mel_fmax=c["mel_fmax"])
             for n, wl in zip(c["windows"], wls)]
    B, W = len(c["gt_lengths"]), len(STFTs)
    mse, mae, sae, nf = (np.zeros((B, W)) for _ in range(4))
    total_MAE = total_MSE = total = 0
    for b in range(B):
        audio = torch.from_numpy(gt[b, :c["gt_lengths"][b]].copy())
        audio_waveglow = torch.from_numpy(pred[b, :c["pred_lengths"][b]].copy())
        audio = audio.squeeze().unsqueeze(0)                                                              # :258
        audio_waveglow = audio_waveglow.squeeze().unsqueeze(0).clamp(min=-0.999, max=0.999)               # :259
        audio_waveglow[torch.isnan(audio_waveglow) | torch.isinf(audio_waveglow)] = 0.0                   # :260
        for j, STFT in enumerate(STFTs):                                                                  # :263
            mel_GT = STFT.mel_spectrogram(audio)
            mel_waveglow = STFT.mel_spectrogram(audio_waveglow)[:, :, :mel_GT.shape[-1]]
            MSE = (torch.nn.MSELoss()(mel_waveglow, mel_GT)).item()
            MAE_spec = torch.nn.L1Loss(reduction='none')(mel_waveglow, mel_GT)
            MAE = (MAE_spec.mean()).item()
            total_MAE += MAE
            total_MSE += MSE
            total += 1
            mse[b, j], mae[b, j], nf[b, j] = MSE, MAE, mel_GT.shape[-1]
            sae[b, j] = torch.nn.L1Loss(reduction='sum')(mel_waveglow, mel_GT).item()
    return mse, mae, sae, nf, total_MSE / total, total_MAE / total


def nv_case(c, gt, pred):
    mg._stub_audio_deps()
    sys.modules.setdefault("soundfile", types.ModuleType("soundfile"))
    if not hasattr(sys.modules["librosa"], "core"):
        sys.modules["librosa"].core = types.SimpleNamespace(resample=None)
    real_stft = torch.stft

    def stft(*a, **kw):
        kw["return_complex"] = True
        return torch.view_as_real(real_stft(*a, **kw))
    torch.stft = stft
    try:
        from CookieTTS._4_mtw.hifigan.nvSTFT import STFT
        (n,), (wl,) = c["windows"], c["win_lengths"]
        fn = STFT(sr=c["sampling_rate"], n_mels=c["n_mel_channels"], n_fft=n, win_size=wl, hop_length=c["hop_length"],
                  fmin=c["mel_fmin"], fmax=c["mel_fmax"])
        B = len(c["gt_lengths"])
        mse, mae, sae, nf = (np.zeros((B, 1)) for _ in range(4))
        gt_mels = []
        for b in range(B):
            y = torch.from_numpy(gt[b, :c["gt_lengths"][b]].copy()).unsqueeze(0)
            y_g_hat = torch.from_numpy(pred[b, :c["pred_lengths"][b]].copy()).unsqueeze(0)
            y_mel = fn.get_mel(y)
            y_g_hat_mel = fn.get_mel(y_g_hat)[:, :, :y_mel.shape[-1]]
            mae[b, 0] = torch.nn.functional.l1_loss(y_mel, y_g_hat_mel).item()                            # hifigan/train.py:210
            mse[b, 0] = torch.nn.functional.mse_loss(y_mel, y_g_hat_mel).item()
            sae[b, 0] = torch.nn.functional.l1_loss(y_mel, y_g_hat_mel, reduction='sum').item()
            nf[b, 0] = y_mel.shape[-1]
            gt_mels.append(y_mel[0].numpy())
    finally:
        torch.stft = real_stft
    return mse, mae, sae, nf, float(np.mean(mse)), float(np.mean(mae)), np.stack(gt_mels)


def make(case):
    c = mr.CASES[case]
    gt, pred = mr.signals(case)
    extra = {}
    if c["framing"] == "nv":
        mse, mae, sae, nf, amse, amae, gt_mel = nv_case(c, gt, pred)
        extra["gt_mel32"] = gt_mel.astype(np.float32)
    else:
        mse, mae, sae, nf, amse, amae = tacotron_case(c, gt, pred)
    l1 = sae.sum(axis=0) / (nf * c["n_mel_channels"]).sum(axis=0)
    r64 = mr.score(pred, gt, c["pred_lengths"], c["gt_lengths"], np.float64, **mr.ctor_args(case))
    rel = np.abs(mse - r64["table"][:, :, 4]) / r64["table"][:, :, 4]
    print(f"{case}: reference float32 vs float64 restatement, MSE relative {rel.min():.1e} .. {rel.max():.1e}; n_frames {nf.tolist()}")
    assert (nf == r64["table"][:, :, 0]).all()
    path = os.path.join(HERE, f"mel_error_{case}.npz")
    np.savez_compressed(path, gt=gt, pred=pred, gt_lengths=np.array(c["gt_lengths"]), pred_lengths=np.array(c["pred_lengths"]),
                        mse32=mse, mae32=mae, sae32=sae, n_frames=nf, average_MSE32=np.float64(amse), average_MAE32=np.float64(amae),
                        l1_32=l1, **extra)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for name in sys.argv[1:] or list(mr.CASES):
        make(name)
