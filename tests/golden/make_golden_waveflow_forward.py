#!/usr/bin/env python3
"""Fixtures of the WaveFlow analysis direction, by RUNNING THE REFERENCE ITSELF: tests/golden/waveflow_forward_<name>.npz.

Run in the build container only (``/root/reference`` does not exist on the GPU box):

    python tests/golden/make_golden_waveflow_forward.py [name ...]

For every case of tests/waveflow_forward_restatement.CASES it runs the reference's own ``efficient_model_ax.WaveGlow.forward`` and
``efficient_loss.WaveGlowLoss`` on the CPU (fp32, under ``torch.no_grad()``) on the infer fixture's mel padded by one frame and its
``inverse_full``, and the numpy restatement in float64 and in float32, and stores data only:

  z_ref, logdet_ref, logdet_w_sum_ref, log_s_sum_ref, loss_ref   the reference's tuple and loss (at the infer fixture's sigma)
  z_f64_delta16 / _scale, log_s_sum_f64_...    the float64 restatement's z and log_s_sum as 16-bit deltas against the reference
  log_s_f32, log_s_f64_delta16 / _scale        its log_s: rounded to fp32 + the 16-bit delta to that rounding
  sums_f64, logdet_w_f64, logdet_f64, loss_f64 its per-item sums, log_det_W_k, logdet and loss
  z_e32 [G], log_s_e32 [S], log_s_sum_e32, logdet_e32, loss_e32   the fp32 restatement's L-inf distances from float64 (per latent
                                               row where there are rows) - what the GPU bounds are made of

Weights and inputs are not stored (cookietts_amd.synthetic and the infer fixtures).
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, "/root/reference")

import waveflow_core_f64_restatement as wcr  # noqa: E402
import waveflow_forward_restatement as fr  # noqa: E402
from make_golden import _ref_waveflow  # noqa: E402


def rms_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def make(name):
    from CookieTTS._4_mtw.waveglow import efficient_loss
    torch.set_num_threads(8)
    cfg, sd, melp, audio, ids, sigma, z_infer = fr.case_inputs(name)
    model = _ref_waveflow(copy.deepcopy(cfg), sd)
    G = cfg["n_group"]
    with torch.no_grad():
        wave = torch.from_numpy(audio.copy())
        out = model(torch.from_numpy(melp.copy()), wave, speaker_ids=None if ids is None else torch.from_numpy(ids))
        loss_ref = float(efficient_loss.WaveGlowLoss(sigma)(out))
    z_ref, logdet_ref, ldw_ref, lss_ref = (np.asarray(t.numpy(), np.float32) for t in out)
    r64 = fr.forward(sd, cfg, melp, audio, ids, np.float64)
    r32 = fr.forward(sd, cfg, melp, audio, ids, np.float32)
    loss64, _ = fr.loss(r64["z"], r64["logdet"], sigma)
    loss32, _ = fr.loss(r32["z"], r32["logdet"], sigma)
    print(f"[golden] waveflow forward {name}: reference z vs infer fixture z {rms_rel(z_ref, z_infer):.2e}; restatement vs reference "
          f"z {rms_rel(r64['z'], z_ref):.2e}, logdet {np.abs(r64['logdet'] - logdet_ref).max():.2e}, loss {abs(loss64 - loss_ref):.2e}")
    zd, zs = fr.pack_delta(r64["z"], z_ref)
    ls32 = r64["log_s"].astype(np.float32)
    ld, ls = fr.pack_delta(r64["log_s"], ls32)
    sd_, ss = fr.pack_delta(r64["log_s_sum"], lss_ref)
    np.savez_compressed(
        fr.case_path(name), z_ref=z_ref, logdet_ref=logdet_ref, logdet_w_sum_ref=ldw_ref, log_s_sum_ref=lss_ref,
        loss_ref=np.float64(loss_ref), sigma=np.float32(sigma),
        z_f64_delta16=zd, z_f64_scale=zs, log_s_f32=ls32, log_s_f64_delta16=ld, log_s_f64_scale=ls,
        log_s_sum_f64_delta16=sd_, log_s_sum_f64_scale=ss,
        sums_f64=r64["sums"], logdet_w_f64=r64["logdet_w"], logdet_f64=r64["logdet"], loss_f64=np.float64(loss64),
        z_e32=fr.row_linf(wcr.rows_of(r32["z"], G), wcr.rows_of(r64["z"], G)), log_s_e32=fr.row_linf(r32["log_s"], r64["log_s"]),
        log_s_sum_e32=np.abs(r32["log_s_sum"].astype(np.float64) - r64["log_s_sum"]).max(),
        logdet_e32=np.abs(r32["logdet"].astype(np.float64) - r64["logdet"]).max(), loss_e32=np.float64(abs(loss32 - loss64)))
    print(f"          -> {os.path.getsize(fr.case_path(name)) / 1024:.0f} KiB")


if __name__ == "__main__":
    for n in (sys.argv[1:] or fr.CASES):
        make(n)
