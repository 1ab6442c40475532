#!/usr/bin/env python3
"""Fixtures of the forward (analysis) direction, by RUNNING THE REFERENCE ITSELF: tests/golden/waveglow_forward_<name>.npz.

Run in the build container only (``/root/reference`` does not exist on the GPU box):

    python tests/golden/make_golden_waveglow_forward.py [name ...]

For every case of tests/waveglow_forward_restatement.CASES it runs the reference's own ``glow.WaveGlow.forward`` and
``WaveGlowLoss`` on the CPU (fp32) and the numpy restatement in float64 and in float32, and stores data only:

  z_ref, log_s_ref, log_det_W_ref, loss_ref   the reference's results (log_s concatenated over the flows; loss at the golden's sigma)
  z_f64_delta16 / _scale, log_s_f64_...       the float64 restatement's z and log_s (waveglow_forward_restatement.pack_delta)
  sums_f64, logdet_f64, loss_f64              its per-item sums, log|det W_k| and loss
  z_linf32, log_s_linf32, loss_dist32         the fp32 restatement's distances from float64 - what the GPU bounds are made of
  sigma; wave                                 "full_f9" only: its seeded waveform (the goldens' inputs are read by name)

Weights are not stored (cookietts_amd.synthetic, seeds in the infer fixtures).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, "/root/reference")

import waveglow_f64_restatement as wr  # noqa: E402
import waveglow_forward_restatement as fr  # noqa: E402
from make_golden import _ref_waveglow  # noqa: E402


def rms_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def make(name):
    from CookieTTS._4_mtw.waveglow import glow
    torch.set_num_threads(8)
    extras = {}
    if name == "full_f9":
        extras["wave"] = fr.full_f9_wave()
        np.savez_compressed(fr.case_path(name), **extras)          # case_inputs reads the waveform from the fixture
    cfg, sd, mel, wave, ids, sigma = fr.case_inputs(name)
    model = _ref_waveglow(cfg, sd)
    with torch.no_grad():
        out = model(torch.from_numpy(mel.copy()), torch.from_numpy(wave.copy()),
                    speaker_id=None if ids is None else torch.from_numpy(ids))
        log_det_W_ref = np.array([float(v) for v in out[2]], np.float32)      # (before the loss: it sums INTO out[2][0], glow.py:59)
        loss_ref = glow.WaveGlowLoss(sigma)(out)
    z_ref = out[0].numpy().astype(np.float32)
    log_s_ref = torch.cat(out[1], 1).numpy().astype(np.float32)
    r64 = fr.forward(sd, cfg, mel, wave, ids, np.float64)
    r32 = fr.forward(sd, cfg, mel, wave, ids, np.float32)
    assert r32["z"].dtype == np.float32 and r32["log_s"].dtype == np.float32
    G = cfg["n_group"]
    loss64, loss32 = fr.loss(r64, G, sigma), fr.loss(r32, G, sigma)
    zd, zs = fr.pack_delta(r64["z"], z_ref)
    ld, ls = fr.pack_delta(r64["log_s"], log_s_ref)
    np.savez_compressed(fr.case_path(name), z_ref=z_ref, log_s_ref=log_s_ref, log_det_W_ref=log_det_W_ref,
                        loss_ref=np.float32(loss_ref.item()), z_f64_delta16=zd, z_f64_scale=zs, log_s_f64_delta16=ld,
                        log_s_f64_scale=ls, sums_f64=r64["sums"], logdet_f64=r64["logdet"], loss_f64=np.float64(loss64),
                        z_linf32=np.float64(wr.linf(r32["z"], r64["z"])), log_s_linf32=np.float64(wr.linf(r32["log_s"], r64["log_s"])),
                        loss_dist32=np.float64(abs(loss32 - loss64)), sigma=np.float32(sigma), **extras)
    assert np.array_equal(np.isnan(log_det_W_ref), np.isnan(r64["logdet"])) and np.isnan(loss64) == np.isnan(float(loss_ref))
    back = fr.load_case(name)
    print(f"[golden] waveglow_forward_{name}: z {z_ref.shape} log_s {log_s_ref.shape} max|log_s| {np.abs(log_s_ref).max():.3f}; "
          f"reference vs f64: z rms rel {rms_rel(z_ref, r64['z']):.2e} linf {wr.linf(z_ref, r64['z']):.2e}, "
          f"log_s linf {wr.linf(log_s_ref, r64['log_s']):.2e}, loss {float(loss_ref):.8f} vs {loss64:.10f}; fp32 restatement: "
          f"z linf {wr.linf(r32['z'], r64['z']):.2e} log_s linf {wr.linf(r32['log_s'], r64['log_s']):.2e} loss {abs(loss32 - loss64):.2e}; "
          f"stored f64 z within {wr.linf(back['z_f64'], r64['z']):.1e}; {os.path.getsize(fr.case_path(name)) / 1024:.0f} KiB")


if __name__ == "__main__":
    for n in (sys.argv[1:] or fr.CASES):
        make(n)
