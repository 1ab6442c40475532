#!/usr/bin/env python3
"""Generate tests/golden/hgedge_<config>.npz by RUNNING THE REFERENCE'S OWN GENERATOR on the CPU, in fp32, fp64 and half.

Run where the reference tree is checked out (it is not on the GPU box):

    COOKIETTS_REFERENCE=<path of the reference tree> python tests/golden/make_golden_hifigan_edge.py [config ...]

The configs and cases are tests/hifigan_edge_cases.py's (CONFIGS, CASES): what the plan of csrc/hifigan_plan.h accepts beyond
the seven ``hifigan_*.npz`` goldens - ragged channel counts, odd upsampling rates, kernel == rate, rate 1, kernel 1, one and four
resblocks per stage, halos at the limit, 1- and 2-frame calls, lengths on and just past the column tiles.  One file per
config; data only, per case ``<case>.<field>``:

    seed               int64                      of the numpy weight recipe (``synthetic.hifigan_state_dict``; weights are not stored)
    mel                float32 [B, num_mels, T]
    audio              float32 [B, 1, T prod(u)]  the reference's fp32 waveform
    ref_fp32_vs_fp64   float64 [2]                (relative RMS, L-inf) of it against ``Generator(h).double()`` on the same input
    audio_half         float16 [B, 1, T prod(u)]  the reference's half-mode waveform (``remove_weight_norm(); .half()``, half mel)
    ref_half_vs_fp32   float64 [2]                (relative RMS, L-inf) of it against ``audio``

as make_golden_hifigan.py and make_golden_hifigan_f16.py define them, with their asserts: waveform RMS in [0.05, 0.8], at most
1 % of the samples with |y| > 0.999, half-mode relative RMS below 5e-3 (a case that misses gets another seed, not a wider band).
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
if os.environ.get("COOKIETTS_REFERENCE"):
    sys.path.insert(0, os.environ["COOKIETTS_REFERENCE"])

import hifigan_edge_cases as ec  # noqa: E402
from make_golden_hifigan import _ref_generator  # noqa: E402

MAX_FILE = 1 << 20
MAX_REL_HALF = 5e-3


def _err(y, want):
    d = y.astype(np.float64) - want.astype(np.float64)
    return float(np.sqrt(np.mean(d ** 2)) / np.sqrt(np.mean(want.astype(np.float64) ** 2))), float(np.abs(d).max())


def main():
    torch.set_num_threads(8)
    only = sys.argv[1:]
    for key, cfg in ec.CONFIGS.items():
        if only and key not in only:
            continue
        fields = {}
        for batch, frames, seed in ec.CASES[key]:
            name = ec.case_name(batch, frames)
            sd = ec.state_dict(key, seed)
            mel = ec.mel(key, batch, frames, seed)
            model = _ref_generator(cfg, sd)
            with torch.no_grad():
                y32 = model(torch.from_numpy(mel.copy())).numpy()
                y64 = model.double()(torch.from_numpy(mel.copy()).double()).numpy()
                y16 = _ref_generator(cfg, sd).half()(torch.from_numpy(mel.copy()).half())
            assert y16.dtype == torch.float16
            y16 = y16.numpy()
            rel, linf = _err(y32, y64)
            rel16, linf16 = _err(y16, y32)
            rms = float(np.sqrt(np.mean(y64 ** 2)))
            sat = float(np.mean(np.abs(y64) > 0.999))
            print(f"{key} {name}: out {y32.shape} rms {rms:.3f} max {np.abs(y64).max():.3f} saturated {sat:.4%} "
                  f"ref_fp32_vs_fp64 rel rms {rel:.3e} linf {linf:.3e}; ref_half_vs_fp32 rel rms {rel16:.3e} linf {linf16:.3e}",
                  flush=True)
            assert 0.05 <= rms <= 0.8, (key, name, rms)
            assert sat <= 0.01, (key, name, sat)
            assert y32.shape == y16.shape == (batch, 1, frames * int(np.prod(cfg["upsample_rates"])))
            assert np.isfinite(y16).all() and rel16 < MAX_REL_HALF, (key, name, rel16)
            for f, v in dict(seed=np.int64(seed), mel=mel, audio=y32.astype(np.float32),
                             ref_fp32_vs_fp64=np.array([rel, linf], np.float64), audio_half=y16,
                             ref_half_vs_fp32=np.array([rel16, linf16], np.float64)).items():
                fields[f"{name}.{f}"] = v
        path = ec.fixture_path(key)
        np.savez_compressed(path, **fields)
        print(f"{path}: {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) <= MAX_FILE, (key, os.path.getsize(path))


if __name__ == "__main__":
    main()
