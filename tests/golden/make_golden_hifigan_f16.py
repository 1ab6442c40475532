#!/usr/bin/env python3
"""Generate tests/golden/hgf16_*.npz by RUNNING THE REFERENCE'S OWN GENERATOR IN ITS HALF MODE on the CPU.

Run where the reference tree is checked out (it is not on the GPU box):

    COOKIETTS_REFERENCE=<path of the reference tree> python tests/golden/make_golden_hifigan_f16.py [case ...]

For each existing HiFi-GAN case (config, seed and mel read from ``hifigan_<name>.npz``) the reference generator is loaded as
``make_golden_hifigan.py`` loads it, then ``remove_weight_norm()`` and ``.half()`` as the server does
(text2speech.py:258-263), and run on the mel cast to half.  Data only:

    audio_half         float16 [B, 1, T prod(u)]  the reference's half-mode waveform
    ref_half_vs_fp32   float64 [2]                (relative RMS, L-inf) of it against the fp32 golden ``audio``

The tests of the HIP half mode scale their bounds from ``ref_half_vs_fp32``; the script asserts the half output is finite
and its relative RMS below 5e-3, so such a bound cannot become vacuous.  The file names do not start with ``hifigan_``:
``hifigan_restatement.golden_cases()`` takes every ``hifigan_*.npz`` for a case of the fp32 tests.
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

from cookietts_amd import synthetic  # noqa: E402
import hifigan_restatement as hr  # noqa: E402
from make_golden_hifigan import _ref_generator  # noqa: E402

MAX_FILE = 1 << 20
MAX_REL = 5e-3


def main():
    torch.set_num_threads(8)
    only = sys.argv[1:]
    for name in hr.golden_cases():
        if only and name not in only:
            continue
        z = hr.load_case(name)
        cfg = synthetic.HIFIGAN_CONFIGS[str(z["config"])]
        sd = synthetic.hifigan_state_dict(cfg, seed=int(z["seed"]))
        model = _ref_generator(cfg, sd).half()
        with torch.no_grad():
            y16 = model(torch.from_numpy(z["mel"].copy()).half())
        assert y16.dtype == torch.float16
        y16 = y16.numpy()
        assert y16.shape == z["audio"].shape and np.isfinite(y16).all(), name
        d = y16.astype(np.float64) - z["audio"].astype(np.float64)
        rel = float(np.sqrt(np.mean(d ** 2)) / np.sqrt(np.mean(z["audio"].astype(np.float64) ** 2)))
        linf = float(np.abs(d).max())
        print(f"{name}: out {y16.shape} ref_half_vs_fp32 rel rms {rel:.3e} linf {linf:.3e}", flush=True)
        assert rel < MAX_REL, (name, rel)
        path = os.path.join(HERE, f"hgf16_{name}.npz")
        np.savez_compressed(path, audio_half=y16, ref_half_vs_fp32=np.array([rel, linf], np.float64))
        assert os.path.getsize(path) <= MAX_FILE, (name, os.path.getsize(path))


if __name__ == "__main__":
    main()
