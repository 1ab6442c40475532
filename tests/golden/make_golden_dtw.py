#!/usr/bin/env python3
"""Goldens of DTW: the reference's own ``DTW`` (``_4_mtw/waveglow/mel2samp.py:81-118``) run on the CPU in float32.

Run in the build container only (it imports the reference):

    python tests/golden/make_golden_dtw.py

The function is imported rather than re-typed (``torch.jit.script`` needs its source file); its module wants ``librosa``, which is not
installed, hence ``make_golden.py``'s stand-ins (``_stub_audio_deps``).

Data only: per case ``dtw_<case>.npz`` holds ``pred16`` / ``target16`` (the inputs of ``dtw_restatement.signals``: float16 holds them
exactly), ``argmin64`` (int8 [B, T]: the float64 restatement's first-wins argmin, -1 = the unshifted frame), ``l1_64_f32`` +
``l1_64_delta16`` / ``l1_64_scale`` (the float64 L1 table [B, s r + 1, T]: rounded to float32 plus the 16-bit delta to that rounding),
``ref_delta16`` / ``ref_scale`` (the reference's float32 output as a 16-bit delta against the float64 argmin's candidate) and ``e32``
(the float32 restatement's L-inf distance from the float64 one over every candidate).

Asserted for every fixture written: the reference's output is the float64 argmin's candidate on EVERY frame - no frame where it is
farther than ``8 * e32`` from that candidate.
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
import dtw_restatement as dr  # noqa: E402


def reference_dtw():
    mg._stub_audio_deps()
    # utils/audio/iso226.py runs an installer when `import iso226` fails: an empty stand-in keeps the import quiet (DTW never uses it)
    sys.modules.setdefault("iso226", types.ModuleType("iso226"))
    import CookieTTS
    sys.path.insert(0, os.path.join(os.path.dirname(CookieTTS.__file__), "_4_mtw", "waveglow"))   # its `waveglow_utils`
    from CookieTTS._4_mtw.waveglow import mel2samp
    return mel2samp.DTW


def make(case, DTW):
    c = dr.CASES[case]
    pred, target = dr.signals(case)
    with torch.no_grad():
        ref = DTW(torch.from_numpy(pred), torch.from_numpy(target), c["s"], c["r"]).numpy()
    r64 = dr.dtw(pred, target, c["s"], c["r"], np.float64)
    e32 = dr.e32_of(pred, c["s"], c["r"])
    far = np.abs(ref.astype(np.float64) - r64["out"]).max(axis=1) > dr.FACTOR * e32                 # [B, T]
    unshifted = float((r64["choice"] < 0).mean())
    print(f"{case}: e32 {e32:.2e}; frames where the reference is not the float64 argmin's candidate: {int(far.sum())} of {far.size}; "
          f"the unshifted frame wins on {100 * unshifted:.1f} %")
    assert not far.any(), (case, np.argwhere(far)[:5])
    l1_f32 = r64["l1"].astype(np.float32)
    ld, ls = dr.pack_delta(r64["l1"], l1_f32)
    rd, rs = dr.pack_delta(ref, r64["out"])
    path = os.path.join(HERE, f"dtw_{case}.npz")
    np.savez_compressed(path, pred16=pred.astype(np.float16), target16=target.astype(np.float16),
                        argmin64=r64["choice"].astype(np.int8), l1_64_f32=l1_f32, l1_64_delta16=ld, l1_64_scale=ls,
                        ref_delta16=rd, ref_scale=rs, e32=np.float64(e32))
    print("wrote", path, os.path.getsize(path), "bytes")
    return far.size


if __name__ == "__main__":
    fn = reference_dtw()
    total = sum(make(name, fn) for name in (sys.argv[1:] or list(dr.CASES)))
    print("frames in all:", total)
