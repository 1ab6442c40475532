#!/usr/bin/env python3
"""Generate tests/golden/hifigan_*.npz and hifigan_state_shapes.json by RUNNING THE REFERENCE'S OWN GENERATOR on the CPU.

Run in the build container only (the reference tree is not on the GPU box):

    python tests/golden/make_golden_hifigan.py [case ...]

Data only: the mel, the seed of the numpy weight recipe (``cookietts_amd.synthetic.hifigan_state_dict`` - weights are never
stored), the reference's fp32 waveform, and the reference's own rounding ``ref_fp32_vs_fp64`` = (relative RMS, L-inf) of
``Generator(h)`` against ``Generator(h).double()`` on the same input, which the tests scale their bounds from.  The state
dict goes in through the reference's ``load_state_dict`` (weight-norm keys), then ``remove_weight_norm`` as its
``load_model`` does.  Every case must be a waveform worth comparing: RMS in [0.05, 0.8], at most 1 % of the samples with
|y| > 0.999 (asserted; a case that misses gets another seed or gain, not a wider band).
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, "/root/reference")

from cookietts_amd import synthetic  # noqa: E402

SHIPPED = ("v1", "v2", "v3", "v1_48khz")
# name, config key, batch, frames, seed
CASES = [
    ("toy_rb1", "toy_rb1", 2, 33, 101),
    ("toy_rb2", "toy_rb2", 2, 129, 102),
    ("toy_rate4", "toy_rate4", 2, 3, 103),
    ("v1", "v1", 2, 33, 111),
    ("v2", "v2", 2, 129, 112),
    ("v3", "v3", 2, 33, 113),
    ("v1_48khz", "v1_48khz", 2, 33, 114),
    ("v1_full_length", "v1", 1, 900, 115),
]


MAX_FILE = 1 << 20


def _ref_generator(cfg, sd_np=None):
    from CookieTTS._4_mtw.hifigan.env import AttrDict
    from CookieTTS._4_mtw.hifigan.models import Generator
    model = Generator(AttrDict(cfg))
    if sd_np is not None:
        res = model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd_np.items()}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        with contextlib.redirect_stdout(io.StringIO()):      # it prints 'Removing weight norm...'
            model.remove_weight_norm()
    return model.eval()


def hifigan_mel(batch, frames, n_mel, seed):
    """The project's log-mel-like input, 2 N(0, 1) - 5 clipped to [-11.52, 2] (the input the state dict's gains were chosen with)."""
    return synthetic.synthetic_mel(batch, frames, n_mel, seed=seed)


def main():
    torch.set_num_threads(8)
    only = sys.argv[1:]
    shapes = {}
    for key in SHIPPED:
        model = _ref_generator(synthetic.HIFIGAN_CONFIGS[key])
        shapes[key] = {k: list(v.shape) for k, v in model.state_dict().items()}
    if not only:
        with open(os.path.join(HERE, "hifigan_state_shapes.json"), "w") as f:
            json.dump(shapes, f, indent=0, sort_keys=True)
            f.write("\n")
    for name, key, B, T, seed in CASES:
        if only and name not in only:
            continue
        cfg = synthetic.HIFIGAN_CONFIGS[key]
        sd = synthetic.hifigan_state_dict(cfg, seed=seed)
        mel = hifigan_mel(B, T, cfg["num_mels"], seed)
        model = _ref_generator(cfg, sd)
        with torch.no_grad():
            y32 = model(torch.from_numpy(mel.copy())).numpy()
            y64 = model.double()(torch.from_numpy(mel.copy()).double()).numpy()
        d = y32.astype(np.float64) - y64
        rel = float(np.sqrt(np.mean(d ** 2)) / np.sqrt(np.mean(y64 ** 2)))
        linf = float(np.abs(d).max())
        rms = float(np.sqrt(np.mean(y64 ** 2)))
        sat = float(np.mean(np.abs(y64) > 0.999))
        print(f"{name}: out {y32.shape} rms {rms:.3f} max {np.abs(y64).max():.3f} saturated {sat:.4%} "
              f"ref_fp32_vs_fp64 rel rms {rel:.3e} linf {linf:.3e}", flush=True)
        assert 0.05 <= rms <= 0.8, (name, rms)
        assert sat <= 0.01, (name, sat)
        assert y32.shape == (B, 1, T * int(np.prod(cfg["upsample_rates"])))
        fields = dict(config=np.array(key), seed=np.int64(seed), mel=mel, audio=y32.astype(np.float32),
                      ref_fp32_vs_fp64=np.array([rel, linf], np.float64))
        path = os.path.join(HERE, f"hifigan_{name}.npz")
        np.savez_compressed(path, **fields)
        if os.path.getsize(path) > MAX_FILE:
            # a committed file stays under 1 MiB: the mel moves to a file of its own (tests/hifigan_restatement.py load_case puts it back)
            np.savez_compressed(os.path.join(HERE, f"hifigan_{name}.mel.npz"), mel=fields.pop("mel"))
            np.savez_compressed(path, **fields)
        assert os.path.getsize(path) <= MAX_FILE, (name, os.path.getsize(path))


if __name__ == "__main__":
    main()
