#!/usr/bin/env python3
"""Generate tests/golden/torchmoji_*.npz by RUNNING THE REFERENCE'S OWN ``TorchMoji`` on the CPU.

Run in the build container only (the reference tree is not on the GPU box):

    python tests/golden/make_golden_torchmoji.py [case ...]

Data only: the tokens (uint16, as the reference's tokenizer gives them), the seed of the numpy weight recipe
(``cookietts_amd.synthetic.torchmoji_state_dict`` - weights are never stored), ``nb_tokens``, the reference's fp32 features
``TorchMoji(nb_classes=None, nb_tokens, feature_output=True)(tokens)`` and, where the lengths of a case are distinct, its
attention weights.  The reference returns those sorted by length (model_def.py:194-195, 250-251: only the features are
un-sorted); a stable descending sort of distinct lengths is unambiguous, so they are un-sorted here and stored in INPUT order.
With tied lengths the reference's own order is whatever ``Tensor.sort`` gives: no attention is stored for such a case.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, "/root/reference")

from cookietts_amd import synthetic  # noqa: E402

NB_TOKENS = 500
# name, lengths, T, seed, (row, column) of an interior zero or None
CASES = [
    ("ragged6", (20, 7, 1, 13, 20, 2), 20, 201, (3, 5)),
    ("ragged3", (20, 7, 1), 20, 202, None),
    ("one_token", (1,), 1, 203, None),
    ("t130", (130, 129), 130, 204, None),
]
MAX_FILE = 1 << 20


def case_tokens(lengths, T, seed, hole):
    rng = np.random.default_rng(seed)
    tok = np.zeros((len(lengths), T), np.uint16)
    for b, n in enumerate(lengths):
        tok[b, :n] = rng.integers(1, NB_TOKENS, size=n)
    if hole is not None:
        assert hole[1] < lengths[hole[0]] - 1
        tok[hole] = 0
    return tok


def main():
    torch.set_num_threads(8)
    warnings.filterwarnings("ignore", message=".*dropout2d.*")
    from CookieTTS.utils.torchmoji.model_def import TorchMoji
    only = sys.argv[1:]
    for name, lengths, T, seed, hole in CASES:
        if only and name not in only:
            continue
        tok = case_tokens(lengths, T, seed, hole)
        sd = synthetic.torchmoji_state_dict(NB_TOKENS, seed)
        distinct = len(set(lengths)) == len(lengths)
        model = TorchMoji(nb_classes=None, nb_tokens=NB_TOKENS, feature_output=True, return_attention=distinct)
        res = model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys and not model.training
        with torch.no_grad():
            out = model(tok)
        fields = dict(tokens=tok, seed=np.int64(seed), nb_tokens=np.int64(NB_TOKENS))
        if distinct:
            feats, att = out
            att = att.numpy()
            perm = np.argsort(-np.asarray(lengths), kind="stable")        # the reference's perm_idx for distinct lengths
            unsorted = np.zeros_like(att)
            unsorted[perm] = att
            assert np.allclose(unsorted.sum(axis=1), 1.0, atol=1e-5)
            for b, n in enumerate(lengths):
                assert (unsorted[b, n:] == 0).all() and (unsorted[b, :n] > 0).all()
            fields["attention"] = unsorted.astype(np.float32)
        else:
            feats = out
        feats = np.asarray(feats, np.float32)
        assert feats.shape == (len(lengths), 2304) and np.isfinite(feats).all()
        fields["features"] = feats
        path = os.path.join(HERE, f"torchmoji_{name}.npz")
        np.savez_compressed(path, **fields)
        print(f"{name}: tokens {tok.shape} features max |.| {np.abs(feats).max():.3f} attention {'yes' if distinct else 'no'} "
              f"{os.path.getsize(path)} bytes", flush=True)
        assert os.path.getsize(path) <= MAX_FILE


if __name__ == "__main__":
    main()
