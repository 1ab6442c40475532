"""MelSpectrogramError without a GPU: the numpy restatement (tests/mel_error_restatement.py) against the reference's own outputs
(tests/golden/mel_error_*.npz), argument validation and refusals by message, the column tuple against the header, and the size
queries on refused configs.

The restatement bound: a float32 windowed DFT sum of N terms carries at worst N * 2^-24 relative error on a magnitude, which is the
same absolute error on a log-mel; with d = O(1) that is the relative error of a pair's MSE / MAE.  Both the reference and the float32
arm are float32 computations of that kind, so each must lie within N_max * 2^-24 (relative) of the float64 arm, and within twice that
of each other.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
import mel_error_restatement as mr


def _metric(case="small", **over):
    from cookietts_amd import MelSpectrogramError
    return MelSpectrogramError(**{**mr.ctor_args(case), **over})


@pytest.mark.parametrize("case", list(mr.CASES))
def test_restatement_matches_reference_golden(case):
    g = mr.load_golden(case)
    gt, pred, r64, r32 = mr.live(case)
    assert np.array_equal(gt, g["gt"]) and np.array_equal(pred, g["pred"])                 # the seeded signals are the goldens'
    assert (r64["table"][:, :, 0] == g["n_frames"]).all() and (r32["table"][:, :, 0] == g["n_frames"]).all()
    tol = max(mr.CASES[case]["windows"]) * 2.0 ** -24
    for key, col in (("mse32", 4), ("mae32", 3), ("sae32", 1)):
        y64 = r64["table"][:, :, col]
        for name, got, k in (("reference", g[key], 1), ("float32 arm", r32["table"][:, :, col], 1)):
            rel = np.abs(got - y64) / np.abs(y64)
            print(f"{case} {key} {name}: relative to float64 {rel.max():.2e} (allowed {k * tol:.2e})")
            assert rel.max() <= k * tol, (case, key, name, rel.max(), tol)
        assert (np.abs(g[key] - r32["table"][:, :, col]) <= 2 * tol * np.abs(y64)).all()
    for key, y64 in (("average_MSE32", r64["average_MSE"]), ("average_MAE32", r64["average_MAE"])):
        assert abs(float(g[key]) - y64) <= tol * abs(y64), (case, key)
    assert (np.abs(g["l1_32"] - r64["l1"]) <= tol * np.abs(r64["l1"])).all()
    if "gt_mel32" in g:                                                                      # the nv cases: the loader's y_mel
        for b in range(len(g["gt_mel32"])):
            assert np.abs(g["gt_mel32"][b] - r64["gt_mel"][b][0]).max() <= tol


def test_restatement_averages_follow_the_reference_order():
    """average_MSE is the mean over (file, window) pairs of the pair means (train.py:276-278, 294-295), not a pooled mean."""
    _, _, r64, _ = mr.live("small")
    t = r64["table"]
    assert r64["average_MSE"] == pytest.approx(t[:, :, 4].mean(), rel=1e-14)
    pooled = t[:, :, 2].sum() / (t[:, :, 0] * 12).sum()
    assert abs(pooled - r64["average_MSE"]) > 1e-6 * pooled                                 # the ragged case tells them apart
    assert r64["l1"] == pytest.approx(t[:, :, 1].sum(0) / (t[:, :, 0] * 12).sum(0), rel=1e-14)


def test_restatement_sanitize_rule():
    x = np.array([np.nan, np.inf, -np.inf, 3.0, -3.0, 0.5], np.float32)
    assert mr.sanitize(x).tolist() == [0.0, np.float32(0.999), np.float32(-0.999), np.float32(0.999), np.float32(-0.999), 0.5]


def test_columns_match_header():
    from cookietts_amd import mel_error
    text = open(os.path.join(REPO, "include", "cookietts_hip.h")).read()
    assert int(re.search(r"#define CTTS_MEL_ERROR_COLUMNS (\d+)", text).group(1)) == len(mel_error.COLUMNS) == 5
    assert int(re.search(r"#define CTTS_MEL_ERROR_MAX_WINDOWS (\d+)", text).group(1)) == 8
    assert len(mel_error.TERMS) == 2 + 8
    row = re.search(r"columns:\s+0 n_frames\s+1 SAE.*?2 SSE.*?3 MAE.*?4 MSE", text, re.S)
    assert row, "the header no longer lists the columns in the order of mel_error.COLUMNS"
    assert mel_error.COLUMNS == mr.COLUMNS == ("n_frames", "SAE", "SSE", "MAE", "MSE")
    import cookietts_amd
    assert cookietts_amd.MelSpectrogramError is mel_error.MelSpectrogramError and "MelSpectrogramError" in cookietts_amd.__all__


def test_constructor_refusals():
    from cookietts_amd import MelSpectrogramError
    with pytest.raises(ValueError, match="1 to 8 filter lengths"):
        MelSpectrogramError([], 16, 8000)
    with pytest.raises(ValueError, match="1 to 8 filter lengths"):
        MelSpectrogramError([64] * 9, 16, 8000)
    with pytest.raises(ValueError, match="multiple of 16"):
        MelSpectrogramError([72], 16, 8000)
    with pytest.raises(ValueError, match="multiple of 16"):
        MelSpectrogramError([8192], 16, 8000)
    with pytest.raises(ValueError, match="n_mel_channels 300"):
        MelSpectrogramError([64], 16, 8000, n_mel_channels=300)
    with pytest.raises(ValueError, match="win_lengths has 1 entries for 2 windows"):
        MelSpectrogramError([64, 96], 16, 8000, win_lengths=[64])
    with pytest.raises(ValueError, match="framing must be one of"):
        MelSpectrogramError([64], 16, 8000, framing="librosa")
    m = MelSpectrogramError([1200, 2400], 600, 48000)
    assert m.win_lengths == (1200, 2400) and m.n_mel_channels == 160 and m.pads == (600, 1200) and m.mag_eps == 0.0
    nv = MelSpectrogramError([1024], 256, 22050, 80, 0.0, 8000.0, framing="nv")
    assert nv.pads == (384,) and nv.mag_eps == 1e-9 and nv.frames(8192) == 32 and m.frames(7300) == 13


def test_argument_refusals():
    m = _metric("small")
    x, y = torch.zeros(2, 400), torch.zeros(2, 300)
    mel = torch.zeros(2, 12, 10)
    with pytest.raises(ValueError, match="exactly one of gt_audio and gt_mel"):
        m(x)
    with pytest.raises(ValueError, match="exactly one of gt_audio and gt_mel"):
        m(x, y, gt_mel=mel)
    with pytest.raises(ValueError, match="gt_mel is a single-window input, this object has 2 windows"):
        m(x, gt_mel=mel)
    with pytest.raises(ValueError, match=r"gt_audio must be \[B, T\]"):
        m(x, torch.zeros(3, 300))
    with pytest.raises(ValueError, match="pred_lengths has 3 entries for a batch of 2"):
        m(x, y, pred_lengths=[400, 400, 400])
    with pytest.raises(ValueError, match=r"pred_lengths\[1\] = 401 exceeds the tensor width 400"):
        m(x, y, pred_lengths=[400, 401])
    with pytest.raises(ValueError, match=r"gt_lengths\[0\] = 48 must exceed the reflect pad 48"):
        m(x, y, gt_lengths=torch.tensor([48, 300]))
    with pytest.raises(ValueError, match=r"pred_lengths\[1\] = 100 gives 7 frames at window 64, fewer than the ground truth's 19"):
        m(x, y, pred_lengths=[400, 100])
    nv = _metric("nv_small")
    with pytest.raises(ValueError, match=r"gt_mel must be \[B, n_mel, frames\]"):
        nv(x, gt_mel=torch.zeros(2, 13, 10))
    with pytest.raises(ValueError, match=r"gt_lengths\[0\] = 11 frames must lie in \[1, 10\]"):
        nv(x, gt_mel=mel, gt_lengths=[11, 10])
    with pytest.raises(NotImplementedError, match="pred_audio requires grad"):
        m(x.clone().requires_grad_(), y)
    with pytest.raises(NotImplementedError, match="gt_audio requires grad"):
        m(x, y.clone().requires_grad_())
    from cookietts_amd import _lib
    with torch.no_grad():                                            # grad-carrying tensors pass where no graph is recorded ...
        with pytest.raises(_lib.HipLibraryError, match="pred_audio: expected a CUDA/HIP tensor"):
            m(x.clone().requires_grad_(), y)                         # ... and then meet the CPU refusal
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        m.per_item(x, y)


def test_size_queries_refuse_bad_configs(hip_lib_path):
    from cookietts_amd import _lib
    lib = _lib.lib()
    m = _metric("small")
    good = m._config()
    assert lib.ctts_mel_error_packed_bytes(C.byref(good)) > 0
    assert lib.ctts_mel_error_workspace_bytes(C.byref(good), 3, 2100, 2085) > 0
    assert lib.ctts_mel_error_workspace_bytes(C.byref(good), 3, 2100, 0) > 0                # the gt_mel form

    def refused(why, **fields):
        cfg = m._config()
        for k, v in fields.items():
            if k == "filter0":
                cfg.filter_lengths[0] = v
            else:
                setattr(cfg, k, v)
        assert lib.ctts_mel_error_packed_bytes(C.byref(cfg)) == 0
        assert why in _lib.last_error(), _lib.last_error()
        assert lib.ctts_mel_error_workspace_bytes(C.byref(cfg), 3, 2100, 2085) == 0
        assert why in _lib.last_error(), _lib.last_error()
    refused("n_windows=9", n_windows=9)
    refused("n_windows=0", n_windows=0)
    refused("n_mel_channels=257", n_mel_channels=257)
    refused("filter_length[0]=72", filter0=72)
    refused("filter_length[0]=4112", filter0=4112)
    refused("filter_length[0]=16", filter0=16)
    refused("framing=2", framing=2)
    refused("hop_length=0", hop_length=0)
    assert lib.ctts_mel_error_workspace_bytes(C.byref(good), 0, 2100, 2085) == 0 and "batch=0" in _lib.last_error()
    assert lib.ctts_mel_error_packed_bytes(None) == 0 and "config is NULL" in _lib.last_error()
    # NULL pointers are refused before anything is launched (no device needed)
    rc = lib.ctts_mel_error_f32(C.byref(good), None, None, None, None, None, None, 0, 3, 2100, 2085, 0, None, None, None, None, 0,
                                None, 0, None)
    assert rc == -1 and "NULL argument" in _lib.last_error()
