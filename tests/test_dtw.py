"""DTW without a GPU: the numpy restatement (tests/dtw_restatement.py) against the reference's own outputs (tests/golden/dtw_*.npz), the
one-mistake variants against the same goldens, the refusals by message, and ``vocoder.validate`` without its new keywords.

Bounds.  A float32 output value differs from the float64 winner's by the float32 arm's own rounding, ``e32`` (stored per case: the L-inf
distance of the two arms over every candidate); the reference's output and the float32 arm's must lie within ``8 * e32`` of the float64
winner wherever they choose the float64 argmin.  An fp32 L1 (two fp32 sums of ``C`` rounded terms) lies within ``tau(C)`` (relative) of
the float64 one, so a float32 choice ``k`` satisfies ``L1_64[k] <= min L1_64 * (1 + tau)``.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import dtw_restatement as dr

_LIVE = {}


def live(case):
    if case not in _LIVE:
        c = dr.CASES[case]
        pred, target = dr.signals(case)
        _LIVE[case] = (pred, target, dr.dtw(pred, target, c["s"], c["r"], np.float64), dr.dtw(pred, target, c["s"], c["r"], np.float32))
    return _LIVE[case]


def judge(case, got, g):
    """-> (frames whose choice is not the float64 argmin, frames outside the value bound among the others, frames whose choice is not a
    tau-minimum of the float64 table)."""
    c = dr.CASES[case]
    same = got["choice"] == g["argmin64"]
    dist = np.abs(np.asarray(got["out"], np.float64) - g["ref"]).max(axis=1)
    k = np.take_along_axis(g["l1_64"], (got["choice"] + 1)[:, None, :], axis=1)[:, 0]
    loose = k > g["l1_64"].min(axis=1) * (1 + dr.tau(c["C"]))
    return int((~same).sum()), int((same & (dist > dr.FACTOR * g["e32"])).sum()), int(loose.sum())


@pytest.mark.parametrize("case", list(dr.CASES))
def test_restatement_matches_reference_golden(case):
    c = dr.CASES[case]
    g = dr.load_golden(case)
    pred, target, r64, r32 = live(case)
    assert np.array_equal(pred, g["pred"]) and np.array_equal(target, g["target"])          # the seeded signals are the goldens'
    assert np.array_equal(r64["choice"], g["argmin64"])
    assert np.abs(r64["l1"] - g["l1_64"]).max() <= 1e-9 * max(1.0, np.abs(g["l1_64"]).max())
    assert np.abs(r64["out"] - g["winner64"]).max() == 0
    # the reference's own float32 output is the float64 argmin's candidate on every frame
    far = np.abs(g["ref"] - g["winner64"]).max(axis=1) > dr.FACTOR * g["e32"] + 1e-9
    assert not far.any()
    # the float32 arm: its candidates within e32, its choices tau-minima, at most 1 % of them not the float64 argmin
    assert dr.e32_of(pred, c["s"], c["r"]) == pytest.approx(g["e32"], rel=1e-12, abs=0)
    other, outside, loose = judge(case, r32, g)
    print(f"{case}: float32 arm: {other} of {r32['choice'].size} frames choose another candidate, {outside} outside 8 e32, {loose} loose")
    assert outside == 0 and loose == 0 and other <= 0.01 * r32["choice"].size
    # its L1 table: each of the C terms moves by at most e32 (this arm forms its weights at every expanded index, as the reference does,
    # and so carries the rounding of rs * (p + 0.5) at large p), and the fp32 sums add tau
    slack = c["C"] * g["e32"] + dr.tau(c["C"]) * g["l1_64"]
    assert (np.abs(r32["l1"].astype(np.float64) - g["l1_64"]) <= slack).all()


def test_goldens_exercise_both_outcomes():
    frames = unshifted = 0
    for case in dr.CASES:
        a = dr.load_golden(case)["argmin64"]
        frames, unshifted = frames + a.size, unshifted + int((a < 0).sum())
    assert frames == sum(c["B"] * c["T"] for c in dr.CASES.values()) and 0.02 * frames < unshifted < 0.5 * frames


@pytest.mark.parametrize("mistake", dr.MISTAKES)
def test_every_mistake_leaves_a_bound(mistake):
    """Each one-mistake variant of the float64 arm fails, on at least one golden, a check the real float64 arm passes on all of them:
    its choice is the stored argmin on every frame and its output the stored winner."""
    caught = []
    for case, c in dr.CASES.items():
        g = dr.load_golden(case)
        got = dr.dtw(g["pred"], g["target"], c["s"], c["r"], np.float64, mistake=mistake)
        other, outside, loose = judge(case, got, g)
        if other or outside or loose:
            caught.append((case, other, outside, loose))
    print(mistake, caught)
    assert caught, f"no golden tells the {mistake!r} variant from the reference"


def test_first_wins_rules_of_the_restatement():
    """pred wins every tie (s odd: the centre candidate IS pred), an earlier candidate a tie with a later one, a NaN sum nothing."""
    rng = np.random.default_rng(5)
    pred = rng.integers(-3, 4, (1, 4, 9)).astype(np.float64)
    r = dr.dtw(pred, pred, 5, 3)
    assert (r["choice"] == -1).all() and np.array_equal(r["out"], pred)
    assert (r["l1"][0, 1 + 5 * 1 + 2] == 0).all()                                           # j = s h + (s - 1) / 2 ties with pred
    target = rng.standard_normal((1, 4, 9))
    target[0, :, 4] = np.nan
    r = dr.dtw(pred, target, 5, 3)
    assert r["choice"][0, 4] == -1 and np.array_equal(r["out"][0, :, 4], pred[0, :, 4])
    one = np.full((1, 3, 1), 2.0)
    r = dr.dtw(one, 0.5 * one, 8, 5)                                                       # T = 1: candidates tie in pairs (j, 39 - j)
    assert np.array_equal(r["l1"][0, 1:, 0], r["l1"][0, 1:, 0][::-1]) and 0 <= r["choice"][0, 0] < 20


def test_assert_messages_and_refusals():
    import cookietts_amd
    from cookietts_amd import DTW, _lib, dtw
    assert cookietts_amd.DTW is dtw.DTW and "DTW" in cookietts_amd.__all__
    x, y = torch.zeros(2, 5, 9), torch.zeros(2, 5, 9)
    with pytest.raises(AssertionError, match="range_ must be an odd integer."):
        DTW(x, y, 8, 4)
    with pytest.raises(AssertionError, match="pred and target shapes must match."):
        DTW(x, torch.zeros(2, 5, 8), 8, 5)
    with pytest.raises(NotImplementedError, match="batch_pred requires grad"):
        DTW(x.clone().requires_grad_(), y, 8, 5)
    with pytest.raises(NotImplementedError, match="batch_target requires grad"):
        DTW(x, y.clone().requires_grad_(), 8, 5)
    with pytest.raises(ValueError, match="product at most 64"):
        DTW(x, y, 13, 5)
    with pytest.raises(ValueError, match="both must be at least 1"):
        DTW(x, y, 0, 5)
    with pytest.raises(ValueError, match=r"batch_pred must be \[B, C, T\]"):
        DTW(torch.zeros(5, 9), torch.zeros(5, 9), 8, 5)
    with pytest.raises(ValueError, match="must be a floating-point tensor"):
        DTW(x.long(), y.long(), 8, 5)
    with pytest.raises(_lib.HipLibraryError, match="batch_pred: expected a CUDA/HIP tensor"):
        DTW(x, y, 8, 5)
    with torch.no_grad():                                            # grad-carrying tensors pass where no graph is recorded ...
        with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
            DTW(x.clone().requires_grad_(), y, 8, 5)                 # ... and then meet the CPU refusal
    with pytest.raises(ValueError, match="lengths has 3 entries for a batch of 2"):
        dtw._lengths([9, 9, 9], 2, 9, "cpu")
    with pytest.raises(ValueError, match=r"lengths\[1\] = 10 must lie in \[1, 9\]"):
        dtw._lengths([9, 10], 2, 9, "cpu")
    with pytest.raises(ValueError, match=r"lengths\[0\] = 0 must lie in \[1, 9\]"):
        dtw._lengths(torch.tensor([0, 9]), 2, 9, "cpu")
    assert dtw._lengths(None, 2, 9, "cpu") is None and dtw._lengths([9, 1], 2, 9, "cpu").dtype == torch.int32


def test_library_refuses_by_name_before_any_launch(hip_lib_path):
    """Every refusal of the C entry point is host code: it answers CTTS_E_ARG with a text, on a machine without a device."""
    from cookietts_amd import _lib
    lib = _lib.lib()
    buf = (C.c_float * 64)()
    other = (C.c_float * 64)()
    out = (C.c_float * 64)()
    p, q, o = (C.cast(b, C.c_void_p) for b in (buf, other, out))

    def refused(why, fn=lib.ctts_mel_dtw_f32, pred=p, target=q, dst=o, B=1, Cn=4, T=16, s=8, r=5):
        assert fn(pred, target, None, dst, None, None, B, Cn, T, s, r, None) == -1
        assert why in _lib.last_error(), _lib.last_error()
    for fn in (lib.ctts_mel_dtw_f32, lib.ctts_mel_dtw_generic_f32):
        refused("NULL argument", fn, pred=None)
        refused("NULL argument", fn, dst=None)
        refused("range=4 must be an odd integer", fn, r=4)
        refused("range=0 must be an odd integer", fn, r=0)
        refused("scale_factor=0 must be at least 1", fn, s=0)
        refused("scale_factor * range = 65 candidates exceed 64", fn, s=13)
        refused("frames=0 must be at least 1", fn, T=0)
        refused("channels=0 must be at least 1", fn, Cn=0)
        refused("batch=0 must lie in", fn, B=0)
        refused("out aliases pred", fn, dst=p)
        refused("out aliases pred", fn, dst=C.c_void_p(p.value + 32))
        refused("out aliases target", fn, dst=q)


def test_validate_without_dtw_target_takes_the_unchanged_path(monkeypatch):
    """``validate(dtw_target=None)`` never touches DTW and hands ``infer`` the very tensor it was given."""
    from cookietts_amd import dtw, vocoder

    def boom(*a, **k):
        raise AssertionError("DTW must not be called")
    monkeypatch.setattr(dtw, "DTW", boom)
    monkeypatch.setattr(vocoder, "DTW", boom, raising=False)
    seen = {}

    class Toy(torch.nn.Module):
        def infer(self, mels, speaker_ids, sigma):
            seen.update(mels=mels, speaker_ids=speaker_ids, sigma=sigma, training=self.training)
            return torch.zeros(mels.shape[0], 7)

    def metric(audio, gt_audio, gt_lengths):
        seen.update(audio=audio, gt=gt_audio, gt_lengths=gt_lengths)
        return {"average_MSE": 1.5, "average_MAE": 0.5}
    model = Toy().train()
    mels, gt = torch.zeros(2, 6, 5), torch.zeros(2, 9)
    for kw in ({}, {"dtw_target": None}, {"dtw_target": None, "dtw": (5, 3), "dtw_lengths": [5, 4]}):
        seen.clear()
        mse, mae, res = vocoder.validate(model, mels, gt, [9, 8], metric, 0.9, **kw)
        assert (mse, mae) == (1.5, 0.5) and seen["mels"] is mels and seen["sigma"] == 0.9 and seen["training"] is False
        assert seen["gt_lengths"] == [9, 8] and model.training
    with pytest.raises(ValueError, match=r"dtw_target must be \[B, n_mel, F\]"):
        vocoder.validate(model, mels, gt, [9, 8], metric, 0.9, dtw_target=torch.zeros(2, 7, 5))
    with pytest.raises(ValueError, match=r"dtw_target must be \[B, n_mel, F\]"):
        vocoder.validate(model, mels, gt, [9, 8], metric, 0.9, dtw_target=torch.zeros(2, 6, 4))
