"""DTW on the device (csrc/dtw.hip) against the reference's outputs and the float64 restatement (tests/golden/dtw_*.npz), its tie, NaN
and ragged-length rules, and ``vocoder.validate(dtw_target=...)``.

Bounds (tests/dtw_restatement.py): a value within ``8 * e32`` of the reference on every frame whose choice is the float64 argmin; every
choice ``k`` a ``tau``-minimum of the float64 L1 table, ``tau = 4 (C + 4) 2^-24`` (two fp32 sums of C rounded terms, times two); at most
1 % of a case's frames with another choice than the float64 argmin (the reference itself has none); the ``l1`` outputs within ``tau``
(relative) of the float64 table.
"""
import numpy as np
import pytest
import torch

import dtw_restatement as dr

pytestmark = pytest.mark.gpu


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype in (torch.float32, torch.int32) else torch.int16).numpy().tobytes()


def _run(pred, target, s, r, lengths=None, generic=False):
    """-> (out, choice, l1_before, l1_after) as device tensors."""
    from cookietts_amd import dtw
    out, info = dtw._run(pred, target, s, r, lengths, True, generic=generic)
    return out, info["choice"], info["l1_before"], info["l1_after"]


_GOT = {}


def _golden_run(case):
    """The device's answer on a golden, computed once and shared (never written to)."""
    if case not in _GOT:
        c, g = dr.CASES[case], dr.load_golden(case)
        _GOT[case] = _run(_dev(g["pred"]), _dev(g["target"]), c["s"], c["r"])
    return _GOT[case]


@pytest.mark.parametrize("case", list(dr.CASES))
def test_values_and_selection_match_reference_golden(hip_lib_path, case):
    c, g = dr.CASES[case], dr.load_golden(case)
    out, choice, before, after = (x.cpu().numpy() for x in _golden_run(case))
    tau, l1 = dr.tau(c["C"]), g["l1_64"]
    assert choice.min() >= -1 and choice.max() < c["s"] * c["r"]
    same = choice == g["argmin64"]
    dist = np.abs(out.astype(np.float64) - g["ref"]).max(axis=1)
    picked = np.take_along_axis(l1, (choice.astype(np.int64) + 1)[:, None, :], axis=1)[:, 0]
    excess = picked / np.maximum(l1.min(axis=1), 1e-300) - 1
    rel_b = np.abs(before - l1[:, 0]) / np.maximum(l1[:, 0], 1e-300)
    rel_a = np.abs(after - picked) / np.maximum(picked, 1e-300)
    print(f"{case}: {int((~same).sum())} of {same.size} frames choose another candidate than the float64 argmin (cap {0.01 * same.size:.2f}); "
          f"values: {dist[same].max(initial=0):.2e} from the reference (allowed {dr.FACTOR * g['e32']:.2e}); selection excess "
          f"{excess.max():.2e}, l1_before {rel_b.max():.2e}, l1_after {rel_a.max():.2e} (tau {tau:.2e})")
    assert (dist[same] <= dr.FACTOR * g["e32"]).all()                                     # values
    assert (picked <= l1.min(axis=1) * (1 + tau)).all()                                     # selection
    assert (~same).sum() <= 0.01 * same.size                                                # cap
    assert (np.abs(before - l1[:, 0]) <= tau * l1[:, 0]).all() and (np.abs(after - picked) <= tau * picked).all()


@pytest.mark.parametrize("case", list(dr.CASES))
def test_repeats_and_every_variant_equals_the_generic_form(hip_lib_path, case):
    c, g = dr.CASES[case], dr.load_golden(case)
    pred, target = _dev(g["pred"]), _dev(g["target"])
    keep = pred.clone()
    first = _golden_run(case)
    again = _run(pred, target, c["s"], c["r"])
    generic = _run(pred, target, c["s"], c["r"], generic=True)
    for a, b, d in zip(first, again, generic):
        assert _bits(a) == _bits(b)                                                         # two runs: the same bits
        assert _bits(a) == _bits(d)                                                         # the compiled (s, r) variant: the generic form's bits
    assert torch.equal(pred, keep)                                                          # no input is written


def test_constant_pred_returns_pred_on_every_interior_frame(hip_lib_path):
    """s = 8, small-integer pred constant over time: every candidate of an interior frame IS pred (weights k/16 of one value), all tie
    and the unshifted frame wins.  Two tiles of 64 frames, C below the four channel slices and above."""
    rng = np.random.default_rng(11)
    for C_, T in ((3, 70), (9, 130)):
        pred = np.repeat(rng.integers(-4, 5, (2, C_, 1)), T, axis=2).astype(np.float32)
        target = rng.standard_normal((2, C_, T)).astype(np.float32)
        out, choice, before, after = _run(_dev(pred), _dev(target), 8, 5)
        inner = slice(3, T - 3)                                                             # h + 1 frames from both ends
        assert (choice[:, inner] == -1).all()
        assert _bits(out[:, :, inner]) == _bits(_dev(pred)[:, :, inner])
        assert _bits(before[:, inner]) == _bits(after[:, inner])


def test_an_earlier_candidate_wins_an_exact_tie(hip_lib_path):
    """Channel 1 is channel 0 mirrored in time about frame 4: the candidates at -3/16 and +3/16 of a frame (j = 18 and 21) swap their two
    channel terms (0.125 + 0.0625 against 0.0625 + 0.125, all exact in fp32) and tie below every other candidate; j = 18 wins."""
    pred = np.full((1, 2, 9), 9.0, np.float32)
    pred[0, 0, 3:6] = (2, 0, 1)
    pred[0, 1, 3:6] = (1, 0, 2)
    target = np.full((1, 2, 9), 0.25, np.float32)
    r = dr.dtw(pred, target, 8, 5)
    assert r["l1"][0, 1 + 18, 4] == r["l1"][0, 1 + 21, 4] == 0.1875 == r["l1"][0, :, 4].min() and r["choice"][0, 4] == 18
    out, choice, before, after = _run(_dev(pred), _dev(target), 8, 5)
    assert int(choice[0, 4]) == 18 and float(before[0, 4]) == 0.5 and float(after[0, 4]) == 0.1875
    assert out[0, :, 4].tolist() == [0.375, 0.1875]
    assert np.array_equal(choice.cpu().numpy(), r["choice"]) and np.array_equal(out.cpu().numpy(), r["out"].astype(np.float32))


def test_nan_never_wins_and_stays_local(hip_lib_path):
    c, g = dr.CASES["s8r5_t67"], dr.load_golden("s8r5_t67")
    h = c["r"] // 2
    clean_out, clean_choice, _, _ = _golden_run("s8r5_t67")
    target = g["target"].copy()
    target[1, :, 30] = np.nan                                                               # a NaN sum: new < old is false
    out, choice, before, after = _run(_dev(g["pred"]), _dev(target), c["s"], c["r"])
    assert int(choice[1, 30]) == -1 and _bits(out[1, :, 30]) == _bits(_dev(g["pred"])[1, :, 30])
    assert torch.isnan(before[1, 30]) and torch.isnan(after[1, 30])
    keep = torch.ones(c["T"], dtype=torch.bool)
    keep[30] = False
    assert _bits(out[:, :, keep]) == _bits(clean_out[:, :, keep]) and _bits(choice[:, keep]) == _bits(clean_choice[:, keep])
    pred = g["pred"].copy()
    pred[2, 5, 64] = np.nan                                                                 # one value of one frame, in the second tile
    out, choice, _, _ = _run(_dev(pred), _dev(g["target"]), c["s"], c["r"])
    far = (torch.arange(c["T"]) - 64).abs() > h + 1                                         # frames that do not read frame 64
    assert _bits(out[:, :, far]) == _bits(clean_out[:, :, far]) and _bits(choice[:, far]) == _bits(clean_choice[:, far])
    assert _bits(out[:2]) == _bits(clean_out[:2])                                           # the other items
    assert int(choice[2, 64]) == -1 and not torch.isnan(out[2, :5, 64]).any()               # the NaN frame itself: nothing beats pred


@pytest.mark.parametrize("on_device", [False, True])
def test_ragged_lengths_equal_the_cropped_items(hip_lib_path, on_device):
    c, g = dr.CASES["s8r5_t67"], dr.load_golden("s8r5_t67")
    pred, target = _dev(g["pred"]), _dev(g["target"])
    lengths = (67, 40, 1)
    arg = torch.tensor(lengths, dtype=torch.int64).cuda() if on_device else list(lengths)
    out, choice, before, after = _run(pred, target, c["s"], c["r"], lengths=arg)
    for b, L in enumerate(lengths):
        o1, c1, b1, a1 = _run(pred[b:b + 1, :, :L], target[b:b + 1, :, :L], c["s"], c["r"])
        assert _bits(out[b:b + 1, :, :L]) == _bits(o1) and _bits(choice[b:b + 1, :L]) == _bits(c1)
        assert _bits(before[b:b + 1, :L]) == _bits(b1) and _bits(after[b:b + 1, :L]) == _bits(a1)
        assert _bits(out[b, :, L:]) == _bits(pred[b, :, L:]) and (choice[b, L:] == -1).all()
        assert (before[b, L:] == 0).all() and (after[b, L:] == 0).all()
    whole = _golden_run("s8r5_t67")
    assert _bits(out[0]) == _bits(whole[0][0])                                              # lengths[0] = T: the call without lengths


def test_out_of_range_device_lengths_are_clamped(hip_lib_path):
    c, g = dr.CASES["s8r5_c7_t3"], dr.load_golden("s8r5_c7_t3")
    pred, target = _dev(g["pred"]), _dev(g["target"])
    got = _run(pred, target, c["s"], c["r"], lengths=torch.tensor([9, 0]).cuda())
    want = _run(pred, target, c["s"], c["r"], lengths=[3, 1])
    for a, b in zip(got, want):
        assert _bits(a) == _bits(b)


def test_noncontiguous_and_half_inputs(hip_lib_path):
    from cookietts_amd import DTW
    c, g = dr.CASES["s5r3_t200"], dr.load_golden("s5r3_t200")
    pred, target = _dev(g["pred"]), _dev(g["target"])
    want = _golden_run("s5r3_t200")[0]
    assert _bits(DTW(pred, target, c["s"], c["r"])) == _bits(want)                          # the public call, no info
    pt, tt = pred.transpose(1, 2).contiguous().transpose(1, 2), target.transpose(1, 2).contiguous().transpose(1, 2)
    assert not pt.is_contiguous() and _bits(DTW(pt, tt, c["s"], c["r"])) == _bits(want)
    half = DTW(pred.half(), target.half(), c["s"], c["r"])                                  # the goldens' inputs are exact in fp16
    assert half.dtype == torch.float16 and _bits(half) == _bits(want.half())
    out, info = DTW(pred.double(), target.double(), c["s"], c["r"], return_info=True)
    assert out.dtype == torch.float64 and set(info) == {"choice", "l1_before", "l1_after"} and all(v.is_cuda for v in info.values())
    assert torch.equal(out.float(), want)


def test_validate_with_dtw_target_equals_dtw_then_validate(hip_lib_path):
    """A toy vocoder that takes 40 mel + 40 logvar channels (train.py:232-236): only the mel half is warped."""
    from cookietts_amd import DTW, MelSpectrogramError, WaveGlow, synthetic, vocoder
    cfg = synthetic.WAVEGLOW_CONFIGS["toy"]
    model = WaveGlow(**cfg)
    model.load_state_dict(synthetic.to_torch(synthetic.waveglow_state_dict(cfg, seed=5)))
    model = model.cuda().eval()
    mels = torch.from_numpy(synthetic.synthetic_mel(2, 6, n_mel=80, seed=3)).cuda()
    noise = 0.02 * torch.randn(2, 40, 6, generator=torch.Generator().manual_seed(1))
    gt_mel = (torch.roll(mels[:, :40], 1, dims=2) + noise.cuda()).contiguous()            # the ground truth runs one frame behind
    metric = MelSpectrogramError((64, 96), 16, 8000, 12, 0.0, 4000.0).cuda()
    T = 6 * cfg["hop_length"]
    gt = _dev((0.3 * np.random.RandomState(0).randn(2, T)).clip(-0.9, 0.9).astype(np.float32))
    gl = [T, T - 300]
    for dtw_args, lengths in (((8, 5), None), ((5, 3), [6, 4])):
        mse, mae, out = vocoder.validate(model, mels, gt, gl, metric, sigma=0.7, dtw_target=gt_mel, dtw=dtw_args, dtw_lengths=lengths)
        warped = torch.cat((DTW(mels[:, :40], gt_mel, *dtw_args, lengths=lengths), mels[:, 40:]), dim=1)
        assert not torch.equal(warped, mels) and torch.equal(warped[:, 40:], mels[:, 40:])
        mse0, mae0, out0 = vocoder.validate(model, warped, gt, gl, metric, sigma=0.7)
        assert _bits(out["table"]) == _bits(out0["table"]) and (mse, mae) == (mse0, mae0)
