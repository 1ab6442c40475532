"""MelSpectrogramError on the device (csrc/mel_error.hip, cookietts_amd/mel_error.py) against the float64 restatement
(tests/mel_error_restatement.py), which tests/test_mel_error.py pins to the reference's own outputs (tests/golden/mel_error_*.npz).

The bound on every table entry and batch term is FACTOR * max(e32, 4 * 2^-23 * |y64|): y64 the float64 restatement, e32 the float32
reference's distance from it (the goldens' values where they hold one, the float32 arm of the restatement for SSE and the gt_mel
form), FACTOR = 8 - the project's bound (tests/test_taco_loss_gpu.py).  Every case appends (case, key, error, bound, ratio = error /
(bound / FACTOR)) to profiles/r28_mel_error_parity.jsonl; a ratio above 8 fails.

MEASURED RATIOS (MI355X, 81 values over the four golden cases and the gt_mel form): the worst is 1.13 of the allowed 8 (`real` item 0
window 1200 SSE), then 1.06 and 1.01 (the same pair's MAE and SAE); `small` and the "nv" cases stay below 0.5.  The sums are formed in
float64 on the device, so what is left is the float32 STFT and mel projection.  Maps: the worst L-infinity ratio against the float32
restatement's own error is 2.4 of the allowed 8 (`nv_small` item 1 pred_mel).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import REPO
import mel_error_restatement as mr

pytestmark = pytest.mark.gpu

PARITY_LOG = os.path.join(REPO, "profiles", "r28_mel_error_parity.jsonl")
_METRICS = {}


def _metric(case):
    """One packed object per case, shared by the tests (its state is the packed basis and cached workspaces only)."""
    if case not in _METRICS:
        from cookietts_amd import MelSpectrogramError
        _METRICS[case] = MelSpectrogramError(**mr.ctor_args(case)).cuda()
    return _METRICS[case]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _within(what, key, got, y64, e32, log):
    got, y64 = float(got), float(y64)
    b = float(mr.bound(e32, y64))
    err = abs(got - y64)
    ratio = err / (b / mr.FACTOR) if b > 0 else (0.0 if err == 0 else float("inf"))
    print(f"{what} {key}: {got:.12g} vs {y64:.12g}, error {err:.2e}, bound {b:.2e}, ratio {ratio:.3g}")
    log.append({"case": what, "key": key, "error": err, "bound": b, "ratio": ratio})
    return err <= b


def _check_parity(what, out, r64, r32, g=None):
    """Every table entry and batch term of one ``forward`` result; e32 from the goldens ``g`` where they hold the value."""
    log, ok = [], True
    tab = out["table"].numpy()
    try:
        assert tab.dtype == np.float64 and tab.shape == r64["table"].shape
        assert (tab[:, :, 0] == r64["table"][:, :, 0]).all(), (tab[:, :, 0], r64["table"][:, :, 0])          # n_frames: exact
        gold = {} if g is None else {1: g["sae32"], 3: g["mae32"], 4: g["mse32"]}
        B, W, _ = tab.shape
        for b in range(B):
            for w in range(W):
                for col in (1, 2, 3, 4):
                    y64 = r64["table"][b, w, col]
                    ref32 = gold[col][b, w] if col in gold else r32["table"][b, w, col]
                    ok &= _within(what, f"item {b} window {w} {mr.COLUMNS[col]}", tab[b, w, col], y64, abs(ref32 - y64), log)
        for key, gk in (("average_MSE", "average_MSE32"), ("average_MAE", "average_MAE32")):
            ref32 = float(g[gk]) if g is not None else r32[key]
            ok &= _within(what, key, out[key], r64[key], abs(ref32 - r64[key]), log)
        for w in range(W):
            ref32 = g["l1_32"][w] if g is not None else r32["l1"][w]
            ok &= _within(what, f"l1 window {w}", out["l1"][w], r64["l1"][w], abs(ref32 - r64["l1"][w]), log)
    finally:
        os.makedirs(os.path.dirname(PARITY_LOG), exist_ok=True)
        with open(PARITY_LOG, "a") as f:
            for row in log:
                f.write(json.dumps(row) + "\n")
    assert ok and max(r["ratio"] for r in log) <= mr.FACTOR, [r for r in log if r["ratio"] > mr.FACTOR]


@pytest.mark.parametrize("case", list(mr.CASES))
def test_score_matches_float64_and_reference_golden(hip_lib_path, case):
    c = mr.CASES[case]
    gt, pred, r64, r32 = mr.live(case)
    out = _metric(case)(_dev(pred), _dev(gt), pred_lengths=list(c["pred_lengths"]), gt_lengths=list(c["gt_lengths"]))
    assert isinstance(out["average_MSE"], float) and not out["table"].is_cuda
    _check_parity(case, out, r64, r32, mr.load_golden(case))


def test_gt_mel_form_matches_float64(hip_lib_path):
    """hifigan/train.py:208-210: the loader's y_mel (the reference's own float32 log-mel, from the goldens) against the generated
    audio; ``l1`` is F.l1_loss of the equal-length batch."""
    case = "nv_real"
    c, g = mr.CASES[case], mr.load_golden(case)
    gt, pred, _, _ = mr.live(case)
    r64, r32 = (mr.score(pred, None, c["pred_lengths"], None, dt, gt_mel=g["gt_mel32"], **mr.ctor_args(case)) for dt in (np.float64, np.float32))
    out = _metric(case)(_dev(pred), gt_mel=_dev(g["gt_mel32"]))
    _check_parity("nv_real gt_mel", out, r64, r32)
    with_audio = _metric(case)(_dev(pred), _dev(gt))
    assert abs(out["l1"][0] - with_audio["l1"][0]) <= 1e-5 * with_audio["l1"][0]        # y_mel is the float32 log-mel of that audio


@pytest.mark.parametrize("case", ["small", "nv_small"])
def test_maps(hip_lib_path, case):
    c = mr.CASES[case]
    gt, pred, r64, r32 = mr.live(case)
    m = _metric(case)
    out = m(_dev(pred), _dev(gt), pred_lengths=list(c["pred_lengths"]), gt_lengths=list(c["gt_lengths"]), return_maps=True)
    plain = m(_dev(pred), _dev(gt), pred_lengths=list(c["pred_lengths"]), gt_lengths=list(c["gt_lengths"]))
    assert torch.equal(out["table"], plain["table"])                                         # the maps change no number
    B, W = len(c["gt_lengths"]), len(c["windows"])
    fmax = int(r64["table"][:, :, 0].max())
    for key in ("mae_spec", "pred_mel", "gt_mel"):
        dev = out[key]
        assert dev.is_cuda and tuple(dev.shape) == (B, W, c["n_mel_channels"], fmax) and dev.dtype == torch.float32
        got = dev.cpu().numpy().astype(np.float64)
        for b in range(B):
            for w in range(W):
                y64, y32 = r64[key][b][w], r32[key][b][w]
                nf = y64.shape[1]
                e32 = np.abs(y32.astype(np.float64) - y64).max()
                err = np.abs(got[b, w, :, :nf] - y64).max()
                print(f"{case} {key} item {b} window {w}: Linf {err:.2e}, float32 restatement {e32:.2e}, ratio {err / e32:.3g}")
                assert err <= mr.FACTOR * e32, (key, b, w, err, e32)
                assert (got[b, w, :, nf:] == 0).all()                                          # exactly zero past the item's frames


def _bits(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("fill", [float("nan"), 1e30])
def test_row_does_not_depend_on_batch_or_padding(hip_lib_path, fill):
    c = mr.CASES["small"]
    gt, pred, _, _ = mr.live("small")
    m = _metric("small")
    gl, pl = list(c["gt_lengths"]), list(c["pred_lengths"])
    base = m.per_item(_dev(pred), _dev(gt), pred_lengths=pl, gt_lengths=gl)
    gt_f, pred_f = gt.copy(), pred.copy()
    for b in range(len(gl)):
        gt_f[b, gl[b]:] = fill
        pred_f[b, pl[b]:] = fill
    filled = m.per_item(_dev(pred_f), _dev(gt_f), pred_lengths=pl, gt_lengths=gl)
    assert torch.isfinite(filled).all()
    assert _bits(filled) == _bits(base)
    for b in range(len(gl)):                                                                 # alone, at its own width
        alone = m.per_item(_dev(pred[b:b + 1, :pl[b]]), _dev(gt[b:b + 1, :gl[b]]))
        assert _bits(alone[0]) == _bits(base[b]), b


def test_repeats_and_leaves_inputs_unchanged(hip_lib_path):
    c = mr.CASES["small"]
    gt, pred, _, _ = mr.live("small")
    pred = pred.copy()
    pred[0, 5], pred[1, 7], pred[2, 9] = np.nan, np.inf, 3.0                                 # what sanitising would rewrite in place
    m = _metric("small")
    p, g = _dev(pred), _dev(gt)
    pl, gl = torch.tensor(c["pred_lengths"]), torch.tensor(c["gt_lengths"])
    before = (_bits(p), _bits(g))
    a = m(p, g, pred_lengths=pl, gt_lengths=gl)
    b = m(p, g, pred_lengths=pl, gt_lengths=gl)
    assert _bits(a["table"]) == _bits(b["table"]) and a["average_MSE"] == b["average_MSE"] and a["l1"] == b["l1"]
    assert (_bits(p), _bits(g)) == before
    assert np.isfinite(a["table"].numpy()).all()


def test_sanitising(hip_lib_path):
    c = mr.CASES["small"]
    gt, pred, _, _ = mr.live("small")
    m = _metric("small")
    kw = dict(pred_lengths=list(c["pred_lengths"]), gt_lengths=list(c["gt_lengths"]))
    dirty = pred.copy()
    dirty[0, [3, 700, 2084]] = np.nan
    dirty[1, [0, 1000]] = [np.inf, -np.inf]
    dirty[2, [10, 129, 399]] = [3.0, -3.0, 3.0]
    by_hand = mr.sanitize(dirty).astype(np.float32)
    assert np.isfinite(by_hand).all() and np.abs(by_hand).max() == np.float32(0.999)
    a = m.per_item(_dev(dirty), _dev(gt), **kw)
    b = m.per_item(_dev(by_hand), _dev(gt), **kw)
    assert torch.isfinite(a).all() and _bits(a) == _bits(b)
    assert _bits(m.per_item(_dev(by_hand), _dev(gt), sanitize=False, **kw)) == _bits(b)
    clean_on, clean_off = m.per_item(_dev(pred), _dev(gt), **kw), m.per_item(_dev(pred), _dev(gt), sanitize=False, **kw)
    assert _bits(clean_on) == _bits(clean_off) and _bits(clean_on) != _bits(b)


@pytest.mark.parametrize("case", ["small", "nv_small"])
def test_digital_silence_scores_exactly_zero(hip_lib_path, case):
    c = mr.CASES[case]
    gt, pred, _, _ = mr.live(case)
    gt, pred = gt.copy(), pred.copy()
    gt[1], pred[1] = 0.0, 0.0
    t = _metric(case).per_item(_dev(pred), _dev(gt), pred_lengths=list(c["pred_lengths"]), gt_lengths=list(c["gt_lengths"])).cpu()
    assert (t[1, :, 1:] == 0).all() and (t[1, :, 0] > 0).all()
    assert (t[0, :, 1:] > 0).all()


def test_device_lengths_score_the_shorter_count(hip_lib_path):
    """Lengths on the device are not checked: a generated item shorter than its ground truth scores min(gt, pred) frames."""
    gt, pred, _, _ = mr.live("small")
    m = _metric("small")
    pl = torch.tensor([1000, 2100, 400], dtype=torch.int64).cuda()                          # item 0: 63 frames against 131
    gl = torch.tensor([2085, 2032, 130], dtype=torch.int32).cuda()
    t = m.per_item(_dev(pred), _dev(gt), pred_lengths=pl, gt_lengths=gl).cpu()
    assert t[:, :, 0].tolist() == [[63.0, 63.0], [128.0, 128.0], [9.0, 9.0]]
    assert torch.isfinite(t).all()
    with pytest.raises(ValueError, match="fewer than the ground truth"):                     # the same lengths on the host are refused
        m.per_item(_dev(pred), _dev(gt), pred_lengths=pl.cpu(), gt_lengths=gl.cpu())
    wild = torch.tensor([10 ** 6, -5, 7], dtype=torch.int32).cuda()                          # read as the nearest bound; never out of a row
    t = m.per_item(_dev(pred), _dev(gt), pred_lengths=wild, gt_lengths=gl).cpu()
    assert t[:, :, 0].tolist() == [[131.0, 131.0], [1.0, 1.0], [1.0, 1.0]] and torch.isfinite(t).all()


def test_c_abi_refusals(hip_lib_path):
    from cookietts_amd import _lib
    lib = _lib.lib()
    m = _metric("small")
    gt, pred, _, _ = mr.live("small")
    p, g = _dev(pred), _dev(gt)
    m.per_item(p, g)                                                                         # packs the basis
    cfg = m._config()
    blob = m._packed[p.device]
    B, Tp, Tg = 3, pred.shape[1], gt.shape[1]
    need = lib.ctts_mel_error_workspace_bytes(C.byref(cfg), B, Tp, Tg)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    table = torch.full((B * 2 * 5 + 10,), -1.0, dtype=torch.float64, device="cuda")
    pl = torch.full((B,), Tp, dtype=torch.int32, device="cuda")
    gl = torch.full((B,), Tg, dtype=torch.int32, device="cuda")
    stream = _lib.stream(p.device)

    def call(packed=blob, pred_=p, table_=table, ws_bytes=need, gt_=g, gt_mel=None):
        return lib.ctts_mel_error_f32(C.byref(cfg), _lib.ptr(packed), _lib.ptr(pred_), _lib.ptr(pl), _lib.ptr(gt_), _lib.ptr(gl),
                                      _lib.ptr(gt_mel), 1, B, Tp, Tg, 0, _lib.ptr(table_), None, None, None, 0, _lib.ptr(ws), ws_bytes,
                                      stream)
    assert call(ws_bytes=need - 1) == -3 and "workspace" in _lib.last_error()                # CTTS_E_WORKSPACE
    assert call(pred_=None) == -1 and "NULL argument" in _lib.last_error()
    assert call(table_=None) == -1 and "NULL argument" in _lib.last_error()
    assert call(gt_=None) == -1 and "exactly one of gt and gt_mel" in _lib.last_error()
    assert call(gt_mel=g) == -1 and "exactly one of gt and gt_mel" in _lib.last_error()
    torch.cuda.synchronize()
    assert (table == -1.0).all()                                                             # a refused call launches nothing
    assert call() == 0
    assert _bits(table[:B * 2 * 5]) == _bits(m.per_item(p, g).reshape(-1))


def test_vocoder_validate(hip_lib_path):
    from cookietts_amd import MelSpectrogramError, WaveGlow, synthetic, vocoder
    cfg = synthetic.WAVEGLOW_CONFIGS["toy"]
    model = WaveGlow(**cfg)
    model.load_state_dict(synthetic.to_torch(synthetic.waveglow_state_dict(cfg, seed=5)))
    model = model.cuda().train()
    mels = torch.from_numpy(synthetic.synthetic_mel(2, 6, n_mel=80, seed=3)).cuda()
    metric = MelSpectrogramError((64, 96), 16, 8000, 12, 0.0, 4000.0).cuda()
    T = 6 * cfg["hop_length"]
    rng = np.random.RandomState(0)
    gt = _dev((0.3 * rng.randn(2, T)).clip(-0.9, 0.9).astype(np.float32))
    gl = [T, T - 300]
    torch.manual_seed(123)
    cpu_state, cuda_state = torch.random.get_rng_state(), torch.cuda.get_rng_state()
    mse, mae, out = vocoder.validate(model, mels, gt, gl, metric, sigma=0.7)
    assert torch.equal(torch.random.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(), cuda_state)
    assert model.training                                                                    # the mode is put back
    model.eval()
    with torch.no_grad(), torch.random.fork_rng(devices=[torch.cuda.current_device()]):
        torch.random.manual_seed(0)
        audio = model.infer(mels, None, sigma=0.7)
    ref = metric(audio, gt, gt_lengths=gl)
    assert _bits(out["table"]) == _bits(ref["table"]) and (mse, mae) == (ref["average_MSE"], ref["average_MAE"])
    assert mse == out["average_MSE"] and mae == out["average_MAE"] and np.isfinite(mse) and mse > 0
    vocoder.validate(model, mels, gt, gl, metric, sigma=0.7)
    assert not model.training
