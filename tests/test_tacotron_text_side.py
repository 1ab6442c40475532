"""Tacotron2 text side (embedding gather, conv + BatchNorm + LeakyReLU, packed BiLSTM, memory assembly) against a float64
restatement, at every batch form of the BiLSTM: the VALU step kernels (<= 4 items, any H % 4 == 0) and the three launch shapes
of the batched MFMA form (<= 16, <= 32 and k x 64 padded rows; H % 64 == 0).

Reference: tests/lstm_seq_restatement.py (numpy, vectorised over the batch), pinned here on the CPU to the reference's own
outputs (tests/golden/tacotron_full.npz, 1e-6) and to ``oracle.tacotron_oracle.encoder``.

Bound of every comparison against float64: with e32 = the L-inf distance of the float32 restatement from the float64 one on
the same inputs (the reference's own rounding, never the code under test), the HIP result must be within
``max(FACTOR * e32, 4 * 2^-23 * max|y64|)`` of float64, FACTOR = 8 (summation order: K over four waves, chained 16x16x4 MFMAs,
the conv-GEMM's input projection; device expf / tanhf).  Every GPU test prints e32 and the HIP error.

Weights are chosen so that the checks are not vacuous (asserted on the reference alone): zeroing W_hh moves the float64
outputs by >= 1000 x the bound, and at model level ``encoder.sylps_layer`` has a non-zero weight so that pred_sylps depends on
the BiLSTM's final states (spread over the batch >= 1000 x its bound, minimum > 1 so that its logarithm is tame).

Measured on the MI355X: the HIP error is 0.4 ... 1.8 x e32 in every comparison (tables in the docstrings of
``test_bilstm_operator_matches_float64`` and ``test_assemble_memory_matches_float64``), so FACTOR stays 8.  The bit-equality
properties hold: one bidirectional launch == two one-direction runs (B = 17, 65), a second run, and a permutation of the items
(B = 33).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from cookietts_amd import synthetic
from oracle import tacotron_oracle as to
import lstm_seq_restatement as tsr

FACTOR = 8                       # see the module docstring (measured: 1.8 at most); beyond 32 an error is a finding, not a tolerance
EPS32 = 2.0 ** -23
SENTINEL = -7.0                  # what out / hn hold before the call: no LSTM output (|h| < 1) can equal it


def _bound(y32, y64):
    """(e32, bound) of one comparison against float64."""
    e32 = float(np.abs(np.asarray(y32, np.float64) - y64).max())
    return e32, max(FACTOR * e32, 4 * EPS32 * float(np.abs(y64).max()))


def _uniform(rng, shape, bound):
    return ((rng.random(shape, dtype=np.float32) * 2.0 - 1.0) * np.float32(bound)).astype(np.float32)


def _ragged(rng, B, T, must):
    """Unsorted lengths in 1..T that contain every value of ``must`` (as many of them as there are items)."""
    lens = rng.integers(1, T + 1, size=B)
    where = rng.permutation(B)[:len(must)]
    lens[where] = must[:len(where)]
    while B > 2 and lens.min() < lens.max() and (np.all(np.diff(lens) >= 0) or np.all(np.diff(lens) <= 0)):
        lens = rng.permutation(lens)
    return lens.astype(np.int64)


# ---------------------------------------------------------------------------------------------------- CPU: the restatement ----
def _golden_sd():
    import json
    g = np.load(os.path.join(GOLDEN, "tacotron_full.npz"))
    hp = synthetic.tacotron_hparams()
    shapes = json.load(open(os.path.join(GOLDEN, "tacotron_state_shapes.json")))
    return g, hp, synthetic.tacotron_state_dict(hp, seed=int(g["seed"]), shapes=shapes)


def test_float32_restatement_matches_reference_golden():
    """The bound of test_oracle_full_model_matches_reference_golden (1e-6) on the reference's own encoder outputs / pred_sylps."""
    g, hp, sd = _golden_sd()
    o = tsr.text_side(sd, hp, g["text"], g["lengths"], g["speakers"], g["torchmoji"], None, np.float32)
    assert o["encoder_outputs"].dtype == np.float32 and o["memory_in"].shape == (3, 30, synthetic.tacotron_memory_in_dim(hp))
    assert np.abs(o["encoder_outputs"] - g["encoder_outputs"]).max() < 1e-6
    assert np.abs(o["pred_sylps"] - g["pred_sylps"]).max() < 1e-6
    assert (o["encoder_outputs"][1, 22:] == 0).all() and (o["encoder_outputs"][2, 9:] == 0).all()


def test_restatement_agrees_with_the_oracle_encoder_on_a_ragged_unsorted_batch():
    """Same equations as the oracle's per-item walk (only the order of the sums inside the BLAS calls differs), with a sylps
    head that reads hn: outputs, hn (through pred_sylps) and the assembled memory."""
    hp = synthetic.tacotron_hparams(**synthetic.TACOTRON_SMALL_OVERRIDES)
    sd = _text_side_weights("small")[1]
    rng = np.random.default_rng(11)
    B, T = 5, 13
    lens = np.array([4, 13, 1, 9, 12])
    text = rng.integers(0, hp.n_symbols, size=(B, T))
    spk = rng.integers(0, hp.n_speakers, size=B)
    tm = rng.standard_normal((B, hp.torchMoji_attDim)).astype(np.float32)
    want_out, want_sylps = to.encoder({k: np.asarray(v) for k, v in sd.items()}, hp, text, lens, spk)
    got = tsr.text_side(sd, hp, text, lens, spk, tm, None, np.float32)
    assert np.abs(got["encoder_outputs"] - want_out).max() < 1e-6
    assert np.abs(got["pred_sylps"] - want_sylps).max() < 2e-6                    # values near 4: a few ulp
    assert float(np.ptp(want_sylps)) > 1e-2                                       # ... and hn really is read
    want_mem = to.memory_assemble({k: np.asarray(v) for k, v in sd.items()}, hp, want_out, want_sylps, spk, tm)
    assert np.abs(got["memory_in"] - want_mem).max() < 2e-6
    for b in range(B):
        assert (got["encoder_outputs"][b, lens[b]:] == 0).all()
    # gt_sylps feeds the SylpsNet; pred_sylps stays the predicted one and nothing but the sylzu column moves
    gt = np.linspace(2.0, 3.0, B).astype(np.float32)
    got_gt = tsr.text_side(sd, hp, text, lens, spk, tm, gt, np.float32)
    want_gt = to.memory_assemble({k: np.asarray(v) for k, v in sd.items()}, hp, want_out, gt[:, None], spk, tm)
    assert np.array_equal(got_gt["pred_sylps"], got["pred_sylps"]) and np.abs(got_gt["memory_in"] - want_gt).max() < 2e-6
    col = hp.encoder_LSTM_dim + hp.speaker_embedding_dim
    assert np.array_equal(np.delete(got_gt["memory_in"], col, axis=2), np.delete(got["memory_in"], col, axis=2))
    assert np.abs(got_gt["memory_in"][:, :, col] - got["memory_in"][:, :, col]).min() > 0.5
    with to.precision(np.float64):                                                # float64 really is float64
        sd64 = tsr.cast_state_dict(sd, np.float64)
        o64, s64 = to.encoder(sd64, hp, text, lens, spk)
    got64 = tsr.text_side(sd, hp, text, lens, spk, tm, None, np.float64)
    assert got64["encoder_outputs"].dtype == np.float64
    assert np.abs(got64["encoder_outputs"] - o64).max() < 1e-13 and np.abs(got64["pred_sylps"] - s64).max() < 1e-13


# ------------------------------------------------------------------------------------------------- operator-level cases ----
# (I, H, B, T, lengths that must occur)
OP_CASES = [
    (32, 64, 5, 12, None),         # smallest H on the batched form; one chunk per wave
    (32, 64, 16, 12, None),        # a full tile
    (32, 192, 17, 12, None),       # 32-row shape; second tile holds one item; three chunks per wave (odd)
    (32, 192, 33, 12, None),       # 64-row shape; tiles 3 and 4 ragged or empty
    (1024, 512, 65, 20, None),     # the model's size; grid.y = 2
    (32, 64, 256, 6, None),        # the maximum batch
    (32, 64, 5, 129, None),        # two 128-column tiles of the input projection
    # VALU form; H not a multiple of 64; padded fourth row; tail slab.  Three items cannot hold 1, 128, 129 and T = 130 at once:
    # the case runs with two sets of lengths that cover them between them
    (16, 72, 3, 130, (129, 1, 130)),
    (16, 72, 3, 130, (128, 130, 1)),
    (32, 64, 1, 1, None),
    (32, 64, 2, 5, None),
]
OP_IDS = [f"I{c[0]}-H{c[1]}-B{c[2]}-T{c[3]}" + ("" if c[4] is None else "-len" + "_".join(map(str, c[4]))) for c in OP_CASES]
CASE_B17, CASE_B33, CASE_B65 = OP_CASES[2], OP_CASES[3], OP_CASES[4]


@functools.lru_cache(maxsize=None)
def _op_case(case):
    """Inputs and the float64 / float32 references of one operator case, computed once.  The conditions on the inputs are
    asserted here, on the reference alone."""
    I, H, B, T, fixed = case
    rng = np.random.default_rng(1000 * H + 10 * B + T)
    x = rng.standard_normal((B, T, I)).astype(np.float32)
    dirs = [(_uniform(rng, (4 * H, I), 1 / np.sqrt(I)), _uniform(rng, (4 * H, H), 2 / np.sqrt(H)),
             _uniform(rng, (4 * H,), 0.5), _uniform(rng, (4 * H,), 0.5)) for _ in range(2)]
    if fixed is not None:
        lens = np.array(fixed, np.int64)
    else:
        must = [1, T] + ([128, 129] if T > 128 else [])
        lens = _ragged(rng, B, T, must[:1] if B == 1 and T == 1 else must[1:] if B == 1 else must)
    out64, hn64 = tsr.bilstm(x, lens, dirs[0], dirs[1], np.float64)
    out32, hn32 = tsr.bilstm(x, lens, dirs[0], dirs[1], np.float32)
    assert out64.dtype == np.float64 and out32.dtype == np.float32
    e32, bound = _bound(np.concatenate([out32.ravel(), hn32.ravel()]), np.concatenate([out64.ravel(), hn64.ravel()]))
    ref = dict(I=I, H=H, B=B, T=T, x=x, dirs=dirs, lens=lens, out64=out64, hn64=hn64, e32=e32, bound=bound)
    # the lengths are what the case asks for
    assert lens.min() >= 1 and lens.max() == T and (B == 1 or lens.min() == 1)
    if T > 128 and fixed is None:
        assert 128 in lens and 129 in lens
    if B > 2:
        assert not np.all(np.diff(lens) >= 0) and not np.all(np.diff(lens) <= 0)
    # zeroing W_hh moves the float64 outputs by >= 1000 x the bound (T = 1 has no recurrent product to check: h0 = 0)
    if T > 1:
        no_hh = [(d[0], np.zeros_like(d[1]), d[2], d[3]) for d in dirs]
        out0, hn0 = tsr.bilstm(x, lens, no_hh[0], no_hh[1], np.float64)
        ref["hh_moves"] = float(np.abs(out0 - out64).max())
        assert ref["hh_moves"] >= 1000 * bound, (ref["hh_moves"], bound)
        assert float(np.abs(hn0 - hn64).max()) >= 1000 * bound
    return ref


@pytest.mark.parametrize("case", OP_CASES, ids=OP_IDS)
def test_operator_case_inputs_meet_the_conditions(case):
    r = _op_case(case)
    print(f"{case}: e32 {r['e32']:.3g} bound {r['bound']:.3g} zeroing W_hh moves the outputs by {r.get('hh_moves', float('nan')):.3g}")
    assert 0 < r["e32"] < 2e-6 and r["bound"] < 2e-5                            # fp32 rounding, not a tolerance of 1e-4


def test_deliberately_wrong_references_are_outside_the_bound():
    """Proof that the parity tests can fail, on the reference side only: each of these slips, made in the restatement, is far
    outside the bound the HIP result is held to."""
    for case in (OP_CASES[0], CASE_B17):
        r = _op_case(case)
        H, T, x, lens, dirs, bound = r["H"], r["T"], r["x"], r["lens"], r["dirs"], r["bound"]
        assert (lens < T).any()
        # the reverse direction indexed from T - 1 instead of len - 1
        out, hn = tsr.bilstm(x, lens, dirs[0], dirs[1], np.float64, mutation="reverse_from_T")
        assert np.array_equal(out[:, :, :H], r["out64"][:, :, :H])              # (the forward direction is untouched)
        err = float(np.abs(out[:, :, H:] - r["out64"][:, :, H:]).max())
        assert err > 1000 * bound and float(np.abs(hn[:, H:] - r["hn64"][:, H:]).max()) > 1000 * bound, (err, bound)
        # hn taken at step T - 1
        out, hn = tsr.bilstm(x, lens, dirs[0], dirs[1], np.float64, mutation="hn_at_T")
        assert np.array_equal(out, r["out64"])
        err = float(np.abs(hn[:, :H] - r["hn64"][:, :H]).max())
        assert err > 1000 * bound, (err, bound)
        # the last 16 columns of W_hh dropped (one K chunk of one wave)
        cut = []
        for d in dirs:
            w_hh = d[1].copy()
            w_hh[:, -16:] = 0
            cut.append((d[0], w_hh, d[2], d[3]))
        out, hn = tsr.bilstm(x, lens, cut[0], cut[1], np.float64)
        err = float(np.abs(out - r["out64"]).max())
        print(f"{case}: 16 columns of W_hh dropped move the outputs by {err:.3g}; bound {bound:.3g}")
        assert err > 1000 * bound and float(np.abs(hn - r["hn64"]).max()) > 1000 * bound, (err, bound)


# ------------------------------------------------------------------------------------------------ operator level on the GPU ----
_DEV_CACHE = {}


def _dev_case(case):
    """Packed weights and the padded device input of a case (kept: several tests run the same case)."""
    if case in _DEV_CACHE:
        return _DEV_CACHE[case]
    from cookietts_amd import _lib
    from cookietts_amd.tacotron2 import PAD, _ld_for
    r = _op_case(case)
    I, H, B, T = r["I"], r["H"], r["B"], r["T"]
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    ld = _ld_for(T)
    packs = []
    with torch.cuda.device(dev):
        for d in r["dirs"]:
            ts = [torch.from_numpy(a).to(dev).contiguous() for a in d]
            w = _lib.LstmWeights(*[t.data_ptr() for t in ts])
            blob = torch.zeros(_lib.nbytes(lib.ctts_lstm_seq_packed_bytes, I, H, what="lstm_seq pack size") // 4,
                               dtype=torch.float32, device=dev)
            _lib.check(lib.ctts_lstm_seq_pack_f32(C.byref(w), I, H, _lib.ptr(blob), _lib.stream(dev)), "ctts_lstm_seq_pack_f32")
            torch.cuda.current_stream(dev).synchronize()
            packs.append(blob)
    x = torch.zeros(B, I, ld, dtype=torch.float32, device=dev)
    x[:, :, PAD:PAD + T] = torch.from_numpy(np.ascontiguousarray(r["x"].transpose(0, 2, 1))).to(dev)
    _DEV_CACHE[case] = (packs, x, ld)
    return _DEV_CACHE[case]


def _hip_bilstm(case, one_launch=True, perm=None):
    """Run the case through ``ctts_lstm_biseq_f32`` (or two ``ctts_lstm_seq_f32`` calls) into hostile buffers:
    rows of 2H + 5 columns, out / hn pre-filled with SENTINEL, both workspaces pre-filled with NaN.  ``perm``: item order."""
    from cookietts_amd import _lib
    from cookietts_amd.tacotron2 import PAD
    r = _op_case(case)
    I, H, B, T = r["I"], r["H"], r["B"], r["T"]
    packs, x, ld = _dev_case(case)
    dev = x.device
    lib = _lib.lib()
    lens_np = r["lens"]
    if perm is not None:
        x = x[torch.from_numpy(perm).to(dev)].contiguous()
        lens_np = lens_np[perm]
    lens = torch.from_numpy(lens_np.astype(np.int32)).to(dev)
    row = 2 * H + 5
    nbytes = _lib.nbytes(lib.ctts_lstm_seq_workspace_bytes, H, B, ld, what="lstm_seq workspace size")
    out = torch.full((B, T, row), SENTINEL, dtype=torch.float32, device=dev)
    hn = torch.full((B, 2 * H), SENTINEL, dtype=torch.float32, device=dev)
    ws = torch.full((2, nbytes // 4), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = _lib.stream(dev)
        if one_launch:
            _lib.check(lib.ctts_lstm_biseq_f32(_lib.ptr(packs[0]), _lib.ptr(packs[1]), _lib.ptr(x), _lib.ptr(lens), _lib.ptr(out),
                                               T * row, row, 0, H, _lib.ptr(hn), 2 * H, 0, H, B, T, I, H, ld, PAD, _lib.ptr(ws[0]),
                                               _lib.ptr(ws[1]), nbytes, st), "ctts_lstm_biseq_f32")
        else:
            for d in range(2):
                _lib.check(lib.ctts_lstm_seq_f32(_lib.ptr(packs[d]), _lib.ptr(x), _lib.ptr(lens), d, _lib.ptr(out), T * row, row,
                                                 d * H, _lib.ptr(hn), 2 * H, d * H, B, T, I, H, ld, PAD, _lib.ptr(ws[d]), nbytes,
                                                 st), "ctts_lstm_seq_f32")
        torch.cuda.synchronize()
    return out.cpu().numpy(), hn.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _hip_case(case):
    return _hip_bilstm(case)


def _check_against_float64(out, hn, r, what):
    H, B, T, lens = r["H"], r["B"], r["T"], r["lens"]
    assert out.shape == (B, T, 2 * H + 5) and hn.shape == (B, 2 * H)
    assert (out[:, :, 2 * H:] == SENTINEL).all(), "the five extra columns of a row were written"
    mask = np.arange(T)[None, :] < lens[:, None]                                # [B, T]
    assert (out[:, :, :2 * H][~mask] == SENTINEL).all(), "out was written beyond an item's length"
    err_out = float(np.abs(np.where(mask[:, :, None], out[:, :, :2 * H] - r["out64"], 0.0)).max())
    err_hn = float(np.abs(hn - r["hn64"]).max())
    print(f"{what}: e32 {r['e32']:.3g}  HIP out {err_out:.3g} hn {err_hn:.3g}  bound {r['bound']:.3g} "
          f"(HIP / e32 = {max(err_out, err_hn) / r['e32']:.2f}, factor {FACTOR})")
    assert np.isfinite(out).all() and np.isfinite(hn).all()
    assert err_out <= r["bound"], (err_out, r["bound"])
    assert err_hn <= r["bound"], (err_hn, r["bound"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", OP_CASES, ids=OP_IDS)
def test_bilstm_operator_matches_float64(hip_lib_path, case):
    """``ctts_lstm_biseq_f32``: out and hn of both directions against the float64 BiLSTM; nothing written beyond a length or in
    the five extra columns; NaN-filled workspaces (what the call needs it zeroes itself).

    Measured on the MI355X (factor in use 8; the largest HIP error is 1.8 x e32):
        (I, H, B, T)            e32       HIP out   HIP hn    bound
        (32, 64, 5, 12)         1.30e-07  1.62e-07  1.01e-07  1.04e-06
        (32, 64, 16, 12)        1.55e-07  1.41e-07  1.02e-07  1.24e-06
        (32, 192, 17, 12)       2.11e-07  1.46e-07  1.26e-07  1.68e-06
        (32, 192, 33, 12)       2.62e-07  2.03e-07  2.03e-07  2.10e-06
        (1024, 512, 65, 20)     7.82e-07  1.15e-06  9.51e-07  6.26e-06
        (32, 64, 256, 6)        1.90e-07  1.50e-07  1.50e-07  1.52e-06
        (32, 64, 5, 129)        1.70e-07  1.70e-07  7.86e-08  1.36e-06
        (16, 72, 3, 130) a      1.52e-07  1.27e-07  8.97e-08  1.21e-06
        (16, 72, 3, 130) b      2.08e-07  1.70e-07  7.24e-08  1.66e-06
        (32, 64, 1, 1)          3.31e-08  5.94e-08  5.94e-08  2.65e-07
        (32, 64, 2, 5)          1.02e-07  1.48e-07  8.43e-08  8.13e-07"""
    _check_against_float64(*_hip_case(case), _op_case(case), f"biseq {case}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CASE_B17, CASE_B65], ids=["B17", "B65"])
def test_batched_one_direction_launch_equals_the_bidirectional_one(hip_lib_path, case):
    """``ctts_lstm_seq_f32`` above four items (``bg_launch_seq(a, a, 1, ...)``): two one-direction runs give what the one
    bidirectional launch per step gives, bit for bit - and so the one-direction launch meets the float64 bound too."""
    out2, hn2 = _hip_bilstm(case, one_launch=False)
    out1, hn1 = _hip_case(case)
    _check_against_float64(out2, hn2, _op_case(case), f"2 x seq {case}")
    assert np.array_equal(out1, out2) and np.array_equal(hn1, hn2)


@pytest.mark.gpu
def test_batched_bilstm_is_deterministic_and_independent_of_the_item_order(hip_lib_path):
    """B = 33 (64-row shape, ragged and empty tiles): a second run is bit-identical, and a permutation of the items gives the
    permuted result bit for bit - an item's sums do not depend on the MFMA column or the tile it sits in."""
    out, hn = _hip_case(CASE_B33)
    again = _hip_bilstm(CASE_B33)
    assert np.array_equal(out, again[0]) and np.array_equal(hn, again[1])
    perm = np.random.default_rng(33).permutation(CASE_B33[2])
    assert (perm != np.arange(CASE_B33[2])).sum() > 24 and (perm // 16 != np.arange(CASE_B33[2]) // 16).any()
    outp, hnp = _hip_bilstm(CASE_B33, perm=perm)
    assert np.array_equal(outp, out[perm]) and np.array_equal(hnp, hn[perm])


# ----------------------------------------------------------------------------------------------------------- model level ----
MODEL_T = 24
H72_OVERRIDES = dict(symbols_embedding_dim=48, encoder_speaker_embed_dim=16, encoder_conv_hidden_dim=64, encoder_LSTM_dim=144)
_HPARAMS = {"default": {}, "small": synthetic.TACOTRON_SMALL_OVERRIDES, "h72": H72_OVERRIDES}
MODEL_CASES = [("default", 3), ("default", 5), ("default", 17), ("default", 33), ("default", 70), ("small", 17)]
MODEL_IDS = [f"{n}-B{b}" for n, b in MODEL_CASES]


@functools.lru_cache(maxsize=None)
def _text_side_weights(name):
    """(hparams, state dict) of the plain synthetic recipe with a BiLSTM that saturates a little (weight_ih x 8, weight_hh x 2)
    and a sylps head that reads hn (weight ~ U(+-4 / sqrt(enc_dim)), bias stays 4.0)."""
    hp = synthetic.tacotron_hparams(**_HPARAMS[name])
    sd = dict(synthetic.tacotron_state_dict(hp, seed=4321))
    rng = np.random.default_rng(99)
    for k in sorted(sd):
        if k.startswith("encoder.lstm.weight_ih_l0"):
            sd[k] = (sd[k] * np.float32(8)).astype(np.float32)
        elif k.startswith("encoder.lstm.weight_hh_l0"):
            sd[k] = (sd[k] * np.float32(2)).astype(np.float32)
    k = "encoder.sylps_layer.linear_layer.weight"
    sd[k] = _uniform(rng, sd[k].shape, 4 / np.sqrt(hp.encoder_LSTM_dim))
    assert float(sd["encoder.sylps_layer.linear_layer.bias"][0]) == 4.0
    return hp, sd


@functools.lru_cache(maxsize=None)
def _model_case(name, B):
    """Inputs and float64 / float32 references of a model-level case, with and without gt_sylps; the conditions on the inputs
    are asserted here, on the reference alone."""
    hp, sd = _text_side_weights(name)
    T = MODEL_T
    rng = np.random.default_rng(7000 + B)
    text = rng.integers(0, hp.n_symbols, size=(B, T))
    lens = _ragged(rng, B, T, [1, T])
    spk = rng.integers(0, hp.n_speakers, size=B)
    tm = rng.standard_normal((B, hp.torchMoji_attDim)).astype(np.float32)
    gt = (1.5 + rng.random(B)).astype(np.float32)
    assert lens.min() == 1 and lens.max() == T and not np.all(np.diff(lens) >= 0) and not np.all(np.diff(lens) <= 0)
    r = dict(hp=hp, sd=sd, text=text, lens=lens, spk=spk, tm=tm, gt=gt, B=B, T=T)
    r64 = tsr.text_side(sd, hp, text, lens, spk, tm, None, np.float64)
    r32 = tsr.text_side(sd, hp, text, lens, spk, tm, None, np.float32)
    assert r64["memory_in"].dtype == np.float64 and r32["memory_in"].dtype == np.float32
    r["r64"] = r64
    r["gt64"] = tsr.assemble(sd, hp, r64["encoder_outputs"], r64["pred_sylps"], spk, tm, gt, np.float64)
    gt32 = tsr.assemble(sd, hp, r32["encoder_outputs"], r32["pred_sylps"], spk, tm, gt, np.float32)
    assert float(np.abs(gt[:, None] - r64["pred_sylps"]).min()) > 0.1            # a given value is never the predicted one
    r["bounds"] = {k: _bound(r32[k], r64[k]) for k in ("encoder_outputs", "hn", "pred_sylps", "memory_in")}
    r["bounds"]["memory_in_gt"] = _bound(gt32, r["gt64"])
    # zeroing W_hh moves the float64 encoder outputs by >= 1000 x the bound
    sd0 = dict(sd)
    for k in sd:
        if k.startswith("encoder.lstm.weight_hh_l0"):
            sd0[k] = np.zeros_like(sd[k])
    out0, _, _ = tsr.encoder_side(sd0, hp, text, lens, spk, np.float64)
    r["hh_moves"] = float(np.abs(out0 - r64["encoder_outputs"]).max())
    assert r["hh_moves"] >= 1000 * max(r["bounds"]["encoder_outputs"][1], r["bounds"]["memory_in"][1]), r["hh_moves"]
    # pred_sylps depends on hn: its spread over the batch is >= 1000 x its bound; its minimum is above 1
    syl = r64["pred_sylps"]
    r["sylps_spread"] = float(np.ptp(syl))
    assert r["sylps_spread"] >= 1000 * r["bounds"]["pred_sylps"][1] and float(syl.min()) > 1.0, (r["sylps_spread"], syl.min())
    return r


@pytest.mark.parametrize("name,B", MODEL_CASES + [("h72", 6)], ids=MODEL_IDS + ["h72-B6"])
def test_model_case_inputs_meet_the_conditions(name, B):
    r = _model_case(name, B)
    print(f"{name} B={B}: (e32, bound) {r['bounds']}; zeroing W_hh moves the outputs by {r['hh_moves']:.3g}; pred_sylps "
          f"spread {r['sylps_spread']:.3g}, min {float(r['r64']['pred_sylps'].min()):.3g}")
    assert all(0 < e32 < 5e-6 and bound < 5e-5 for e32, bound in r["bounds"].values())


_GPU_MODELS = {}


def _gpu_model(name):
    if name not in _GPU_MODELS:
        from cookietts_amd.tacotron2 import Tacotron2
        hp, sd = _text_side_weights(name)
        m = Tacotron2(hp)
        m.load_state_dict(synthetic.to_torch(sd))
        _GPU_MODELS[name] = m.cuda().eval()
    return _GPU_MODELS[name]


def _report(what, got, want64, e32_bound):
    e32, bound = e32_bound
    err = float(np.abs(got - want64).max())
    print(f"{what}: e32 {e32:.3g}  HIP {err:.3g}  bound {bound:.3g} (HIP / e32 = {err / e32:.2f}, factor {FACTOR})")
    return err, bound


@pytest.mark.gpu
@pytest.mark.parametrize("name,B", MODEL_CASES, ids=MODEL_IDS)
def test_assemble_memory_matches_float64(hip_lib_path, name, B):
    """``Tacotron2._assemble_memory`` (no decoder run): the whole memory tensor - rows past each length included: encoder part
    exactly zero, per-utterance columns present - and pred_sylps against float64, with and without gt_sylps.  Given gt_sylps,
    pred_sylps is still the predicted one and only the sylzu column changes.

    Measured on the MI355X (e32 / HIP error per comparison; factor in use 8; the largest HIP error is 1.83 x e32):
        case          encoder_outputs      memory               pred_sylps           memory (gt_sylps)
        default B=3   3.09e-07 / 4.20e-07  4.76e-07 / 4.20e-07  2.25e-07 / 2.25e-07  4.76e-07 / 4.20e-07
        default B=5   2.45e-07 / 4.25e-07  4.30e-07 / 4.25e-07  3.80e-07 / 3.80e-07  4.30e-07 / 4.25e-07
        default B=17  2.54e-07 / 4.65e-07  8.36e-07 / 4.65e-07  3.86e-07 / 3.51e-07  8.36e-07 / 4.65e-07
        default B=33  2.89e-07 / 4.99e-07  1.06e-06 / 5.84e-07  4.11e-07 / 4.14e-07  1.06e-06 / 4.99e-07
        default B=70  2.96e-07 / 5.23e-07  1.25e-06 / 5.42e-07  3.83e-07 / 5.39e-07  1.25e-06 / 5.23e-07
        small B=17    2.64e-07 / 4.35e-07  4.16e-07 / 4.35e-07  2.21e-07 / 3.38e-07  4.16e-07 / 4.35e-07"""
    r = _model_case(name, B)
    m = _gpu_model(name)
    hp, lens = r["hp"], r["lens"]
    args = [torch.from_numpy(r[k]).cuda() for k in ("text", "lens", "spk", "tm")]
    mem, syl, enc_dim = m._assemble_memory(*args, None)
    mem_gt, syl_gt, _ = m._assemble_memory(*args, torch.from_numpy(r["gt"]).cuda())
    mem, syl, mem_gt, syl_gt = (t.cpu().numpy() for t in (mem, syl, mem_gt, syl_gt))
    assert enc_dim == hp.encoder_LSTM_dim and mem.shape == r["r64"]["memory_in"].shape and syl.shape == (B, 1)
    fails = []
    for what, got, want, key in ((f"{name} B={B} encoder_outputs", mem[:, :, :enc_dim], r["r64"]["encoder_outputs"], "encoder_outputs"),
                                 (f"{name} B={B} memory", mem, r["r64"]["memory_in"], "memory_in"),
                                 (f"{name} B={B} pred_sylps", syl, r["r64"]["pred_sylps"], "pred_sylps"),
                                 (f"{name} B={B} memory (gt_sylps)", mem_gt, r["gt64"], "memory_in_gt")):
        err, bound = _report(what, got, want, r["bounds"][key])
        if not err <= bound:
            fails.append((what, err, bound))
    assert not fails, fails
    for b in range(B):                                                           # pad_packed_sequence zeros, exactly
        assert (mem[b, lens[b]:, :enc_dim] == 0).all() and (mem_gt[b, lens[b]:, :enc_dim] == 0).all()
    # gt_sylps: pred_sylps is still the predicted one, and only the sylzu column of the memory changes
    col = enc_dim + hp.speaker_embedding_dim
    assert np.array_equal(syl_gt, syl)
    assert np.array_equal(np.delete(mem_gt, col, axis=2), np.delete(mem, col, axis=2))
    assert (np.abs(mem_gt[:, :, col] - mem[:, :, col]).min(axis=1) > 1e-3).all()


@pytest.mark.gpu
def test_encoder_without_a_batched_form_runs_groups_of_four(hip_lib_path):
    """``Encoder.forward_into_memory`` with encoder_LSTM_dim = 144 (H = 72: no batched form) at B = 6: the host's groups of
    four plus two on the VALU step kernels, into the caller's own memory / hn buffers, against float64.
    Measured on the MI355X (e32 / HIP error, factor 8): encoder_outputs 1.40e-07 / 1.52e-07, hn 1.05e-07 / 1.13e-07."""
    from cookietts_amd import _lib
    r = _model_case("h72", 6)
    m = _gpu_model("h72")
    hp, B, T, lens = r["hp"], r["B"], r["T"], r["lens"]
    enc = hp.encoder_LSTM_dim
    assert _lib.lib().ctts_lstm_seq_workspace_bytes(enc // 2, 6, 128 + 16) == 0       # really no batched form for this H
    row = enc + 7
    memory = torch.full((B, T, row), SENTINEL, dtype=torch.float32, device="cuda")
    hn = torch.full((B, enc), SENTINEL, dtype=torch.float32, device="cuda")
    m.encoder.forward_into_memory(m.embedding.weight, *[torch.from_numpy(r[k]).cuda() for k in ("text", "lens", "spk")], memory, hn)
    torch.cuda.synchronize()
    memory, hn = memory.cpu().numpy(), hn.cpu().numpy()
    mask = np.arange(T)[None, :] < lens[:, None]
    assert (memory[:, :, enc:] == SENTINEL).all() and (memory[:, :, :enc][~mask] == SENTINEL).all()
    err_out, bound_out = _report("h72 B=6 encoder_outputs", np.where(mask[:, :, None], memory[:, :, :enc], 0.0),
                                 r["r64"]["encoder_outputs"], r["bounds"]["encoder_outputs"])
    err_hn, bound_hn = _report("h72 B=6 hn", hn, r["r64"]["hn"], r["bounds"]["hn"])
    assert err_out <= bound_out and err_hn <= bound_hn, (err_out, bound_out, err_hn, bound_hn)


@pytest.mark.gpu
def test_embedding_gather_beyond_one_block_of_columns(hip_lib_path):
    """``ctts_taco_embed_f32`` at T = 300 (blockIdx.x = 0 and 1 of embed_kernel), B = 2, against a plain gather, bit for bit;
    the halo columns stay zero."""
    from cookietts_amd import _lib
    from cookietts_amd.tacotron2 import PAD, _ld_for
    B, T, E, S, n_sym, n_spk = 2, 300, 48, 16, 179, 7
    rng = np.random.default_rng(300)
    emb = rng.standard_normal((n_sym, E)).astype(np.float32)
    spk_w = rng.standard_normal((n_spk, S)).astype(np.float32)
    text = rng.integers(0, n_sym, size=(B, T))
    text[0, 255], text[0, 256], text[1, T - 1] = n_sym - 1, 0, n_sym - 1
    spk = np.array([6, 2])
    ld = _ld_for(T)
    dev = torch.device("cuda", 0)
    x = torch.zeros(B, E + S, ld, dtype=torch.float32, device=dev)
    ts = [torch.from_numpy(a).to(dev) for a in (emb, spk_w, text.astype(np.int64), spk.astype(np.int64))]
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ctts_taco_embed_f32(*[_lib.ptr(t) for t in ts], _lib.ptr(x), B, T, E, S, ld, PAD, _lib.stream(dev)),
                   "ctts_taco_embed_f32")
        torch.cuda.synchronize()
    x = x.cpu().numpy()
    want = np.concatenate([emb[text].transpose(0, 2, 1), np.repeat(spk_w[spk][:, :, None], T, axis=2)], axis=1)
    assert np.array_equal(x[:, :, PAD:PAD + T], want)
    assert (x[:, :, :PAD] == 0).all() and (x[:, :, PAD + T:] == 0).all()
