"""Split-bf16 (bf16x3) LSTM cell products in the TEACHER-FORCED decoder loop above 64 rows (``set_f32_gemm_mode("bf16x3")`` then
``Decoder.forward`` / ``Tacotron2.forward``: ``ctts_taco_decoder_steps_forced_bf16x3`` over csrc/tacotron_batched_bf16x3.h, the
arithmetic contract of ``ctts_taco_decoder_steps_bf16x3``).

Reference: the fp32 restatement of the teacher-forced loop (tests/tacotron_forced_restatement.py, pinned by the reference's own
``Tacotron2.forward`` goldens), and that restatement with the three cells' products split (``tacotron_bf16x3_restatement.
make_lstm_cell`` in place of ``oracle.tacotron_oracle.lstm_cell`` around the decoder call only).

Bounds.  PARITY_TOL = 5e-6 on mel, alignments, sigmoid(gate) and hidden_att_contexts against the fp32 restatement.  Measured on
the CPU with exactly the inputs below, for the three parity shapes: the restated mode is within mel 2.7e-7, gate 1.6e-7,
alignments 1.9e-8, hidden 7.4e-7 of the fp32 restatement (RESTATED_TOL = 1e-6), the smallest planted fault (``no w_hi x_lo``)
moves the mel by 8.6e-5 and the hidden record by 2.1e-4 (FAULT_FLOOR = 2e-5): the bound lies a factor of 6 above the restated
mode and a factor of 17 below a lost term.  The first test pins both sides at (128, 40, 4), so the GPU bound separates a correct
kernel from one that lost a term (the suite's MEL_TOL = 1e-4 barely could).  Against the reference's goldens the bound is the
suite's MEL_TOL.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from cookietts_amd import _lib, synthetic
from oracle import tacotron_oracle as to
import tacotron_bf16x3_restatement as t3
import tacotron_forced_restatement as fr

PARITY_TOL = 5e-6         # either mode on the GPU against the fp32 restatement
RESTATED_TOL = 1e-6       # the restated mode, every term
FAULT_FLOOR = 2e-5        # the restated mode with a planted fault
MEL_TOL = 1e-4            # BASELINE.json (the reference's goldens)
E_ARG = -1                # CTTS_E_ARG
FAULTS = {"no w_lo x_hi": ("hh", "hl"), "no w_hi x_lo": ("hh", "lh"), "hi hi only": ("hh",)}
NEW_SYMBOL = "ctts_taco_decoder_steps_forced_bf16x3"
PARITY_CASES = [(70, 40, 5), (128, 40, 4), (256, 24, 4)]
NAMES = ("mel", "gate", "alignments", "hidden", "memory")


def split_decoder_forward(*args, terms=t3.TERMS, **kw):
    """``tacotron_forced_restatement.decoder_forward`` with the three cells' products split (``terms``: the products summed)."""
    saved = to.lstm_cell
    to.lstm_cell = t3.make_lstm_cell(terms)
    try:
        return _FP32_DECODER_FORWARD(*args, **kw)
    finally:
        to.lstm_cell = saved


_FP32_DECODER_FORWARD = fr.decoder_forward


def _hp_sd():
    hp = synthetic.tacotron_hparams()
    shapes = json.load(open(os.path.join(GOLDEN, "tacotron_state_shapes.json")))
    return hp, synthetic.tacotron_state_dict(hp, seed=11, shapes=shapes)


@functools.lru_cache(maxsize=None)
def _inputs(B, T, n):
    """(hparams, state dict, memory_in, lengths, masks, gt_mel) of a synthetic case: built once, shared, never modified."""
    hp, sd = _hp_sd()
    lens = [T] + [int(x) for x in np.random.default_rng(B).integers(18, T + 1, size=B - 1)]
    memory_in = (np.random.default_rng(100 + B).standard_normal((B, T, synthetic.tacotron_memory_in_dim(hp))) * 0.5).astype(np.float32)
    lengths = np.asarray(lens, dtype=np.int64)
    masks = synthetic.prenet_dropout_masks(n, B, hp.prenet_dim, seed=100 + B + 1)
    gt_mel = synthetic.synthetic_mel(B, n, hp.n_mel_channels, seed=B)
    for a in (memory_in, lengths, masks, gt_mel):
        a.setflags(write=False)
    return hp, sd, memory_in, lengths, masks, gt_mel


@functools.lru_cache(maxsize=None)
def _case(B, T, n):
    """The inputs and the fp32 restatement's (mel, gate logits, alignments, hidden, memory) on them."""
    hp, sd, memory_in, lengths, masks, gt_mel = _inputs(B, T, n)
    ref = fr.decoder_forward(sd, hp, memory_in, gt_mel, lengths, masks)
    for a in ref:
        a.setflags(write=False)
    return hp, sd, memory_in, lengths, masks, gt_mel, ref


def _sig(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def _errors(out, ref):
    """L_inf of (mel, sigmoid(gate), alignments, hidden) against the fp32 restatement."""
    o = [np.asarray(x.cpu().numpy() if torch.is_tensor(x) else x) for x in out[:4]]
    return (float(np.abs(o[0] - ref[0]).max()), float(np.abs(_sig(o[1]) - _sig(ref[1])).max()),
            float(np.abs(o[2] - ref[2]).max()), float(np.abs(o[3] - ref[3]).max()))


@functools.lru_cache(maxsize=None)
def _default_fields():
    from cookietts_amd import Tacotron2
    c = Tacotron2(synthetic.tacotron_hparams()).decoder.c_config()
    return tuple((f, getattr(c, f)) for f, _ in c._fields_)


def _cfg(**edits):
    """The default decoder shape's config struct with some fields replaced."""
    return _lib.TacoDecoderConfig(**dict(_default_fields(), **edits))


# --------------------------------------------------------------------------- without a GPU ----
def test_restated_forced_loop_is_fp32_grade_and_a_lost_term_is_not():
    """(B, T, n) = (128, 40, 4): the restated teacher-forced bf16x3 loop sits within RESTATED_TOL of the fp32 restatement on mel,
    gate logits, alignments and hidden_att_contexts (measured 2.7e-7 / 1.6e-7 / 1.9e-8 / 7.4e-7 at most over the three parity
    shapes); every planted fault is at least FAULT_FLOOR away on the mel (smallest: ``no w_hi x_lo``, 8.6e-5)."""
    hp, sd, memory_in, lengths, masks, gt_mel, ref = _case(128, 40, 4)
    full = split_decoder_forward(sd, hp, memory_in, gt_mel, lengths, masks)
    e = [float(np.abs(a - b).max()) for a, b in zip(full[:4], ref[:4])]
    print("restated forced bf16x3 vs fp32 restatement, L_inf: " + "; ".join(f"{k} {v:.2e}" for k, v in zip(NAMES, e)))
    assert max(e) <= RESTATED_TOL
    assert RESTATED_TOL < PARITY_TOL < FAULT_FLOOR
    assert np.array_equal(full[4], ref[4])                  # the bottlenecked memory is no cell's business
    for name, terms in FAULTS.items():
        bad = split_decoder_forward(sd, hp, memory_in, gt_mel, lengths, masks, terms=terms)
        f = float(np.abs(bad[0] - ref[0]).max())
        print(f"planted fault '{name}': mel L_inf {f:.2e}, hidden L_inf {np.abs(bad[3] - ref[3]).max():.2e}")
        assert f >= FAULT_FLOOR, name


def test_restated_forced_loop_matches_the_reference_golden(monkeypatch):
    """Golden ``tacotron_forced_default`` (3 rows, 37 frames, the reference's own Tacotron2.forward): the teacher-forced pass with
    the DECODER's cells split (the encoder's LSTM stays fp32) stays within MEL_TOL on pred_mel, pred_mel_postnet, alignments,
    hidden_att_contexts and sigmoid(gate) (measured <= 9.1e-7 on all five); ``hi hi only`` leaves it on both mels (1.7e-4 /
    2.5e-4)."""
    g = fr.load_golden("default")
    hp = synthetic.tacotron_hparams()
    shapes = json.load(open(os.path.join(GOLDEN, "tacotron_state_shapes.json")))
    sd = synthetic.tacotron_state_dict(hp, seed=int(g["seed"]), shapes=shapes)
    assert g["gt_mel"].shape == (3, 80, 37)
    keys = ("pred_mel", "pred_mel_postnet", "alignments", "hidden_att_contexts")

    def run(terms):              # tacotron_forward looks decoder_forward up in its module: split cells around the decoder call only
        monkeypatch.setattr(fr, "decoder_forward", functools.partial(split_decoder_forward, terms=terms))
        return fr.tacotron_forward(sd, hp, g["gt_mel"], g["text"], g["lengths"], g["speakers"], g["gt_sylps"], g["torchmoji"], g["masks"])
    out = run(t3.TERMS)
    e = {k: float(np.abs(out[k] - g[k]).max()) for k in keys}
    e["sigmoid(gate)"] = float(np.abs(_sig(out["pred_gate_logits"]) - _sig(g["pred_gate_logits"])).max())
    print("restated forced bf16x3 vs the reference's forward: " + "; ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) < MEL_TOL
    bad = run(("hh",))
    f = [float(np.abs(bad[k] - g[k]).max()) for k in ("pred_mel", "pred_mel_postnet")]
    print(f"'hi hi only' vs the reference's forward: pred_mel {f[0]:.2e}, pred_mel_postnet {f[1]:.2e}")
    assert min(f) > MEL_TOL


def test_forced_bf16x3_symbol_and_refusals_without_gpu(hip_lib_path):
    """Exported, declared, typed; ABI 7; the bf16x3 refusals with every pointer NULL; then the fp32 teacher-forced entry's argument
    checks, before any launch (made-up, aligned, never dereferenced addresses)."""
    lib = _lib.lib()
    header = open(os.path.join(REPO, "include", "cookietts_hip.h")).read()
    assert (NEW_SYMBOL + "(") in header and NEW_SYMBOL in _lib.SIGNATURES and getattr(lib, NEW_SYMBOL) is not None
    assert _lib.SIGNATURES[NEW_SYMBOL] == _lib.SIGNATURES["ctts_taco_decoder_steps_forced_f32"]
    assert "#define CTTS_ABI_VERSION 7" in header and lib.ctts_abi_version() == 7
    fn = getattr(lib, NEW_SYMBOL)
    nulls = (None, None, None, None, 70, 40, 0, 1, 1, None, 0, None)
    odd = _cfg(window_range=20)
    assert lib.ctts_taco_decoder_max_batch(C.byref(odd)) == 4
    assert fn(C.byref(odd), *nulls) == E_ARG and b"no batched form" in lib.ctts_last_error()
    p240 = _cfg(prenet_dim=240)
    assert fn(C.byref(p240), *nulls) == E_ARG
    assert b"prenet_dim" in lib.ctts_last_error() and b"32" in lib.ctts_last_error()
    cfg = _cfg()
    assert lib.ctts_taco_decoder_max_batch(C.byref(cfg)) == 256
    pk, pre, al, hid, ws = (C.c_void_p(4096 * i) for i in range(1, 6))
    T, TXT = 7, 40
    for B in (5, 70):                                  # the fp32 schedules' rows and the split cells' rows
        need = lib.ctts_taco_decoder_workspace_bytes(C.byref(cfg), B, TXT)
        assert need > 0
        good = [pk, pre, al, hid, B, TXT, 0, T, T, ws, need, None]
        for i in (0, 1, 2, 3, 9):
            a = list(good); a[i] = None
            assert fn(C.byref(cfg), *a) == E_ARG and b"NULL pointer" in lib.ctts_last_error(), (B, i)
        for edit, msg in (({4: 0}, b"batch=0"), ({4: 257}, b"batch=257"), ({6: 3, 7: 5}, b"step0=3 n_steps=5 max_steps=7"),
                          ({6: -1}, b"step0=-1"), ({7: -1}, b"n_steps=-1"), ({5: 0}, b"text_len=0"),
                          ({10: need - 4}, b"bytes < required")):
            a = list(good)
            for i, v in edit.items():
                a[i] = v
            assert fn(C.byref(cfg), *a) == E_ARG and msg in lib.ctts_last_error(), (B, msg, lib.ctts_last_error())


# --------------------------------------------------------------------------------- on the GPU ----
_MODEL = {}


def _model():
    """One model on the GPU for the synthetic cases of the file (seed 11); every test sets the mode it wants."""
    if "m" not in _MODEL:
        from cookietts_amd import Tacotron2
        hp, sd = _hp_sd()
        m = Tacotron2(hp)
        m.load_state_dict(synthetic.to_torch(sd))
        _MODEL["m"] = m.cuda().eval()
    return _MODEL["m"]


def _run(m, mode, case, rows=None):
    """Decoder.forward(..., return_hidden_state=True) on the first ``rows`` rows of a case: (mel, gate logits, alignments, hidden,
    memory)."""
    hp, sd, memory_in, lengths, masks, gt_mel = case[:6]
    m.set_f32_gemm_mode(mode)
    rows = rows or len(lengths)
    return m.decoder(torch.tensor(memory_in[:rows]).cuda(), torch.tensor(gt_mel[:rows]).cuda(), torch.tensor(lengths[:rows]).cuda(),
                     keep_masks=np.ascontiguousarray(masks[:, :, :rows]), return_hidden_state=True)


def _equal(a, b, rows=None):
    return all(torch.equal(x[:rows] if rows else x, y) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,n", PARITY_CASES)
def test_forced_bf16x3_matches_the_fp32_restatement(hip_lib_path, B, T, n):
    """70 rows (padded to 128; ragged lengths incl. texts shorter than the 33-token window), 128 and 256 rows: both modes within
    PARITY_TOL of the fp32 restatement on mel, sigmoid(gate), alignments and hidden, and the mode's mel is NOT the fp32 mode's
    bits - the split cells ran in ``forward``.  Measured on an MI355X: bf16x3 mel 2.6e-7 / 2.7e-7 / 2.8e-7, hidden <= 7.7e-7;
    fp32 mode mel <= 1.0e-7, hidden <= 2.8e-7."""
    case = _case(B, T, n)
    ref = case[6]
    if B == 70:
        assert case[3].min() < 2 * case[0].windowed_attention_range + 1
    m = _model()
    out = _run(m, "bf16x3", case)
    assert len(next(iter(m.decoder._ws.values()))) == 1      # one group, one workspace
    e = _errors(out, ref)
    print(f"forced bf16x3 B={B}: L_inf mel {e[0]:.2e} sigmoid(gate) {e[1]:.2e} alignments {e[2]:.2e} hidden {e[3]:.2e}")
    f32 = _run(m, "f32", case)
    e32 = _errors(f32, ref)
    print(f"forced fp32   B={B}: L_inf mel {e32[0]:.2e} sigmoid(gate) {e32[1]:.2e} alignments {e32[2]:.2e} hidden {e32[3]:.2e}")
    assert out[0].shape == (B, 80, n) and out[3].shape == ref[3].shape
    assert max(e) <= PARITY_TOL
    assert max(e32) <= PARITY_TOL
    assert not torch.equal(out[0], f32[0])
    assert torch.equal(out[4], f32[4])                       # the bottlenecked memory: init is fp32 in both


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [16, 64])
def test_forced_bf16x3_is_inert_at_or_below_64_rows(hip_lib_path, rows):
    case = _case(70, 40, 5)
    m = _model()
    on = _run(m, "bf16x3", case, rows=rows)
    off = _run(m, "f32", case, rows=rows)
    assert len(on) == 5 and _equal(on, off)


@pytest.mark.gpu
def test_forced_bf16x3_blocks_rows_and_repeats(hip_lib_path):
    """70 rows, 21 steps.  Blocks of 8 / 8 / 5 steps (step0 > 0: the attention RNN of a block's first step runs in a launch of
    its own, every other one as a role of the two-cell launch; a block's last second decoder RNN runs alone) equal one block of
    21 bit for bit - a cell's bits are the same alone and as a role.  A repeated call is bit-equal.  The first 70 rows of a
    71-row call and of the 256-row case equal the 70-row call bit for bit."""
    m = _model()
    case = _inputs(70, 40, 21)
    one = _run(m, "bf16x3", case)
    assert all(bool(torch.isfinite(x).all()) for x in one) and one[0].shape == (70, 80, 21)
    assert _equal(one, _run(m, "bf16x3", case))
    m.decoder.forced_chunk = 8
    try:
        blocks = _run(m, "bf16x3", case)
    finally:
        m.decoder.forced_chunk = None
    assert _equal(one, blocks)
    assert not torch.equal(one[0], _run(m, "f32", case)[0])
    c128 = _inputs(128, 40, 4)
    assert _equal(_run(m, "bf16x3", c128, rows=71), _run(m, "bf16x3", c128, rows=70), rows=70)
    c256 = _inputs(256, 24, 4)
    assert _equal(_run(m, "bf16x3", c256), _run(m, "bf16x3", c256, rows=70), rows=70)


@pytest.mark.gpu
def test_fp32_forced_entry_point_on_the_bf16x3_blob_gives_the_fp32_bits(hip_lib_path, monkeypatch):
    """The bf16x3 blob is the fp32 blob followed by the planes: ctts_taco_decoder_steps_forced_f32 on it, at 70 rows, gives what
    it gives on the fp32 blob bit for bit (init, prenet frames and projection run on it in both)."""
    case = _inputs(70, 40, 5)
    m = _model()
    f32 = _run(m, "f32", case)
    lib = _lib.lib()
    calls = []

    def forced_f32(cfg, blob, prenet_all, align, hidden, batch, *rest):
        calls.append(batch)
        return lib.ctts_taco_decoder_steps_forced_f32(cfg, blob, prenet_all, align, hidden, batch, *rest)
    m.set_f32_gemm_mode("bf16x3")
    monkeypatch.setattr(lib, NEW_SYMBOL, forced_f32)
    out = _run(m, "bf16x3", case)
    c = m.decoder.c_config()
    assert m.decoder._packed[2].numel() * 4 == lib.ctts_taco_decoder_packed_bf16x3_bytes(C.byref(c)) and calls == [70]
    assert _equal(out, f32)


@pytest.mark.gpu
def test_forced_bf16x3_72_rows_match_the_reference_golden(hip_lib_path):
    """Golden ``default`` 24 times over = 72 rows in one call (lengths sorted as pack_padded_sequence wants, masks tiled and
    reordered alike), Tacotron2.forward in mode "bf16x3": every copy matches the reference's nine-key dict within MEL_TOL on the
    keys test_tacotron_forced._compare asserts."""
    from test_tacotron_forced import _case as _golden, _compare, _forward, _model as _golden_model
    g, hp, sd = _golden("default")
    m = _golden_model("default")
    rep = lambda a: np.concatenate([a] * 24, axis=0)                       # noqa: E731
    order = np.argsort(-rep(g["lengths"]), kind="stable")
    g72 = {k: (v if np.ndim(v) == 0 else np.ascontiguousarray(np.concatenate([v] * 24, axis=2)[:, :, order]) if k == "masks"
               else np.ascontiguousarray(rep(v)[order])) for k, v in g.items()}
    assert g72["gt_mel"].shape == (72, 80, 37) and (np.diff(g72["lengths"]) <= 0).all()
    m.set_f32_gemm_mode("bf16x3")
    try:
        out = _forward(m, g72, return_hidden_state=True)
        assert len(next(iter(m.decoder._ws.values()))) == 1
    finally:
        m.set_f32_gemm_mode(None)                                          # the model is shared with test_tacotron_forced.py
    _compare(out, g72, "hip bf16x3 72 rows")
    src = order % 3
    for k in ("pred_mel", "alignments", "hidden_att_contexts"):             # every copy, not only the worst one
        assert np.abs(out[k] - g[k][src]).reshape(72, -1).max(axis=1).max() < MEL_TOL, k
