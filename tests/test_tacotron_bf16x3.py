"""Split-bf16 (bf16x3) LSTM cell products of the Tacotron2 decoder above 64 rows (``set_f32_gemm_mode("bf16x3")`` over
csrc/tacotron_batched_bf16x3.h; the arithmetic is listed at ``ctts_taco_decoder_steps_bf16x3``).

Bounds.  GPU parity: L_inf of mel, alignments and sigmoid(gate) against the fp32 oracle <= PARITY_TOL = 5e-6 - 50 x what the fp32
GPU path (profiles/r6_final_pytest_gpu.log: <= 1.0e-7) and the restated mode (tests/tacotron_bf16x3_restatement.py: 1.1e-7 at
(128, 40, 4)) leave, and 5 x below the smallest planted fault: a dropped cross term is 2.6e-5 / 5.2e-5, hi * hi alone 6.1e-5.  The
first test pins both sides of that on the CPU, so the GPU bound separates a correct kernel from one that lost a term (the suite's
MEL_TOL = 1e-4 cannot see one).  The stop-rule golden keeps the suite's 1e-4 against the reference's postnet mel.
"""
import ctypes
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

PARITY_TOL = 5e-6         # mode on against the fp32 oracle
RESTATED_TOL = 1e-6       # the restatement, every term
FAULT_FLOOR = 2e-5        # the restatement with a planted fault
MEL_TOL = 1e-4            # BASELINE.json (the stop-rule golden)
E_ARG = -1                # CTTS_E_ARG
FAULTS = {"no w_lo x_hi": ("hh", "hl"), "no w_hi x_lo": ("hh", "lh"), "hi hi only": ("hh",)}
NEW_SYMBOLS = ("ctts_taco_decoder_packed_bf16x3_bytes", "ctts_taco_decoder_pack_bf16x3", "ctts_taco_decoder_steps_bf16x3")
PARITY_CASES = [(70, 40, 5), (128, 40, 4), (256, 24, 4)]


def _hp_sd():
    hp = synthetic.tacotron_hparams()
    shapes = json.load(open(os.path.join(GOLDEN, "tacotron_state_shapes.json")))
    return hp, synthetic.tacotron_state_dict(hp, seed=11, shapes=shapes)


@functools.lru_cache(maxsize=None)
def _case(B, T, n):
    """Model and inputs exactly as tests/test_tacotron_batched.py::test_batched_decoder_matches_oracle builds them, and the fp32
    oracle's outputs: computed once, shared, never modified."""
    hp, sd = _hp_sd()
    rng = np.random.default_rng(B)
    lens = [T] + [int(x) for x in rng.integers(18, T + 1, size=B - 1)]
    rng = np.random.default_rng(100 + B)
    memory_in = (rng.standard_normal((B, T, synthetic.tacotron_memory_in_dim(hp))) * 0.5).astype(np.float32)
    lengths = np.asarray(lens, dtype=np.int64)
    masks = synthetic.prenet_dropout_masks(n, B, hp.prenet_dim, seed=100 + B + 1)
    ref = to.decoder_inference_steps(sd, hp, memory_in, lengths, masks, n)
    for a in (memory_in, lengths, masks) + tuple(ref):
        a.setflags(write=False)
    return hp, sd, memory_in, lengths, masks, ref


_MODEL = {}


def _model():
    """One decoder model on the GPU for the whole file (seed 11); every test sets the mode it wants."""
    if "m" not in _MODEL:
        from cookietts_amd import Tacotron2
        hp, sd = _hp_sd()
        m = Tacotron2(hp)
        m.load_state_dict(synthetic.to_torch(sd))
        _MODEL["m"] = m.cuda().eval()
    return _MODEL["m"]


def _run(m, mode, memory_in, lengths, masks, n, rows=None, **kw):
    m.set_f32_gemm_mode(mode)
    rows = rows or len(lengths)
    return m.decoder.inference(torch.tensor(memory_in[:rows]).cuda(), torch.tensor(lengths[:rows]).cuda(),
                               keep_masks=np.ascontiguousarray(masks[:, :, :rows]), fixed_steps=n, **kw)


def _errors(out, ref):
    mel, gate, align = out[:3]
    ref_mel, ref_gate, ref_align = ref
    return (float(np.abs(mel.cpu().numpy() - ref_mel).max()), float(np.abs(align.cpu().numpy() - ref_align).max()),
            float(np.abs(gate.cpu().numpy() - 1 / (1 + np.exp(-ref_gate))).max()))


@functools.lru_cache(maxsize=None)
def _default_fields():
    from cookietts_amd import Tacotron2
    c = Tacotron2(synthetic.tacotron_hparams()).decoder.c_config()
    return tuple((f, getattr(c, f)) for f, _ in c._fields_)


def _cfg(**edits):
    """The default decoder shape's config struct with some fields replaced."""
    return _lib.TacoDecoderConfig(**dict(_default_fields(), **edits))


def _small_decoder():
    from cookietts_amd import Tacotron2
    return Tacotron2(synthetic.tacotron_hparams(**synthetic.TACOTRON_SMALL_OVERRIDES)).decoder


# --------------------------------------------------------------------------- without a GPU ----
def test_restatement_is_fp32_grade_and_a_lost_term_is_not():
    """(B, T, n) = (128, 40, 4): the restated mode sits within 1e-6 of the fp32 oracle (measured 1.1e-7); each planted fault is at
    least 2e-5 away (measured 2.6e-5, 5.2e-5, 6.1e-5): PARITY_TOL lies a factor 4 and more from both."""
    hp, sd, memory_in, lengths, masks, ref = _case(128, 40, 4)
    full = t3.decoder_inference_steps(sd, hp, memory_in, lengths, masks, 4)
    e = np.abs(full[0] - ref[0]).max()
    print(f"restated bf16x3 vs fp32 oracle, mel L_inf {e:.2e}; gate {np.abs(full[1] - ref[1]).max():.2e}; "
          f"alignments {np.abs(full[2] - ref[2]).max():.2e}")
    assert e <= RESTATED_TOL
    assert RESTATED_TOL < PARITY_TOL < FAULT_FLOOR
    for name, terms in FAULTS.items():
        bad = t3.decoder_inference_steps(sd, hp, memory_in, lengths, masks, 4, terms=terms)
        f = np.abs(bad[0] - ref[0]).max()
        print(f"planted fault '{name}': mel L_inf {f:.2e}")
        assert f >= FAULT_FLOOR, name


def test_gemm_mode_host_surface_on_a_cpu_model(hip_lib_path):
    from cookietts_amd import Tacotron2
    m = Tacotron2(synthetic.tacotron_hparams()).eval()
    dec = m.decoder
    assert dec.f32_gemm_mode is None and m.f32_gemm_mode is None
    for name in (None, "default", "f32"):
        assert dec.set_f32_gemm_mode(name) is dec and not dec._bf16x3
    assert dec.set_f32_gemm_mode("bf16x3") is dec and dec._bf16x3 and dec.f32_gemm_mode == "bf16x3"
    with pytest.raises(NotImplementedError, match="bf16x6"):
        dec.set_f32_gemm_mode("bf16x6")
    with pytest.raises(ValueError):
        dec.set_f32_gemm_mode("tf32")
    assert dec._bf16x3                                       # a refused name changes nothing
    # Tacotron2 forwards to its decoder and returns itself
    assert m.set_f32_gemm_mode("f32") is m and not dec._bf16x3 and m.f32_gemm_mode == "f32"
    assert m.set_f32_gemm_mode("bf16x3") is m and dec._bf16x3
    # the packed blob is dropped when the mode changes and kept when it does not
    sentinel = ("device", "key", "blob")
    dec._packed = sentinel
    m.set_f32_gemm_mode("bf16x3")
    assert dec._packed is sentinel
    m.set_f32_gemm_mode("f32")
    assert dec._packed is None
    dec._packed = sentinel
    for name in (None, "default", "f32"):
        m.set_f32_gemm_mode(name)
        assert dec._packed is sentinel
    dec.set_f32_gemm_mode("bf16x3")
    assert dec._packed is None
    # a shape the library refuses: here, not at the first call
    odd = Tacotron2(synthetic.tacotron_hparams(prenet_dim=200)).decoder
    with pytest.raises(NotImplementedError, match="prenet_dim"):
        odd.set_f32_gemm_mode("bf16x3")
    assert odd.set_f32_gemm_mode("f32") is odd


def _plane_bytes(c):
    """The documented size of the split planes (include/cookietts_hip.h): a hi | lo pair per weight of the three cells."""
    P, Dm, Ra, Rd, Rd2 = c.prenet_dim, c.memory_dim, c.attention_rnn_dim, c.decoder_rnn_dim, c.second_decoder_rnn_dim
    return 4 * (4 * Ra * (P + Dm + Rd + Ra) + 4 * Rd * (Ra + Dm + Rd) + 4 * Rd2 * (Rd + Rd2))


def test_bf16x3_size_query_symbols_and_refusals_without_gpu(hip_lib_path):
    header = open(os.path.join(REPO, "include", "cookietts_hip.h")).read()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert (name + "(") in header and name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert "#define CTTS_ABI_VERSION 7" in header and lib.ctts_abi_version() == 7
    default = _cfg()
    assert _plane_bytes(default) == 4 * (5120 * 2816 + 3072 * 2560 + 3072 * 1536) == 108_003_328      # "+ 108 MB at the default shape"
    for c in (default, _small_decoder().c_config()):
        assert lib.ctts_taco_decoder_max_batch(ctypes.byref(c)) == 256
        p32 = lib.ctts_taco_decoder_packed_bytes(ctypes.byref(c))
        assert p32 > 0 and lib.ctts_taco_decoder_packed_bf16x3_bytes(ctypes.byref(c)) == p32 + _plane_bytes(c)
    # a shape without the batched form: 0 and a message, CTTS_E_ARG from the others before anything is touched (NULL pointers)
    odd = _cfg(window_range=20)
    assert lib.ctts_taco_decoder_max_batch(ctypes.byref(odd)) == 4 and lib.ctts_taco_decoder_packed_bytes(ctypes.byref(odd)) > 0
    assert lib.ctts_taco_decoder_packed_bf16x3_bytes(ctypes.byref(odd)) == 0
    assert b"no batched form" in lib.ctts_last_error()
    assert lib.ctts_taco_decoder_pack_bf16x3(ctypes.byref(odd), None, None, None) == E_ARG
    assert b"no batched form" in lib.ctts_last_error()
    assert lib.ctts_taco_decoder_steps_bf16x3(ctypes.byref(odd), None, None, None, None, None, None, 70, 40, 0, 1, 1, None,
                                              None) == E_ARG
    assert b"no batched form" in lib.ctts_last_error()


def test_a_k_piece_that_is_no_multiple_of_32_is_refused_by_name(hip_lib_path):
    """The planes' chunk is 32 K columns: a cell's X piece (prenet | context | hidden states) that is not a multiple of 32 wide is
    refused with CTTS_E_ARG and the field's name before anything is launched or read (every pointer is NULL here).  Such a shape
    has no batched form either (every K of it is a multiple of 64, which leaves no piece that is not a multiple of 32: swept
    below), so the refusal never takes a shape away from a caller of the fp32 entry points."""
    lib = _lib.lib()
    for field, value in (("prenet_dim", 240), ("memory_dim", 496), ("decoder_rnn_dim", 784), ("attention_rnn_dim", 1296)):
        c = _cfg(**{field: value}, **({"second_decoder_rnn_dim": value} if field == "decoder_rnn_dim" else {}))
        assert value % 16 == 0 and value % 32 != 0 and lib.ctts_taco_decoder_packed_bytes(ctypes.byref(c)) > 0, field
        assert lib.ctts_taco_decoder_packed_bf16x3_bytes(ctypes.byref(c)) == 0
        assert field.encode() in lib.ctts_last_error(), lib.ctts_last_error()
        assert lib.ctts_taco_decoder_pack_bf16x3(ctypes.byref(c), None, None, None) == E_ARG
        assert field.encode() in lib.ctts_last_error()
        assert lib.ctts_taco_decoder_steps_bf16x3(ctypes.byref(c), None, None, None, None, None, None, 70, 40, 0, 1, 1, None,
                                                  None) == E_ARG
        assert field.encode() in lib.ctts_last_error() and b"32" in lib.ctts_last_error()
    # every shape with the batched form is taken: widths in steps of 16 around the default shape
    taken = 0
    for P in (224, 240, 256):
        for Dm in (480, 496, 512):
            for Rd in (736, 752, 768):
                for Ra in (1248, 1264, 1280):
                    c = _cfg(prenet_dim=P, memory_dim=Dm, decoder_rnn_dim=Rd, second_decoder_rnn_dim=Rd, attention_rnn_dim=Ra)
                    batched = lib.ctts_taco_decoder_max_batch(ctypes.byref(c)) == 256
                    assert (lib.ctts_taco_decoder_packed_bf16x3_bytes(ctypes.byref(c)) > 0) == batched, (P, Dm, Rd, Ra)
                    taken += batched
    assert taken >= 2


# --------------------------------------------------------------------------------- on the GPU ----
@pytest.mark.gpu
@pytest.mark.parametrize("B,T,n", PARITY_CASES)
def test_bf16x3_decoder_matches_the_fp32_oracle(hip_lib_path, B, T, n):
    """70 rows (padded to 128, ragged lengths incl. texts shorter than the window), 128 and 256 rows: within PARITY_TOL of the
    fp32 oracle, and not the fp32 mode's bits - the split cells ran."""
    hp, sd, memory_in, lengths, masks, ref = _case(B, T, n)
    m = _model()
    out = _run(m, "bf16x3", memory_in, lengths, masks, n)
    assert len(next(iter(m.decoder._ws.values()))) == 1      # one workspace, the per-launch form
    e = _errors(out, ref)
    print(f"bf16x3 B={B}: L_inf mel {e[0]:.2e} alignments {e[1]:.2e} gate {e[2]:.2e}")
    assert max(e) <= PARITY_TOL
    f32 = _run(m, "f32", memory_in, lengths, masks, n)
    assert max(_errors(f32, ref)) <= PARITY_TOL
    assert not torch.equal(out[0], f32[0])


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [16, 64])
def test_bf16x3_is_inert_at_or_below_64_rows(hip_lib_path, rows):
    hp, sd, memory_in, lengths, masks, ref = _case(70, 40, 5)
    m = _model()
    on = _run(m, "bf16x3", memory_in, lengths, masks, 5, rows=rows, return_hidden_state=True)
    off = _run(m, "f32", memory_in, lengths, masks, 5, rows=rows, return_hidden_state=True)
    assert all(torch.equal(a, b) for a, b in zip(on, off))


@pytest.mark.gpu
def test_fp32_entry_point_on_the_bf16x3_blob_gives_the_fp32_bits(hip_lib_path, monkeypatch):
    """The bf16x3 blob is the fp32 blob followed by the planes: ctts_taco_decoder_steps_f32 on it, at 70 rows, gives what it gives
    on the fp32 blob bit for bit (init runs on it in both)."""
    hp, sd, memory_in, lengths, masks, ref = _case(70, 40, 5)
    m = _model()
    f32 = _run(m, "f32", memory_in, lengths, masks, 5)
    lib = _lib.lib()
    calls = []

    def steps_f32(cfg, blob, km, mel, gate, align, hidden, *rest):
        assert hidden is None
        calls.append(rest[0])
        return lib.ctts_taco_decoder_steps_f32(cfg, blob, km, mel, gate, align, *rest)
    m.set_f32_gemm_mode("bf16x3")
    monkeypatch.setattr(lib, "ctts_taco_decoder_steps_bf16x3", steps_f32)
    out = _run(m, "bf16x3", memory_in, lengths, masks, 5)
    c = m.decoder.c_config()
    assert m.decoder._packed[2].numel() * 4 == lib.ctts_taco_decoder_packed_bf16x3_bytes(ctypes.byref(c)) and calls == [70]
    assert all(torch.equal(a, b) for a, b in zip(out[:3], f32[:3]))


@pytest.mark.gpu
def test_bf16x3_rows_do_not_depend_on_the_rest_of_the_batch(hip_lib_path):
    hp, sd, memory_in, lengths, masks, ref = _case(128, 40, 4)
    m = _model()
    full = _run(m, "bf16x3", memory_in, lengths, masks, 4, rows=71)
    part = _run(m, "bf16x3", memory_in, lengths, masks, 4, rows=70)
    assert all(torch.equal(a[:70], b) for a, b in zip(full[:3], part[:3]))
    # ... nor on the padded row count: the same 70 rows inside a 256-row call
    hp, sd, mem256, len256, masks256, _ = _case(256, 24, 4)
    whole = _run(m, "bf16x3", mem256, len256, masks256, 4)
    head = _run(m, "bf16x3", mem256, len256, masks256, 4, rows=70)
    assert all(torch.equal(a[:70], b) for a, b in zip(whole[:3], head[:3]))


@pytest.mark.gpu
def test_bf16x3_is_bit_identical_run_to_run(hip_lib_path):
    hp, sd = _hp_sd()
    B, T, n = 128, 40, 30
    rng = np.random.default_rng(128)
    lengths = np.asarray([T] + [int(x) for x in rng.integers(18, T + 1, size=B - 1)], dtype=np.int64)
    memory_in = (np.random.default_rng(1280).standard_normal((B, T, synthetic.tacotron_memory_in_dim(hp))) * 0.5).astype(np.float32)
    masks = synthetic.prenet_dropout_masks(n, B, hp.prenet_dim, seed=1281)
    m = _model()
    first = _run(m, "bf16x3", memory_in, lengths, masks, n)
    assert torch.isfinite(first[0]).all()
    for _ in range(2):
        again = _run(m, "bf16x3", memory_in, lengths, masks, n)
        assert all(torch.equal(a, b) for a, b in zip(first[:3], again[:3]))


@pytest.mark.gpu
def test_bf16x3_hidden_states_match_the_fp32_mode(hip_lib_path):
    hp, sd, memory_in, lengths, masks, ref = _case(70, 40, 5)
    m = _model()
    on = _run(m, "bf16x3", memory_in, lengths, masks, 5, return_hidden_state=True)
    off = _run(m, "f32", memory_in, lengths, masks, 5, return_hidden_state=True)
    assert on[3].shape == (70, hp.second_decoder_rnn_dim + hp.memory_bottleneck_dim, 5)
    d = float((on[3] - off[3]).abs().max())
    print(f"hidden_att_contexts, bf16x3 vs fp32 mode at 70 rows: L_inf {d:.2e}")
    assert 0 < d <= PARITY_TOL


@pytest.mark.gpu
def test_bf16x3_128_rows_stop_where_the_reference_stops_its_four(hip_lib_path):
    """The stop-rule golden's four utterances 32 times over = 128 rows in one call, stop rule live: T_mel is the golden's and every
    copy's postnet mel is the reference's within the suite's 1e-4 (no crossing lies within 0.2 of the threshold)."""
    from test_tacotron_stop import _load, _model as _stop_model
    g, hp, sd, masks, cases = _load()
    m = _stop_model(sd, hp).set_f32_gemm_mode("bf16x3")
    rep = lambda a: np.concatenate([a] * 32, axis=0)                       # noqa: E731
    order = np.argsort(-rep(g["lengths"]), kind="stable")                  # pack_padded_sequence wants the lengths sorted
    args = [torch.from_numpy(rep(g[k])[order]).cuda() for k in ("text", "lengths", "speakers", "torchmoji")]
    masks128 = np.ascontiguousarray(np.concatenate([masks] * 32, axis=2)[:, :, order])
    src = order % 4
    for name in ("delay0", "cap_in_delay"):
        thr, delay, cap, T = cases[name]
        m.decoder.gate_delay, m.decoder.max_decoder_steps, m.decoder.gate_threshold = int(delay), int(cap), float(thr)
        out = m.inference(*args, keep_masks=masks128)
        assert len(next(iter(m.decoder._ws.values()))) == 1
        o = out["pred_mel_postnet"].cpu().numpy()
        assert o.shape == (128, 80, T), (name, o.shape, T)
        e = np.abs(o - g[f"{name}_pred_mel_postnet"][src]).max()
        print(f"128 rows / {name}: T_mel {T}, postnet mel L_inf vs the reference's four {e:.2e}")
        assert e < MEL_TOL
