"""The small kernels the ax / WaveFlow conditioning path is assembled from, each called directly through the C ABI on padded
buffers and compared with numpy: ``ctts_embed_rows_f32``, ``ctts_pad_rows_f32`` / ``ctts_unpad_rows_f32``,
``ctts_interleave_phases_f32``, ``ctts_replicate_halo_f32``, ``ctts_resample_rows_f32`` (all three modes),
``ctts_scale_add_rows_f32``, ``ctts_affine_rows_f32``, ``ctts_vol_unscale_f32``, ``ctts_deemphasis_f32`` and
``ctts_fold_weightnorm_f32`` (which feeds every packer of the project).

Every case: batch 3, a row count that is no multiple of 16, ``ld > pad + T`` with the model's halo ``PAD``; the destination (and
64 guard floats either side of every device buffer) is pre-filled with a sentinel and everything the entry does not own - halo
columns, rows above ``C`` / ``rows``, spare rows of other items, the guards - must still hold its bits.  T in {1, 255, 256, 257}:
one thread, a ragged block, a full block, one element in a second block.

Three kinds of bound, none of them tuned to the code under test:
  * movers (embed, pad / unpad, interleave, replicate halo, 'nearest' resampling): bit-equal to numpy indexing;
  * one or two roundings (scale_add, affine, the two linear resampling modes): derived per element from the fp32 format - see
    each test; the interpolation positions are ATen's fp32 ones (tests/ax_cond_f64_restatement.py, pinned to torch there);
    de-emphasis carries fp64 state and rounds once: ``2^-24 |y64| + 1e-12 max|y64|``;
  * device ``powf`` / ``log2f`` / ``sqrtf`` and a four-wave sum (vol_unscale, fold_weightnorm): ``FACTOR`` x the error of the numpy
    fp32 restatement on the inputs of that launch (for fold_weightnorm per row, with the floor ``4 * 2^-23 * max|w64|``:
    ``_bound`` of test_tacotron_text_side.py).  The special values of vol_unscale launched ONE at a time are not held to their own
    e32 (one rounding against one rounding) but to a derived bound - see test_vol_unscale_single_special_values.

Every arithmetic comparison prints and appends (case, HIP L-inf, e32, ratio, bound) to profiles/r21_02_ax_cond_glue_parity.jsonl.

Measured on the MI355X (the 96 records of the jsonl): vol_unscale's relative error is 1.97 x that of the numpy fp32 restatement on
the 257-element vector and 1.0 x on the n = 1 launch held to its own e32; fold_weightnorm's row error is 1.0 ... 1.26 x e32
(fan = 255, five rows), so FACTOR stays 8 (4 x 1.97 rounded up to a power of two).  The special values launched singly sit at
0 ... 0.28 of their derived bound; against the single element's OWN e32 the ratio is 1.0 at +-2^-20 and 11.1 at +-3.7 (HIP
1.81e-7, numpy 1.63e-8: one lucky rounding of log2f(3.7) on the host, both far inside 2^-23 (1 + ln 10 |log2 3.7|) = 6.4e-7) -
which is why those launches are not held to it.  The derived bounds hold with room: scale_add, affine and de-emphasis return
the bits of the numpy fp32 evaluation (ratio 1.0), the linear resampling modes sit at 0.57 ... 1.0 x it.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import ax_cond_f64_restatement as acr
from conftest import REPO
from cookietts_amd import _lib
from cookietts_amd._lib import PAD
from oracle import waveflow_oracle as wf

FACTOR = acr.FACTOR              # 8; measured ratios in the module docstring.  Beyond 32 an error is a finding, not a tolerance
EPS32 = 2.0 ** -23
PARITY_LOG = os.path.join(REPO, "profiles", "r21_02_ax_cond_glue_parity.jsonl")
SENTINEL = np.float32(-7.25)
GUARD = 64
B = 3
TS = (1, 255, 256, 257)
IDS = np.array([0, 511, 42], np.int64)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


class Buf:
    """A float32 numpy array inside a device allocation with sentinel guards either side."""

    def __init__(self, a):
        a = np.ascontiguousarray(a, np.float32)
        flat = np.full(a.size + 2 * GUARD, SENTINEL, np.float32)
        flat[GUARD:GUARD + a.size] = a.ravel()
        self.shape, self.n = a.shape, a.size
        self.t = torch.from_numpy(flat).cuda()

    def ptr(self, offset=0):
        return C.c_void_p(self.t.data_ptr() + 4 * (GUARD + offset))

    def get(self):
        torch.cuda.synchronize()
        h = self.t.cpu().numpy()
        assert (_bits(h[:GUARD]) == _bits(SENTINEL)).all() and (_bits(h[GUARD + self.n:]) == _bits(SENTINEL)).all(), "guard written"
        return h[GUARD:GUARD + self.n].reshape(self.shape).copy()


def _sentinel(*shape):
    return np.full(shape, SENTINEL, np.float32)


def _stream():
    return _lib.stream(torch.device("cuda", 0))


def _call(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*args, _stream()), name)


def _log(rec):
    print(json.dumps(rec))
    try:
        with open(PARITY_LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def _record(case, got, y64, y32, bound):
    """Log one arithmetic comparison; -> (L-inf of the HIP result, the record)."""
    err = np.abs(np.asarray(got, np.float64) - y64)
    linf = float(np.where(np.isnan(err), np.inf, err).max())
    e32 = float(np.abs(np.asarray(y32, np.float64) - y64).max())
    rec = dict(case=case, linf=linf, e32=e32, ratio=(linf / e32 if e32 else None), bound=float(np.max(bound)))
    _log(rec)
    return linf, rec


def _ld(T):
    return PAD + T + 11          # > pad + T, no multiple of anything


# ------------------------------------------------------------------------------------------------------- CPU sanity ----
def test_float64_deemphasis_matches_the_oracle_and_a_lost_carry_shows():
    """The float64 recurrence is the oracle's (scipy.signal.lfilter([1], [1, -p]) in the reference, ax:351-355); with a DC
    offset in the input, a carry lost between two of the kernel's 256 spans moves the output by orders of magnitude more than
    the bound of the GPU test - asserted here, on the reference alone."""
    for T in (1, 255, 257, 1000):
        ref = _deemph_case(T)
        assert _same_bits(ref["y64"].astype(np.float32), wf.deemphasis(ref["x"], 0.97))
        if T > 1:
            assert ref["lost_carry_moves"] >= 1000 * ref["bound"].max(), (T, ref["lost_carry_moves"])


@functools.lru_cache(maxsize=None)
def _deemph_case(T):
    rng = np.random.default_rng(T)
    x = (0.5 + 0.1 * rng.standard_normal((B, T))).astype(np.float32)
    y64 = acr.deemphasis64(x, 0.97)
    bound = 2.0 ** -24 * np.abs(y64) + 1e-12 * np.abs(y64).max()
    span = -(-T // 256)                                                          # the kernel's layout: 256 spans of ceil(T / 256)
    lost = np.concatenate([acr.deemphasis64(x[:, n:n + span], 0.97) for n in range(0, T, span)], axis=1)
    for a in (x, y64, bound):
        a.setflags(write=False)
    return dict(x=x, y64=y64, bound=bound, lost_carry_moves=float(np.abs(lost - y64).max()), span=span)


def test_deemphasis_lengths_sit_on_the_span_layout():
    assert _deemph_case(1000)["span"] == 4 and 256 - -(-1000 // 4) == 6          # T = 1000: six idle threads
    assert _deemph_case(257)["span"] == 2 and _deemph_case(256)["span"] == 1


# --------------------------------------------------------------------------------------------------------- movers ----
@pytest.mark.gpu
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("E", [1, 4, 20])
def test_embed_rows_writes_the_speaker_rows_and_nothing_else(hip_lib_path, E, T):
    rng = np.random.default_rng(100 * E + T)
    Cr, row0, ld = 27, 3, _ld(T)
    table = rng.standard_normal((_lib.N_SPEAKERS, E)).astype(np.float32)
    tab = torch.from_numpy(table).cuda()
    for ids in (IDS, np.array([0, -1, 42], np.int64), np.array([0, _lib.N_SPEAKERS, 42], np.int64)):
        x = Buf(_sentinel(B, Cr, ld))
        idt = torch.from_numpy(ids).cuda()
        _call("ctts_embed_rows_f32", _lib.ptr(tab), _lib.ptr(idt), x.ptr(), row0, E, B, Cr, T, ld, PAD)
        got = x.get()
        want = _sentinel(B, Cr, ld)
        for b in range(B):
            ok = 0 <= ids[b] < _lib.N_SPEAKERS
            want[b, row0:row0 + E, PAD:PAD + T] = table[ids[b]][:, None] if ok else np.nan
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), ids                           # a bad id poisons its own item, all of its rows
        assert nan[1, row0:row0 + E, PAD:PAD + T].all() == (not 0 <= ids[1] < _lib.N_SPEAKERS) and not nan[[0, 2]].any()
        assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), ids


@pytest.mark.gpu
@pytest.mark.parametrize("T", TS)
def test_pad_rows_and_unpad_rows_round_trip(hip_lib_path, T):
    rng = np.random.default_rng(T)
    Cr, ld = 21, _ld(T)
    src_rows, src_ld = Cr + 2, T + 3                                             # batch stride != C * T, row stride != T
    src = rng.standard_normal((B, src_rows, src_ld)).astype(np.float32)
    s, dst = Buf(src), Buf(_sentinel(B, Cr + 1, ld))                             # one spare row per item: the C the entry is given is
    for b in range(B):                                                          # Cr, the items are launched one by one
        _call("ctts_pad_rows_f32", s.ptr(b * src_rows * src_ld), src_rows * src_ld, src_ld, dst.ptr(b * (Cr + 1) * ld), 1, Cr, T,
              ld, PAD)
    got = dst.get()
    want = _sentinel(B, Cr + 1, ld)
    want[:, :Cr, PAD:PAD + T] = src[:, :Cr, :T]
    assert _same_bits(got, want)
    # the whole batch in one launch, dense destination rows
    dst2 = Buf(_sentinel(B, Cr, ld))
    _call("ctts_pad_rows_f32", s.ptr(), src_rows * src_ld, src_ld, dst2.ptr(), B, Cr, T, ld, PAD)
    assert _same_bits(dst2.get(), want[:, :Cr])
    # and back, into another dense layout
    back_rows, back_ld = Cr + 1, T + 2
    back = Buf(_sentinel(B, back_rows, back_ld))
    _call("ctts_unpad_rows_f32", dst2.ptr(), back.ptr(), back_rows * back_ld, back_ld, B, Cr, T, ld, PAD)
    want_back = _sentinel(B, back_rows, back_ld)
    want_back[:, :Cr, :T] = src[:, :Cr, :T]
    assert _same_bits(back.get(), want_back)
    assert _same_bits(s.get(), src)


@pytest.mark.gpu
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("s,p", [(2, 1), (3, 3), (4, 0)])
def test_interleave_phases_is_the_transposed_conv_output_order(hip_lib_path, s, p, extra, T):
    rng = np.random.default_rng(1000 * s + 10 * T + extra)
    Cr, T_in, T_out = 21, T + extra, s * T
    ld_in, ld_out = _ld(T_in), _ld(T_out)
    ph = rng.standard_normal((s, B, Cr, ld_in)).astype(np.float32)              # halo and tail columns hold values too: a read past
    phd, y = Buf(ph), Buf(_sentinel(B, Cr, ld_out))                             # T_in would show
    _call("ctts_interleave_phases_f32", phd.ptr(), y.ptr(), B, Cr, s, p, T_in, ld_in, PAD, T_out, ld_out, PAD)
    n = np.arange(T_out)
    r, m = (n + p) % s, (n + p) // s
    inside = m < T_in
    want = _sentinel(B, Cr, ld_out)
    want[:, :, PAD:PAD + T_out] = np.where(inside[None, None, :], ph[r, :, :, PAD + np.minimum(m, T_in - 1)].transpose(1, 2, 0), np.float32(0))
    if extra == 0 and p > 0:
        assert not inside.all()                                                 # columns with (n + p) / s >= T_in exist: they are 0
    assert _same_bits(y.get(), want)
    assert _same_bits(phd.get(), ph)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 257])
@pytest.mark.parametrize("halo", [1, 4])
def test_replicate_halo_fills_the_halo_only(hip_lib_path, halo, T):
    rng = np.random.default_rng(10 * T + halo)
    Cr, ld = 21, _ld(T)
    x = _sentinel(B, Cr, ld)
    x[:, :, PAD:PAD + T] = rng.standard_normal((B, Cr, T)).astype(np.float32)
    xd = Buf(x)
    _call("ctts_replicate_halo_f32", xd.ptr(), B, Cr, T, ld, PAD, halo)
    want = x.copy()
    want[:, :, PAD - halo:PAD] = x[:, :, PAD:PAD + 1]
    want[:, :, PAD + T:PAD + T + halo] = x[:, :, PAD + T - 1:PAD + T]
    assert _same_bits(xd.get(), want)                                           # columns beyond `halo` still hold the sentinel


@pytest.mark.gpu
@pytest.mark.parametrize("T_in", [1, 43, 129])
@pytest.mark.parametrize("factor", [2, 3, 30])
def test_resample_rows_nearest_by_scale_factor(hip_lib_path, factor, T_in):
    rng = np.random.default_rng(100 * factor + T_in)
    Cr, T_out = 5, T_in * factor
    ld_in, ld_out = _ld(T_in), _ld(T_out)
    x = rng.standard_normal((B, Cr + 2, ld_in)).astype(np.float32)
    xd, y = Buf(x[:, :Cr]), Buf(_sentinel(B, Cr, ld_out))
    _call("ctts_resample_rows_f32", xd.ptr(), y.ptr(), B, Cr, T_in, ld_in, PAD, T_out, ld_out, PAD, 2, float(factor))
    idx = acr.positions_nearest_scale(T_in, factor)
    assert len(idx) == T_out
    want = _sentinel(B, Cr, ld_out)
    want[:, :, PAD:PAD + T_out] = x[:, :Cr, PAD:PAD + T_in][:, :, idx]
    assert _same_bits(y.get(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("T", TS)
def test_resample_rows_shifted_copy_is_the_centre_crop(hip_lib_path, T):
    """``_to_latent_length``'s crop: 'nearest' at scale 1.0 from the source advanced by ``lo`` columns, one item per launch, more
    rows in the source buffer than are copied."""
    rng = np.random.default_rng(T)
    Cr, lo, hi = 21, 2, 2
    hT = T + lo + hi
    ld_in, ld_out = _ld(hT), _ld(T)
    x = rng.standard_normal((B, Cr + 11, ld_in)).astype(np.float32)
    xd, y = Buf(x), Buf(_sentinel(B, Cr + 3, ld_out))
    for b in range(B):
        _call("ctts_resample_rows_f32", xd.ptr(b * (Cr + 11) * ld_in + lo), y.ptr(b * (Cr + 3) * ld_out), 1, Cr, hT - lo, ld_in, PAD,
              T, ld_out, PAD, 2, 1.0)
    want = _sentinel(B, Cr + 3, ld_out)
    want[:, :Cr, PAD:PAD + T] = x[:, :Cr, PAD + lo:PAD + lo + T]
    assert _same_bits(y.get(), want)


# ------------------------------------------------------------------------------------------- one or two roundings ----
@pytest.mark.gpu
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("alias", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("with_r", [False, True], ids=["no_r", "r"])
@pytest.mark.parametrize("with_alpha", [False, True], ids=["no_alpha", "alpha"])
def test_scale_add_rows_within_two_roundings(hip_lib_path, with_alpha, with_r, alias, T):
    """y = alpha * x + r: a product and a sum, contracted into one fma or not - |got - y64| <= 2^-23 (|alpha x| + |r|)."""
    rng = np.random.default_rng(T + 1000 * with_alpha + 2000 * with_r)
    Cr, ld = 21, _ld(T)
    x = _sentinel(B, Cr, ld)
    x[:, :, PAD:PAD + T] = rng.standard_normal((B, Cr, T)).astype(np.float32)
    r = rng.standard_normal((B, Cr, ld)).astype(np.float32)
    alpha = np.array([0.8125 + 2.0 ** -20], np.float32)                          # not a power of two: the product really rounds
    xd, rd, ad = Buf(x), Buf(r), torch.from_numpy(alpha).cuda()
    yd = xd if alias else Buf(_sentinel(B, Cr, ld))
    _call("ctts_scale_add_rows_f32", xd.ptr(), _lib.ptr(ad) if with_alpha else None, rd.ptr() if with_r else None, yd.ptr(), B,
          Cr, T, ld, PAD)
    got = yd.get()
    a64 = float(alpha[0]) if with_alpha else 1.0
    xv, rv = x[:, :, PAD:PAD + T].astype(np.float64), (r[:, :, PAD:PAD + T].astype(np.float64) if with_r else 0.0)
    y64 = a64 * xv + rv
    bound = EPS32 * (np.abs(a64 * xv) + np.abs(rv))
    a32 = alpha[0] if with_alpha else np.float32(1)
    y32 = a32 * x[:, :, PAD:PAD + T] + (r[:, :, PAD:PAD + T] if with_r else np.float32(0))
    linf, rec = _record(f"scale_add_rows alpha={with_alpha} r={with_r} alias={alias} T={T}", got[:, :, PAD:PAD + T], y64, y32, bound)
    assert (np.abs(got[:, :, PAD:PAD + T].astype(np.float64) - y64) <= bound).all(), (rec, acr.worst(got[:, :, PAD:PAD + T], y64))
    outside = np.ones((B, Cr, ld), bool)
    outside[:, :, PAD:PAD + T] = False
    assert (_bits(got)[outside] == _bits(SENTINEL)).all()
    if not alias:
        assert _same_bits(xd.get(), x)
    assert _same_bits(rd.get(), r)


@pytest.mark.gpu
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("shift,scale", [(11.52, 0.25), (1.0, 0.5), (-0.3, 1.7)])
def test_affine_rows_within_two_roundings_on_its_rows_only(hip_lib_path, shift, scale, T):
    """x = (x + shift) * scale on rows [0, rows) of C: a sum and a product, each within 2^-24 relative -> 1.01 * 2^-23 |y64|."""
    rng = np.random.default_rng(T)
    Cr, rows, ld = 21, 13, _ld(T)
    x = _sentinel(B, Cr, ld)
    x[:, :, PAD:PAD + T] = rng.standard_normal((B, Cr, T)).astype(np.float32)
    xd = Buf(x)
    _call("ctts_affine_rows_f32", xd.ptr(), B, Cr, rows, T, ld, PAD, shift, scale)
    got = xd.get()
    xv = x[:, :rows, PAD:PAD + T]
    y64 = (xv.astype(np.float64) + float(np.float32(shift))) * float(np.float32(scale))
    y32 = (xv + np.float32(shift)) * np.float32(scale)
    bound = 1.01 * EPS32 * np.abs(y64)
    linf, rec = _record(f"affine_rows shift={shift} scale={scale} T={T}", got[:, :rows, PAD:PAD + T], y64, y32, bound)
    assert (np.abs(got[:, :rows, PAD:PAD + T].astype(np.float64) - y64) <= bound).all(), (rec, acr.worst(got[:, :rows, PAD:PAD + T], y64))
    want = x.copy()
    want[:, :rows, PAD:PAD + T] = got[:, :rows, PAD:PAD + T]
    assert _same_bits(got, want)                                                # rows above `rows`, halo and tail: untouched


def _lerp_case(name, pos, T_in, T_out, mode, scale_factor):
    """resample_rows in a linear mode against float64 with the fp32 positions `pos`: gemm_lerp is one product rounding plus one
    fma rounding -> |got - y64| <= 2^-23 (l0 |a| + l1 |b|) per element."""
    i0, i1, l0, l1 = pos
    assert len(i0) == T_out
    rng = np.random.default_rng(1000 * T_in + T_out)
    Cr = 5
    ld_in, ld_out = _ld(T_in), _ld(T_out)
    x = rng.standard_normal((B, Cr, ld_in)).astype(np.float32)                  # halo and tail hold values: a read past T_in shows
    xd, y = Buf(x), Buf(_sentinel(B, Cr, ld_out))
    _call("ctts_resample_rows_f32", xd.ptr(), y.ptr(), B, Cr, T_in, ld_in, PAD, T_out, ld_out, PAD, mode, scale_factor)
    got = y.get()
    xv = x[:, :, PAD:PAD + T_in]
    a, b = xv[..., i0].astype(np.float64), xv[..., i1].astype(np.float64)
    y64 = l0.astype(np.float64) * a + l1.astype(np.float64) * b
    y32 = l0 * xv[..., i0] + l1 * xv[..., i1]
    bound = EPS32 * (l0 * np.abs(a) + l1 * np.abs(b))
    rows = got[:, :, PAD:PAD + T_out]
    linf, rec = _record(name, rows, y64, y32, bound)
    assert (np.abs(rows.astype(np.float64) - y64) <= bound).all(), (rec, acr.worst(rows, y64))
    outside = np.ones((B, Cr, ld_out), bool)
    outside[:, :, PAD:PAD + T_out] = False
    assert (_bits(got)[outside] == _bits(SENTINEL)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("T_in,T_out", [(1, 5), (2, 257), (7, 7), (129, 645), (645, 129)])
def test_resample_rows_linear_align_corners(hip_lib_path, T_in, T_out):
    _lerp_case(f"resample_rows mode=0 {T_in}->{T_out}", acr.positions_align_corners(T_in, T_out), T_in, T_out, 0, 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("T_in", [1, 2, 43])
@pytest.mark.parametrize("factor", [2, 6, 30])
def test_resample_rows_linear_by_scale_factor(hip_lib_path, factor, T_in):
    pos = acr.positions_linear_scale(T_in, factor)
    assert pos[0][0] == 0 and pos[3][0] == 0 and (pos[0][-1] == pos[1][-1] == T_in - 1)       # the clamp at both ends
    _lerp_case(f"resample_rows mode=1 x{factor} T_in={T_in}", pos, T_in, T_in * factor, 1, float(factor))


# ------------------------------------------------------------------------------------------------------- vol_unscale ----
SPECIAL = np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -20, -2.0 ** -20, 3.7, -3.7, np.nan], np.float32)


def _vol_vector():
    """257 inputs: the special values, 100 normal deviates, 148 magnitudes log-uniform in [2^-20, 4] of either sign."""
    rng = np.random.default_rng(257)
    m = 257 - len(SPECIAL) - 100
    mag = np.exp2(rng.uniform(-20, 2, m)).astype(np.float32) * rng.choice([-1, 1], m).astype(np.float32)
    return np.concatenate([SPECIAL, rng.standard_normal(100).astype(np.float32), mag]).astype(np.float32)


def _vol_rel(y, y64, ok):
    return np.abs(np.asarray(y, np.float64)[ok] - y64[ok]) / np.abs(y64[ok])


def _vol_derived_bound(x):
    """Relative error a 1-ulp log2f followed by a 1-ulp powf can leave on 10^log2|x|: the error of log2 (<= 2^-23 |log2 x|) is
    amplified by ln 10, the power adds its own ulp -> 2^-23 (1 + ln 10 |log2 x|), 1 % for the second-order terms."""
    return 1.01 * EPS32 * (1.0 + np.log(10.0) * np.abs(np.log2(np.abs(np.asarray(x, np.float64)))))


def _vol_launch(x):
    """One launch over x -> (result, float64 reference, mask of the elements with a relative error); the exact properties hold
    for every input: NaN stays NaN, zeros keep their bits, the sign is kept."""
    xd = Buf(x)
    _call("ctts_vol_unscale_f32", xd.ptr(), x.size)
    got = xd.get()
    y64 = acr.vol_unscale(x.astype(np.float64), np.float64)
    nan, zero = np.isnan(x), x == 0
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[zero], _bits(x)[zero])                      # zeros stay the zeros they were
    assert np.array_equal(np.signbit(got)[~nan], np.signbit(x)[~nan])
    return got, y64, ~nan & ~zero


def _vol_log(case, rel, e32_rel, bound, held_to):
    rec = dict(case=case, rel_linf=float(rel.max()), e32_rel=e32_rel, ratio=(float(rel.max()) / e32_rel if e32_rel else None),
               bound=float(bound), held_to=held_to, factor=FACTOR)
    _log(rec)
    return rec


@pytest.mark.gpu
def test_vol_unscale_against_float64(hip_lib_path):
    """sign(x) 10^log2|x| at n = 257 (the special values inside the vector) and n = 1: the relative error against float64 is at
    most FACTOR x the largest relative error of the numpy fp32 restatement ON THE INPUTS OF THAT LAUNCH (the error of log2 is
    amplified by ln 10 |log2 x| in both).  One element against one rounding is a lottery, so the n = 1 launch takes the
    element of the vector where the restatement's own error is largest - chosen on the reference alone."""
    x = _vol_vector()
    assert x.size == 257
    y32 = acr.vol_unscale(x, np.float32)
    got, y64, ok = _vol_launch(x)
    e32 = _vol_rel(y32, y64, ok)
    assert e32.max() > 2.0 ** -24 and (e32 <= _vol_derived_bound(x[ok])).all()    # amplified, and inside the derivation's bound
    rel = _vol_rel(got, y64, ok)
    rec = _vol_log("vol_unscale n=257", rel, float(e32.max()), FACTOR * e32.max(), "FACTOR x own e32")
    assert rel.max() <= FACTOR * e32.max(), (rec, x[ok][int(np.argmax(rel))])
    one = x[ok][int(np.argmax(e32))].reshape(1)
    got1, y64_1, ok1 = _vol_launch(one)
    e32_1 = _vol_rel(acr.vol_unscale(one, np.float32), y64_1, ok1)
    assert e32_1.max() == e32.max()
    rel1 = _vol_rel(got1, y64_1, ok1)
    rec = _vol_log(f"vol_unscale n=1 x={float(one[0])!r}", rel1, float(e32_1.max()), FACTOR * e32_1.max(), "FACTOR x own e32")
    assert rel1.max() <= FACTOR * e32_1.max(), rec


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SPECIAL)), ids=[repr(float(v)) for v in SPECIAL])
def test_vol_unscale_single_special_values(hip_lib_path, i):
    """Each special value as a launch of its own (one thread): the exact properties, and - NOT the own-e32 rule: a single
    element's fp32 restatement error is whatever one rounding happened to be, e.g. 1.63e-8 at 3.7 where the HIP result is
    1.81e-7 off (11.1 x it) - the derived bound of two 1-ulp device functions, 2^-23 (1 + ln 10 |log2 x|) (6.4e-7 at 3.7).
    The record carries the true ratio against the element's own e32."""
    x = SPECIAL[i:i + 1].copy()
    got, y64, ok = _vol_launch(x)
    if not ok.any():
        return
    rel = _vol_rel(got, y64, ok)
    e32 = _vol_rel(acr.vol_unscale(x, np.float32), y64, ok)
    bound = _vol_derived_bound(x)
    rec = _vol_log(f"vol_unscale n=1 special x={float(x[0])!r}", rel, float(e32.max()), bound.max(), "derived 2^-23 (1 + ln10 |log2 x|)")
    assert (rel <= bound).all(), rec
    if abs(float(x[0])) == 1.0:
        assert rel.max() == 0.0                                                  # 10^0


# -------------------------------------------------------------------------------------------------------- deemphasis ----
@pytest.mark.gpu
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("T", [1, 255, 256, 257, 1000, 66150])
def test_deemphasis_carries_float64_state_across_the_spans(hip_lib_path, T, in_place):
    ref = _deemph_case(T)
    if T > 1:
        assert ref["lost_carry_moves"] >= 1000 * ref["bound"].max()
    xd = Buf(ref["x"])
    yd = xd if in_place else Buf(_sentinel(B, T))
    _call("ctts_deemphasis_f32", xd.ptr(), yd.ptr(), B, T, C.c_double(0.97))
    got = yd.get()
    y32 = wf.deemphasis(ref["x"], 0.97)
    linf, rec = _record(f"deemphasis T={T} in_place={in_place}", got, ref["y64"], y32, ref["bound"])
    err = np.abs(got.astype(np.float64) - ref["y64"])
    assert (err <= ref["bound"]).all(), (rec, acr.worst(got[:, None, :], ref["y64"][:, None, :]))
    if not in_place:
        assert _same_bits(xd.get(), ref["x"])


# --------------------------------------------------------------------------------------------------- fold_weightnorm ----
@pytest.mark.gpu
@pytest.mark.parametrize("out_ch", [1, 5])
@pytest.mark.parametrize("fan", [1, 3, 63, 64, 65, 255, 256, 257, 3744])
def test_fold_weightnorm_against_float64(hip_lib_path, fan, out_ch):
    """w[o] = v[o] * (g[o] / ||v[o]||): 256 threads stride the row, four waves reduce.  Per row:
    max(FACTOR * e32, 4 * 2^-23 * max|w64|), e32 the numpy fp32 restatement's distance from float64 on that row."""
    rng = np.random.default_rng(10 * fan + out_ch)
    v = rng.standard_normal((out_ch, fan)).astype(np.float32)
    g = (rng.uniform(0.5, 2.0, out_ch) * np.where(np.arange(out_ch) % 2, -1.0, 1.0)).astype(np.float32)
    if out_ch > 1:
        assert (g > 0).any() and (g < 0).any()
    else:
        g = -g if fan % 2 else g                                                 # both signs over the single-row cases
    w64 = acr.fold_weightnorm(g, v, np.float64)
    w32 = acr.fold_weightnorm(g, v, np.float32)
    assert w64.dtype == np.float64 and w32.dtype == np.float32
    vd, gd, wd = Buf(v), Buf(g), Buf(_sentinel(out_ch, fan))
    _call("ctts_fold_weightnorm_f32", vd.ptr(), gd.ptr(), wd.ptr(), out_ch, fan)
    got = wd.get()
    err = np.abs(got.astype(np.float64) - w64).max(axis=1)
    e32 = np.abs(w32.astype(np.float64) - w64).max(axis=1)
    bound = np.maximum(FACTOR * e32, 4 * EPS32 * np.abs(w64).max(axis=1))
    o = int(np.argmax(err / bound))
    rec = dict(case=f"fold_weightnorm fan={fan} out_ch={out_ch}", linf=float(err[o]), e32=float(e32[o]),
               ratio=(float(err[o] / e32[o]) if e32[o] else None), bound=float(bound[o]), factor=FACTOR)
    _log(rec)
    assert np.isfinite(got).all() and (err <= bound).all(), (rec, f"row {o}, column {int(np.argmax(np.abs(got[o] - w64[o])))}")
    assert _same_bits(vd.get(), v) and _same_bits(gd.get(), g)
