"""The Winograd F(6,3) hex form of the fp32 WaveGlow in-layers: its constants, its column map and its knobs (no GPU).

1. the algebra: with the interpolation points 0, +-1, +-2, +-1/2, inf the matrices the library packs with (winograd_g63_kernel: G),
   transforms with (winograd_transform_hex_kernel: B^T) and combines with (wn_winograd_layer.hip: A^T, multipliers 2^-5 .. 2^5)
   satisfy A^T [(G g) . (B^T d)] = correlation(g, d) for random g, d in float64 - also in the grouping the kernels use
   (P1 +- P2, P3 +- P4, P5 +- P6; even / odd halves of the transform).
2. the mapping: hex column q of a layer of dilation d stands for t_k = (q / d) 6d + q % d + k d, k = 0..5, with
   Lh = ceil(L / 6d) d hex columns; a member is stored when it lies below L.  The six members together hit every column of
   [0, L) exactly once - also where L is no multiple of 6d and where L < 6d.
3. the knobs: CTTS_F32_WINOGRAD_F63_MIN and CTTS_F32_WINOGRAD_NO_F63 have bits of their own, are documented, and the library
   reads them.
"""
import os
from fractions import Fraction as Fr

import numpy as np
import pytest

from conftest import REPO
from cookietts_amd import _lib

TOL = 1e-9                                                     # the issue's: the matrices reproduce the conv to 1e-9 in float64
DILATIONS = [1 << i for i in range(8)]

# rows j = 0..7 (the eight products), as the kernels spell them
G = np.array([[1, 0, 0], [Fr(-2, 9)] * 3, [Fr(-2, 9), Fr(2, 9), Fr(-2, 9)], [Fr(1, 90), Fr(1, 45), Fr(2, 45)], [Fr(1, 90), Fr(-1, 45), Fr(2, 45)],
              [Fr(32, 45), Fr(16, 45), Fr(8, 45)], [Fr(32, 45), Fr(-16, 45), Fr(8, 45)], [0, 0, 1]], dtype=object).astype(np.float64)
BT = np.array([[1, 0, -21 / 4, 0, 21 / 4, 0, -1, 0],
               [0, 1, 1, -17 / 4, -17 / 4, 1, 1, 0],
               [0, -1, 1, 17 / 4, -17 / 4, -1, 1, 0],
               [0, 1 / 2, 1 / 4, -5 / 2, -5 / 4, 2, 1, 0],
               [0, -1 / 2, 1 / 4, 5 / 2, -5 / 4, -2, 1, 0],
               [0, 2, 4, -5 / 2, -5, 1 / 2, 1, 0],
               [0, -2, 4, 5 / 2, -5, -1 / 2, 1, 0],
               [0, -1, 0, 21 / 4, 0, -21 / 4, 0, 1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 1, 1, 1, 1, 0],
               [0, 1, -1, 2, -2, 1 / 2, -1 / 2, 0],
               [0, 1, 1, 4, 4, 1 / 4, 1 / 4, 0],
               [0, 1, -1, 8, -8, 1 / 8, -1 / 8, 0],
               [0, 1, 1, 16, 16, 1 / 16, 1 / 16, 0],
               [0, 1, -1, 32, -32, 1 / 32, -1 / 32, 1]], dtype=np.float64)


def _kernel_form(g, d):
    """The products and the combination exactly as the layer kernel groups them, and the transform as its kernel spells it."""
    x0, x1, x2, x3, x4, x5, x6, x7 = d
    e1, o1 = (x2 + x6) - 4.25 * x4, (x1 + x5) - 4.25 * x3
    e2, o2 = (0.25 * x2 + x6) - 1.25 * x4, (0.5 * x1 + 2 * x5) - 2.5 * x3
    e3, o3 = (4 * x2 + x6) - 5 * x4, (2 * x1 + 0.5 * x5) - 2.5 * x3
    V = [(x0 - x6) + 5.25 * (x4 - x2), e1 + o1, e1 - o1, e2 + o2, e2 - o2, e3 + o3, e3 - o3, (x7 - x1) + 5.25 * (x3 - x5)]
    w0, w1, w2 = g
    U = [w0, -2 * (w0 + w1 + w2) / 9, -2 * (w0 - w1 + w2) / 9, w0 / 90 + w1 / 45 + 2 * w2 / 45, w0 / 90 - w1 / 45 + 2 * w2 / 45,
         32 * w0 / 45 + 16 * w1 / 45 + 8 * w2 / 45, 32 * w0 / 45 - 16 * w1 / 45 + 8 * w2 / 45, w2]
    P = [u * v for u, v in zip(U, V)]
    sa, sb, sc, se, sf, sg = P[1] + P[2], P[1] - P[2], P[3] + P[4], P[3] - P[4], P[5] + P[6], P[5] - P[6]
    return np.array([(sa + sc) + sf + P[0], (sb + 2 * se) + sg / 2, (sa + 4 * sc) + sf / 4, (sb + 8 * se) + sg / 8,
                     (sa + 16 * sc) + sf / 16, (sb + 32 * se) + sg / 32 + P[7]])


def test_f63_constants_give_the_correlation():
    rng = np.random.default_rng(63)
    for _ in range(200):
        g, d = rng.standard_normal(3), rng.standard_normal(8)
        want = np.array([sum(g[t] * d[k + t] for t in range(3)) for k in range(6)])
        got = AT @ ((G @ g) * (BT @ d))
        assert np.max(np.abs(got - want)) < TOL
        assert np.max(np.abs(_kernel_form(g, d) - want)) < TOL


def test_output_side_multipliers_are_powers_of_two():
    m = np.abs(AT[AT != 0])
    assert set(m.tolist()) == {2.0 ** e for e in range(-5, 6)}
    # the four outputs without an end product, and the two with one
    assert (AT[1:5, 0] == 0).all() and (AT[1:5, 7] == 0).all() and AT[0, 0] == AT[5, 7] == 1 and AT[0, 7] == AT[5, 0] == 0


@pytest.mark.parametrize("d", DILATIONS)
def test_hex_columns_cover_every_column_once(d):
    for L in sorted({1, d, 2 * d, 5 * d, 6 * d - 1, 6 * d, 6 * d + 1, 7 * d, 11 * d + 1, 160, 288, 416, 1184}):
        Lh = (L + 6 * d - 1) // (6 * d) * d
        hits = np.zeros(L + 6 * d + 1, dtype=int)
        dropped = 0
        for q in range(Lh):
            for k in range(6):
                ns = (q // d) * 6 * d + q % d + k * d           # the kernel's rule, stored when ns < L
                if ns < L:
                    hits[ns] += 1
                else:
                    dropped += 1
        assert (hits[:L] == 1).all() and (hits[L:] == 0).all(), (d, L)
        assert dropped == 6 * Lh - L and 6 * Lh - L < 6 * d, (d, L)      # never a whole hex block beyond the end
        # and back: natural column t -> (hex column, member)
        for t in range(L):
            blk, r = divmod(t, 6 * d)
            q, k = blk * d + r % d, r // d
            assert q < Lh and (q // d) * 6 * d + q % d + k * d == t


def test_hex_form_of_a_dilated_conv_matches_the_direct_form():
    """A whole dilated 3-tap conv row by row through the hex map, zero padding included, L no multiple of 6d and L < 6d."""
    rng = np.random.default_rng(7)
    for d, L in [(1, 37), (4, 160), (4, 416), (64, 160), (128, 160), (128, 1184), (32, 1184)]:
        C = 5
        x, w = rng.standard_normal((C, L)), rng.standard_normal((3, C))
        xp = np.zeros((C, L + 8 * d + 6 * d))
        xp[:, d:d + L] = x                                      # xp[:, t + d] = x[t], zero outside [0, L)
        direct = sum(w[t] @ xp[:, t * d:t * d + L] for t in range(3))
        Lh = (L + 6 * d - 1) // (6 * d) * d
        got = np.full(L, np.nan)
        for q in range(Lh):
            t0 = (q // d) * 6 * d + q % d
            taps = np.stack([xp[:, t0 + j * d] for j in range(8)])               # x[t0 + (j - 1) d]
            y = AT @ np.einsum("jc,jc->j", (G @ w), (BT @ taps))
            for k in range(6):
                if t0 + k * d < L:
                    got[t0 + k * d] = y[k]
        assert np.max(np.abs(got - direct)) < TOL * max(1.0, np.max(np.abs(direct))), (d, L)


NEW = ("CTTS_F32_WINOGRAD_F63_MIN", "CTTS_F32_WINOGRAD_NO_F63")


def test_new_knobs_have_bits_of_their_own_and_are_documented():
    bits = dict(_lib.TUNING_BITS, **_lib.TUNING_BITS_EXT)
    assert all(n in _lib.TUNING_BITS_EXT and n not in _lib.TUNING_BITS for n in NEW) and {bits[n] for n in NEW} == {32, 33}
    assert len(bits) == len(_lib.TUNING_BITS) + len(_lib.TUNING_BITS_EXT) and len(set(bits.values())) == len(bits)
    hdr = open(os.path.join(REPO, "include", "cookietts_hip.h")).read()
    tun = open(os.path.join(REPO, "cookietts_amd", "csrc", "tuning.h")).read()
    for n in NEW:
        assert f"{bits[n]} {n}" in hdr and n in tun, n


def test_library_reads_the_new_knobs(hip_lib_path, monkeypatch):
    for n in NEW + ("CTTS_F32_WINOGRAD_F43_MIN", "CTTS_F32_WINOGRAD_NO_F43"):
        monkeypatch.delenv(n, raising=False)
    _lib.tuning_reload()
    try:
        assert not any(_lib.tuning_active(n) for n in NEW)
        monkeypatch.setenv("CTTS_F32_WINOGRAD_F63_MIN", "0")            # 0 = always: set, not "off"
        _lib.tuning_reload()
        assert _lib.tuning_active("CTTS_F32_WINOGRAD_F63_MIN") and not _lib.tuning_active("CTTS_F32_WINOGRAD_NO_F63")
        assert not _lib.tuning_active("CTTS_F32_WINOGRAD_F43_MIN") and not _lib.tuning_active("CTTS_F32_WINOGRAD_NO_F43")
        monkeypatch.setenv("CTTS_F32_WINOGRAD_NO_F63", "1")
        _lib.tuning_reload()
        assert all(_lib.tuning_active(n) for n in NEW) and not _lib.tuning_active("CTTS_F32_WINOGRAD_NO_F43")
    finally:
        monkeypatch.undo()
        _lib.tuning_reload()
