"""The Winograd F(4,3) quad form of the fp32 WaveGlow in-layers: its constants, its column map and its knobs (no GPU).

1. the algebra: with the interpolation points 0, +-1, +-2, inf the matrices the library packs with (winograd_g43_kernel: G),
   transforms with (winograd_transform_quad_kernel: B^T) and combines with (wn_winograd_layer.hip: A^T, multipliers 1, 2, 4, 8)
   satisfy A^T [(G g) . (B^T d)] = correlation(g, d) for random g, d - also in the grouping the kernels use (P1 +- P2, P3 +- P4).
2. the mapping: quad column q of a layer of dilation d stands for t_k = (q / d) 4d + q % d + k d, k = 0..3, with
   Lq = ceil(L / 4d) d quad columns; a member is stored when it lies below L.  The four members together hit every column of
   [0, L) exactly once - also where L is no multiple of 4d and where L < 4d.
3. the knobs: CTTS_F32_WINOGRAD_F43_MIN and CTTS_F32_WINOGRAD_NO_F43 have bits of their own, are documented, and the library
   reads them.
"""
import os

import numpy as np
import pytest

from conftest import REPO
from cookietts_amd import _lib

TOL = 1e-11                                                    # test_winograd_algebra.py's
DILATIONS = [1 << i for i in range(8)]

# rows j = 0..5 (the six products), as the kernels spell them
G = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]])
BT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)


def _kernel_form(g, d):
    """The products and the combination exactly as the layer kernel groups them, and the transform as its kernel spells it."""
    x0, x1, x2, x3, x4, x5 = d
    s12, d12, s34, d34, d13, d24 = x1 + x2, x1 - x2, x3 + x4, x3 - x4, x1 - x3, x2 - x4
    V = [4 * x0 - 5 * x2 + x4, s34 - 4 * s12, 4 * d12 - d34, -2 * d13 - d24, 2 * d13 - d24, 4 * x1 - 5 * x3 + x5]
    w0, w1, w2 = g
    U = [w0 / 4, -(w0 + w1 + w2) / 6, -(w0 - w1 + w2) / 6, w0 / 24 + w1 / 12 + w2 / 6, w0 / 24 - w1 / 12 + w2 / 6, w2]
    P = [u * v for u, v in zip(U, V)]
    a, b, c, e = P[1] + P[2], P[1] - P[2], P[3] + P[4], P[3] - P[4]
    return np.array([a + c + P[0], b + 2 * e, a + 4 * c, b + 8 * e + P[5]])


def test_f43_constants_give_the_correlation():
    rng = np.random.default_rng(43)
    for _ in range(200):
        g, d = rng.standard_normal(3), rng.standard_normal(6)
        want = np.array([sum(g[t] * d[k + t] for t in range(3)) for k in range(4)])
        got = AT @ ((G @ g) * (BT @ d))
        assert np.max(np.abs(got - want)) < TOL
        assert np.max(np.abs(_kernel_form(g, d) - want)) < TOL


def test_output_side_multipliers_are_powers_of_two():
    m = np.abs(AT[AT != 0])
    assert set(m.tolist()) == {1.0, 2.0, 4.0, 8.0}
    # the two outputs without an end product, and the two with one
    assert AT[1, 0] == AT[1, 5] == AT[2, 0] == AT[2, 5] == 0 and AT[0, 0] == AT[3, 5] == 1 and AT[0, 5] == AT[3, 0] == 0


@pytest.mark.parametrize("d", DILATIONS)
def test_quad_columns_cover_every_column_once(d):
    for L in sorted({1, d, 2 * d, 3 * d, 4 * d - 1, 4 * d, 4 * d + 1, 5 * d, 7 * d + 1, 160, 288, 1184}):
        Lq = (L + 4 * d - 1) // (4 * d) * d
        hits = np.zeros(L + 4 * d + 1, dtype=int)
        dropped = 0
        for q in range(Lq):
            for k in range(4):
                ns = (q // d) * 4 * d + q % d + k * d           # the kernel's rule, stored when ns < L
                if ns < L:
                    hits[ns] += 1
                else:
                    dropped += 1
        assert (hits[:L] == 1).all() and (hits[L:] == 0).all(), (d, L)
        assert dropped == 4 * Lq - L and 4 * Lq - L < 4 * d, (d, L)      # never a whole quad block beyond the end
        # and back: natural column t -> (quad column, member)
        for t in range(L):
            blk, r = divmod(t, 4 * d)
            q, k = blk * d + r % d, r // d
            assert q < Lq and (q // d) * 4 * d + q % d + k * d == t


def test_quad_form_of_a_dilated_conv_matches_the_direct_form():
    """A whole dilated 3-tap conv row by row through the quad map, zero padding included, L no multiple of 4d and L < 4d."""
    rng = np.random.default_rng(7)
    for d, L in [(1, 37), (2, 37), (4, 160), (64, 160), (128, 160), (128, 1184), (32, 1184)]:
        C = 5
        x, w = rng.standard_normal((C, L)), rng.standard_normal((3, C))
        xp = np.zeros((C, L + 6 * d + 4 * d))
        xp[:, d:d + L] = x                                      # xp[:, t + d] = x[t], zero outside [0, L)
        direct = sum(w[t] @ xp[:, t * d:t * d + L] for t in range(3))
        Lq = (L + 4 * d - 1) // (4 * d) * d
        got = np.full(L, np.nan)
        for q in range(Lq):
            t0 = (q // d) * 4 * d + q % d
            taps = np.stack([xp[:, t0 + j * d] for j in range(6)])               # x[t0 + (j - 1) d]
            y = AT @ np.einsum("jc,jc->j", (G @ w), (BT @ taps))
            for k in range(4):
                if t0 + k * d < L:
                    got[t0 + k * d] = y[k]
        assert np.max(np.abs(got - direct)) < TOL * max(1.0, np.max(np.abs(direct))), (d, L)


NEW = ("CTTS_F32_WINOGRAD_F43_MIN", "CTTS_F32_WINOGRAD_NO_F43")


def test_new_knobs_have_bits_of_their_own_and_are_documented():
    bits = _lib.TUNING_BITS
    assert all(n in bits for n in NEW) and {bits[n] for n in NEW} == {6, 22}
    assert len(set(bits.values())) == len(bits) and all(0 <= b <= 30 for b in bits.values())
    hdr = open(os.path.join(REPO, "include", "cookietts_hip.h")).read()
    tun = open(os.path.join(REPO, "cookietts_amd", "csrc", "tuning.h")).read()
    for n in NEW:
        assert f"{bits[n]} {n}" in hdr and n in tun, n


def test_library_reads_the_new_knobs(hip_lib_path, monkeypatch):
    for n in NEW + ("CTTS_F32_WINOGRAD_MIN", "CTTS_F32_WINOGRAD_FUSED_MIN", "CTTS_F32_WINOGRAD_NO_FUSED"):
        monkeypatch.delenv(n, raising=False)
    _lib.tuning_reload()
    try:
        assert not any(_lib.tuning_active(n) for n in NEW)
        monkeypatch.setenv("CTTS_F32_WINOGRAD_F43_MIN", "0")            # 0 = always: set, not "off"
        _lib.tuning_reload()
        assert _lib.tuning_active("CTTS_F32_WINOGRAD_F43_MIN") and not _lib.tuning_active("CTTS_F32_WINOGRAD_NO_F43")
        assert not _lib.tuning_active("CTTS_F32_WINOGRAD_FUSED_MIN") and not _lib.tuning_active("CTTS_F32_WINOGRAD_MIN")
        monkeypatch.setenv("CTTS_F32_WINOGRAD_NO_F43", "1")
        _lib.tuning_reload()
        assert all(_lib.tuning_active(n) for n in NEW) and not _lib.tuning_active("CTTS_F32_WINOGRAD_NO_FUSED")
    finally:
        monkeypatch.undo()
        _lib.tuning_reload()
