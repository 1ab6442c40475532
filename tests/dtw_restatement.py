"""numpy restatement of the reference's ``DTW`` (``_4_mtw/waveglow/mel2samp.py:81-118``), at float64 and at float32.

For one item ``pred, target [C, T]`` with ``s = scale_factor``, ``r = range_`` (odd), ``h = r // 2``: ``P`` is ``pred`` with ``h`` zero frames
on each side (``Tp = T + 2h``); ``E = F.interpolate(P, scale_factor=float(s), mode='linear', align_corners=False)`` has ``s * Tp`` entries,
``E[p] = (1 - lam) P[i0] + lam P[i1]`` with ``src = max(0, (p + 0.5) / s - 0.5)``, ``i0 = floor(src)``, ``i1 = min(i0 + 1, Tp - 1)``,
``lam = src - i0``; candidate ``j`` at frame ``t`` is ``E[j + t s]``.  The running best starts as ``pred``; candidates are tried in ascending
``j`` and replace it only when their ``sum_c |cand - target|`` is strictly smaller.

The float64 arm uses the exact weights ``(j + 0.5) / s - 0.5`` (they depend on ``j`` alone); the float32 arm mimics the reference's CPU
arithmetic: ``rs = float32(1 / s)``, ``src = rs * (p + 0.5) - 0.5`` at every expanded index in float32, both products rounded, float32 sums.

``MISTAKES`` are deliberate one-mistake variants; tests/test_dtw.py shows that the goldens tell each of them from the real thing.
"""
import os

import numpy as np

FACTOR = 8                      # the project's factor on e32 (tests/ax_cond_f64_restatement.py:50)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MISTAKES = ("le", "replicate_pad", "align_corners", "last_first")

# the smallest shapes at which the kernel can go wrong.  amp: the scale of the random walk (one frame has no neighbours to be warped
# onto: at the noise's own scale a shrunk copy of it wins there, and such candidates tie in pairs)
CASES = {
    "s8r5_t67": dict(s=8, r=5, C=80, T=67, B=3, seed=3201),            # T not a multiple of 64
    "s5r5_c160": dict(s=5, r=5, C=160, T=130, B=2, seed=3202),         # inexact 1/5
    "s5r3_t200": dict(s=5, r=3, C=80, T=200, B=2, seed=3203),          # the HiFi-GAN call
    "s3r1_t67": dict(s=3, r=1, C=80, T=67, B=2, seed=3204),            # no padding, both end clamps live
    "s8r5_c7_t3": dict(s=8, r=5, C=7, T=3, B=2, seed=3205),            # the whole item inside the padding; C below any channel slicing
    "s8r5_t1": dict(s=8, r=5, C=80, T=1, B=1, seed=3206, amp=0.05),
}


def tau(C):
    """Relative bound between an fp32 L1 (a sum of C rounded terms, each from a rounded candidate) and the float64 one: two fp32 sums
    of C rounded terms, times two for margin."""
    return 4 * (C + 4) * 2.0 ** -24


def signals(case):
    """-> (pred, target) float32 [B, C, T], every value representable in float16 (the fixtures store them as such).  target: a random
    walk over time; pred: that walk read at a slowly drifting fractional offset, plus noise of 0.05."""
    c = CASES[case]
    rng = np.random.default_rng(c["seed"])
    B, C, T, amp = c["B"], c["C"], c["T"], c.get("amp", 1.0)
    M = T + 8                                                            # the walk, with margin for the offset
    walk = amp * (rng.standard_normal((B, C, 1)) + 0.3 * np.cumsum(rng.standard_normal((B, C, M)), axis=2))
    t = np.arange(T)
    target = walk[:, :, 4:4 + T]
    pred = np.empty((B, C, T))
    for b in range(B):
        phase = rng.uniform(0, 2 * np.pi)
        d = 1.2 * np.sin(2 * np.pi * t / 45.0 + phase) + 0.4 * np.sin(2 * np.pi * t / 11.0 + 2 * phase)   # frames, |d| < 2
        pos = 4 + t + d
        i0 = np.floor(pos).astype(int)
        lam = pos - i0
        pred[b] = (1 - lam) * walk[b][:, i0] + lam * walk[b][:, i0 + 1]
    pred += 0.05 * rng.standard_normal(pred.shape)
    f16 = lambda x: x.astype(np.float16).astype(np.float32)
    return f16(pred), f16(target)


def expand(pred, s, r, dtype, mistake=None):
    """pred [C, T] -> E [C, s * (T + 2h)]: the padded, interpolated item."""
    C, T = pred.shape
    h = r // 2
    Tp = T + 2 * h
    P = np.zeros((C, Tp), dtype)
    P[:, h:h + T] = pred
    if mistake == "replicate_pad" and h:
        P[:, :h] = pred[:, :1]
        P[:, h + T:] = pred[:, -1:]
    p = np.arange(s * Tp)
    if mistake == "align_corners":
        src = p.astype(np.float64) * ((Tp - 1) / max(s * Tp - 1, 1))
        src = src.astype(dtype)
    elif dtype == np.float32:
        rs = np.float32(1.0 / s)
        src = rs * (p.astype(np.float32) + np.float32(0.5)) - np.float32(0.5)
        src = np.maximum(src, np.float32(0))
    else:
        j, t = p % s, p // s                                             # exact: the fraction depends on p mod s alone
        src = np.maximum((j + 0.5) / s - 0.5 + t, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), Tp - 1)
    i1 = np.minimum(i0 + 1, Tp - 1)
    lam = np.clip(src - i0.astype(dtype), 0, 1).astype(dtype)
    w0 = (dtype(1) - lam).astype(dtype)
    return (w0 * P[:, i0]).astype(dtype) + (lam * P[:, i1]).astype(dtype)


def dtw(pred, target, s, r, dtype=np.float64, lengths=None, mistake=None):
    """pred, target [B, C, T] -> dict(l1 [B, s r + 1, T]: row 0 the unshifted frame, row 1 + j candidate j; choice [B, T]: the winner
    (-1 = unshifted; the first of equal minima, pred before any candidate); out [B, C, T]).  Item b is cut to lengths[b] frames."""
    assert r % 2 == 1
    pred, target = np.asarray(pred, dtype), np.asarray(target, dtype)
    B, C, T = pred.shape
    nc = s * r
    l1 = np.zeros((B, nc + 1, T), dtype)
    choice = np.full((B, T), -1, np.int64)
    out = pred.copy()
    for b in range(B):
        L = T if lengths is None else int(lengths[b])
        E = expand(pred[b, :, :L], s, r, dtype, mistake)
        cands = np.stack([pred[b, :, :L]] + [E[:, j::s][:, :L] for j in range(nc)])                 # [nc + 1, C, L]
        tab = np.abs(cands - target[b, :, :L][None]).astype(dtype).sum(axis=1, dtype=dtype)        # [nc + 1, L]
        l1[b, :, :L] = tab
        best, ch = tab[0].copy(), np.full(L, -1, np.int64)
        order = range(nc - 1, -1, -1) if mistake == "last_first" else range(nc)
        for j in order:
            with np.errstate(invalid="ignore"):
                win = tab[1 + j] <= best if mistake == "le" else tab[1 + j] < best
            best = np.where(win, tab[1 + j], best)
            ch = np.where(win, j, ch)
        choice[b, :L] = ch
        out[b, :, :L] = np.take_along_axis(cands, (ch + 1)[None, None, :], axis=0)[0]
    return {"l1": l1, "choice": choice, "out": out}


def e32_of(pred, s, r):
    """The float32 arm's L-inf distance from the float64 arm over EVERY candidate of every frame (so that it does not depend on which
    one wins): what float32 arithmetic alone moves an output value by."""
    return max(float(np.abs(expand(x.astype(np.float32), s, r, np.float32).astype(np.float64)
                            - expand(x.astype(np.float64), s, r, np.float64)).max()) for x in pred)


# ------------------------------------------------------------------------------------------------ fixtures ----
def pack_delta(x64, ref32):
    """float64 array as a 16-bit delta against a float32 array: (int16 delta, scale) with x64 ~= ref + delta * scale."""
    d = np.asarray(x64, np.float64) - np.asarray(ref32, np.float64)
    scale = float(np.abs(d).max()) / 32767.0 or 1.0
    return np.round(d / scale).astype(np.int16), np.float64(scale)


def unpack_delta(delta16, scale, ref32):
    return np.asarray(ref32, np.float64) + delta16.astype(np.float64) * float(scale)


_CACHE = {}


def load_golden(case):
    """dict(pred, target: float32; ref: the reference's output (float64 array, within 1e-9 of its float32 values); l1_64 [B, s r + 1, T];
    argmin64 [B, T] (-1 = unshifted); e32)."""
    if case not in _CACHE:
        g = np.load(os.path.join(GOLDEN, f"dtw_{case}.npz"))
        c = CASES[case]
        pred, target = g["pred16"].astype(np.float32), g["target16"].astype(np.float32)
        argmin = g["argmin64"].astype(np.int64)
        l1_64 = unpack_delta(g["l1_64_delta16"], g["l1_64_scale"], g["l1_64_f32"])
        # the reference's output is stored against the float64 winner: rebuild that from the inputs and the stored argmin
        win = np.stack([np.take_along_axis(
            np.stack([pred[b].astype(np.float64)] + [expand(pred[b].astype(np.float64), c["s"], c["r"], np.float64)[:, j::c["s"]][:, :c["T"]]
                                                     for j in range(c["s"] * c["r"])]), (argmin[b] + 1)[None, None, :], axis=0)[0]
            for b in range(c["B"])])
        _CACHE[case] = {"pred": pred, "target": target, "ref": unpack_delta(g["ref_delta16"], g["ref_scale"], win), "winner64": win,
                        "l1_64": l1_64, "argmin64": argmin, "e32": float(g["e32"])}
    return _CACHE[case]
