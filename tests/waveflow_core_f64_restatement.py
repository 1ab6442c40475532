"""numpy restatement of the WaveFlow 2-D core (``WaveFlowCoupling`` + ``WN_2d`` of the ``efficient_model_ax.WaveGlow`` family) at a
chosen precision: ``dtype`` = ``np.float64`` (what ``ctts_waveflow_inverse_f32`` / ``ctts_waveflow_inverse_cond_f32`` are judged
against) or ``np.float32`` (the restatement's own rounding, the e32 of every bound).  TEST INFRASTRUCTURE ONLY.

It begins where ``ax_cond_f64_restatement.cond_frames`` ends: the per-flow conditioning at FRAME rate (or, for the folded form, the
mel and the one k=1 cond layer) and the dense, weight-norm-free fp32 weights exactly as ``ctts_waveflow_flow_weights`` takes them.
Written from the model's equations, the lines ``oracle/waveflow_oracle.py:269-377`` follow (gax = glow_ax.py, ax =
efficient_model_ax.py, em = efficient_modules.py), not from the kernels:

  squeeze / un-squeeze     ax:310, 346     a[b, g, l] = z[b, G*l + g]
  early outputs            ax:311-313, 340-341   the LAST split is the initial latent, earlier chunks re-join in front
  un-mix                   em:360-403 (PermuteHeight) / em:271-276 (W^-1 a), before or after the coupling (ax:324-325, 337-338)
  conditioning             gax:545-554     F.interpolate(size=L, 'linear', align_corners=True), then 2C rows per layer (gax:580-592)
  row recurrence           em:42-65        row 0 passes; a[r+1] = (a[r+1] - t) / exp(log_s) with (log_s, t) = WN_2d(rows 0..r)
  WN_2d of one row         gax:556-635     start :558, Conv2d (kh, kw) dilation (dh_i, dw_i), width padding only :518-523 - or
                                           depthwise + pointwise :525-531 -, the row queues :597-602, gated unit :36-198,
                                           res/skip :612-626, end :628
  NaN -> 0                 ax:333-334

Height tap ``ah`` of layer i at row r reads that layer's input of row ``r - (kh-1-ah)*dh_i`` (zeros for rows < 0: the queue starts
zero-filled) at column ``l + (j - kw//2)*dw_i`` (zeros outside [0, L)).

Part of the operation's DEFINITION and therefore fp32 at either ``dtype`` (as ``ax_cond_f64_restatement`` argues): parameters and
inputs, and the interpolation positions (``acr.positions_align_corners``).  Only ``l0*a + l1*b`` and everything behind it run in
``dtype``.

``perturb`` (a set of names) breaks the restatement ON PURPOSE, one mistake each - the tests assert on the reference alone that every
mistake moves the output by far more than the bound on the case that is meant to catch it:
  'tap_row'     a height tap (other than the current row's) reads the row one above the right one
  'first_rows'  rows < 0 read what the ring held from the previous call on the same inputs (the layer's input of the last row)
                instead of zero: a stale slot
  'halo'        the width taps read the edge value instead of zero outside [0, L)
  'lerp_shift'  the conditioning lerp uses align_corners=False positions
  'skip_init'   layer 0's skip rows are added to the previous row's ``out`` instead of starting it
  'end_rows'    log_s and t swapped

``x3=True`` is the split-bf16 variant (CTTS_GEMM_BF16X3): every operand of the in-layer / pointwise / cond-segment / res-skip
products is ``hi = bf16(x), lo = bf16(x - hi)`` and a product is ``hi*hi + hi*lo + lo*hi`` summed in float64; everything else as at
``dtype``.
"""
from __future__ import annotations

import numpy as np

import ax_cond_f64_restatement as acr
from oracle import waveflow_oracle as wf
from oracle.waveglow_oracle import fold_weightnorm
from tacotron_bf16x3_restatement import split

F32 = np.float32
UNITS = ("GTU", "GTRU", "GTLRU", "GLU", "TTU", "STU", "GTSU", "SPTU", "GSIU", "GSIRU", "GTSRU", "GSIRRU", "GSIRLRU", "GSIRRLRU")
PERTURBATIONS = ('tap_row', 'first_rows', 'halo', 'lerp_shift', 'skip_init', 'end_rows')


# ------------------------------------------------------------------------------------------------------- parameters ----
def params(cfg):
    """Reference constructor kwargs -> the core's shape parameters (what ``ctts_waveflow_config`` carries)."""
    wn = cfg["WN_config"]
    n_layers, kh, kw = wn["n_layers"], wn["kernel_size_h"], wn["kernel_size_w"]
    dh, dw = wn.get("n_layers_dilations_h", 1), wn.get("n_layers_dilations_w")
    assert wn.get("res_skip", True), "res_skip=False is not restated"
    return dict(n_flows=cfg["n_flows"], n_group=cfg["n_group"], C=wn["n_channels"], n_layers=n_layers, kh=kh, kw=kw,
                dil_h=[dh] * n_layers if isinstance(dh, int) else list(dh),
                dil_w=[2 ** i for i in range(n_layers)] if dw is None else ([dw] * n_layers if isinstance(dw, int) else list(dw)),
                unit=str(wn.get("gated_unit", 'GTU')).upper(), merge=bool(wn.get("merge_res_skip", False)),
                sep=bool(wn.get("seperable_conv")) and not (kh == 1 and kw == 1),
                conv_mix=cfg.get("channel_mixing", '1x1conv').lower() in "1x1convinvertibleconv1x1invconv",
                mix_first=bool(cfg.get("mix_first", True)),
                n_early_every=cfg.get("n_early_every", 0) or 0, n_early_size=cfg.get("n_early_size", 0))


def active_rows(p):
    """Latent rows each flow runs on (ax:170-189)."""
    n, out = p["n_group"], []
    for k in range(p["n_flows"]):
        if p["n_early_every"] > 0 and k % p["n_early_every"] == 0 and k > 0:
            n -= p["n_early_size"]
        out.append(n)
    return out


def flow_weights(sd, cfg, k, folded=False):
    """Dense fp32 weights of flow k in the layouts of ``ctts_waveflow_flow_weights`` (weight norm folded in fp32)."""
    p = params(cfg)
    pre = f"WN.{k}.WN"

    def w(name):
        if name + ".weight" in sd:
            return np.asarray(sd[name + ".weight"], F32)
        return fold_weightnorm(sd[name + ".weight_g"], sd[name + ".weight_v"]).astype(F32)

    def b(name):
        return np.asarray(sd[name + ".bias"], F32)
    n = range(p["n_layers"])
    out = dict(start_w=w(pre + ".start").reshape(p["C"]), start_b=b(pre + ".start"),
               rs_w=[w(f"{pre}.res_skip_layers.{i}")[:, :, 0, 0] for i in n], rs_b=[b(f"{pre}.res_skip_layers.{i}") for i in n],
               end_w=w(pre + ".end")[:, :, 0, 0], end_b=b(pre + ".end"), w_inverse=None, cond_w=None, cond_b=None)
    if p["sep"]:
        out.update(dw_w=[w(f"{pre}.in_layers.{i}.0")[:, 0] for i in n], dw_b=[b(f"{pre}.in_layers.{i}.0") for i in n],
                   in_w=[w(f"{pre}.in_layers.{i}.1")[:, :, 0, 0] for i in n], in_b=[b(f"{pre}.in_layers.{i}.1") for i in n])
    else:
        out.update(in_w=[w(f"{pre}.in_layers.{i}") for i in n], in_b=[b(f"{pre}.in_layers.{i}") for i in n])
    if p["conv_mix"]:
        out["w_inverse"] = np.linalg.inv(np.asarray(sd[f"convinv.{k}.weight"], F32)[:, :, 0]).astype(F32)
    if folded:
        out["cond_w"], out["cond_b"] = w(pre + ".cond_layers.0")[:, :, 0], b(pre + ".cond_layers.0")
    return {key: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for key, v in out.items()}


# ------------------------------------------------------------------------------------------------------- primitives ----
def gated_unit(name, u, C, dtype):
    """``oracle.waveflow_oracle.gated_unit``'s fourteen definitions (gax:36-198) evaluated in ``dtype``; the constants are the
    fp32 values ATen applies to fp32 tensors."""
    a, b = u[:, :C], u[:, C:]
    c = lambda v: dtype(F32(v))                                                   # noqa: E731
    sig = lambda v: dtype(1) / (dtype(1) + np.exp(-v))                             # noqa: E731
    lrelu = lambda v, s: np.where(v >= 0, v, v * c(s))                             # noqa: E731
    sin16 = lambda v: np.sin(dtype(16) * v)                                        # noqa: E731
    selu = lambda v: c(1.0507009873554805) * (np.maximum(v, 0) + np.minimum(0, c(1.6732632423543772) * np.expm1(v)))   # noqa: E731
    first = {"GLU": lambda v: v, "GTSU": lambda v: v - np.tanh(v), "GTSRU": lambda v: v - np.tanh(v), "GSIU": np.sin,
             "GSIRU": sin16, "GSIRRU": sin16, "GSIRLRU": sin16, "GSIRRLRU": sin16}.get(name, np.tanh)
    second = {"GTRU": lambda v: np.maximum(v, dtype(0)), "GTSRU": lambda v: np.maximum(v, dtype(0)),
              "GSIRRU": lambda v: np.maximum(v, dtype(0)), "GTLRU": lambda v: lrelu(v, 0.01), "GSIRLRU": lambda v: lrelu(v, 0.01),
              "GSIRRLRU": lambda v: lrelu(v, (0.01 + 0.1) / 2), "TTU": np.tanh, "STU": selu,
              "SPTU": lambda v: np.where(v > 20, v, np.log1p(np.exp(np.minimum(v, dtype(20)))))}.get(name, sig)
    assert name in UNITS, name
    with np.errstate(over="ignore"):
        return (first(a) * second(b)).astype(dtype)


def _mm(W, x, x3):
    """W [M, K] times x [B, K, L]; with ``x3`` the three split-bf16 products summed in float64."""
    if not x3:
        return np.matmul(W, x)
    wh, wl = W if isinstance(W, tuple) else split(W)                       # (a weight the caller has split already)
    xh, xl = x if isinstance(x, tuple) else split(x)
    return np.matmul(wh, xh) + np.matmul(wh, xl) + np.matmul(wl, xh)


def _shift(x, s, edge):
    """y[..., l] = x[..., l + s], zeros (or, with ``edge``, the edge value) outside (a split pair: both halves)."""
    if isinstance(x, tuple):
        return tuple(_shift(v, s, edge) for v in x)
    if s == 0:
        return x
    L = x.shape[-1]
    idx = np.arange(L) + s
    y = x[..., np.clip(idx, 0, L - 1)]
    if not edge:
        y = np.where((idx >= 0) & (idx < L), y, x.dtype.type(0))
    return y


def _positions_half_pixel(n_in, n_out):
    """'linear', align_corners=False to a given size, fp32 like ATen: real = max(scale * (n + 0.5) - 0.5, 0), scale = in / out."""
    scale = F32(n_in) / F32(n_out)
    real = np.maximum(scale * (np.arange(n_out, dtype=F32) + F32(0.5)) - F32(0.5), F32(0)).astype(F32)
    return acr._lambdas(real, n_in)


def interp_cond(frames, L, dtype, perturb=()):
    """[B, rows, T] at frame rate -> [B, rows, L] (gax:545-554); T == L is the identity, as in F.interpolate."""
    frames = np.asarray(frames, dtype)
    T = frames.shape[-1]
    if 'lerp_shift' in perturb:
        return acr._lerp(frames, _positions_half_pixel(T, L), dtype)
    if T == L:
        return frames
    return acr.lerp_align_corners(frames, L, dtype)


# ------------------------------------------------------------------------------------------------------- one flow ----
def wn_rows(w, p, a, cond, dtype, perturb=(), x3=False, stale=None, hist_out=None):
    """The coupling inverse of ONE flow on the un-mixed rows a [B, Ga, L] with cond [B, 2C*n_layers, L] -> new rows."""
    B, Ga, L = a.shape
    C, n_layers, kh, kw = p["C"], p["n_layers"], p["kh"], p["kw"]
    edge = 'halo' in perturb
    W = {key: ([np.asarray(v, dtype) for v in val] if isinstance(val, list) else (None if val is None else np.asarray(val, dtype)))
         for key, val in w.items()}
    pre = split if x3 else (lambda m: m)                                   # the GEMM weights, split once
    if p["sep"]:
        in_w = [pre(W["in_w"][i]) for i in range(n_layers)]
    else:
        in_w = [[[pre(np.ascontiguousarray(W["in_w"][i][:, :, ah, j])) for j in range(kw)] for ah in range(kh)] for i in range(n_layers)]
    rs_w = [pre(W["rs_w"][i]) for i in range(n_layers)]
    y = [a[:, 0, :]]
    hist = [[] for _ in range(n_layers)]                       # hist[i][r]: input of layer i at row r (the row queues)
    zeros = np.zeros((B, C, L), dtype)
    out_prev = zeros
    halves = {}
    for r in range(Ga - 1):
        x = W["start_w"][None, :, None] * y[r][:, None, :] + W["start_b"][None, :, None]
        out = None
        for i in range(n_layers):
            dw, dh = p["dil_w"][i], p["dil_h"][i]
            hist[i].append(x)

            def row_of(ah):
                rr = r - (kh - 1 - ah) * dh
                if 'tap_row' in perturb and ah < kh - 1:
                    rr -= 1
                if rr >= 0:
                    return hist[i][rr]
                return stale[i][-1] if ('first_rows' in perturb and stale is not None) else zeros
            bias = W["in_b"][i][None, :, None] + cond[:, 2 * C * i:2 * C * (i + 1), :]
            if p["sep"]:
                d = np.zeros((B, C, L), dtype) + W["dw_b"][i][None, :, None]
                for ah in range(kh):
                    row = row_of(ah)
                    for j in range(kw):
                        d = d + W["dw_w"][i][None, :, ah, j, None] * _shift(row, (j - kw // 2) * dw, edge)
                u = _mm(in_w[i], d, x3) + bias
            else:
                u = bias
                for ah in range(kh):
                    row = row_of(ah)
                    if x3:                                                     # split the row once, not once per width tap
                        if id(row) not in halves:
                            halves[id(row)] = (row, split(row))                # (the array is kept: its id stays unique)
                        row = halves[id(row)][1]
                    for j in range(kw):
                        u = u + _mm(in_w[i][ah][j], _shift(row, (j - kw // 2) * dw, edge), x3)
            act = gated_unit(p["unit"], u.astype(dtype), C, dtype)
            rs = _mm(rs_w[i], act, x3) + W["rs_b"][i][None, :, None]
            if i < n_layers - 1 and not p["merge"]:                                # gax:612-626
                x = (x + rs[:, :C]).astype(dtype)
                skip = rs[:, C:]
            else:
                skip = rs
            if out is None:
                out = (out_prev + skip) if 'skip_init' in perturb else skip
            else:
                out = out + skip
            out = out.astype(dtype)
        out_prev = out
        e = np.matmul(W["end_w"], out) + W["end_b"][None, :, None]
        log_s, t = (e[:, 1, :], e[:, 0, :]) if 'end_rows' in perturb else (e[:, 0, :], e[:, 1, :])
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            y.append(((a[:, r + 1, :] - t) / np.exp(log_s)).astype(dtype))
    if hist_out is not None:
        hist_out.extend(hist)
    a = np.stack(y, axis=1)
    return np.where(np.isnan(a), dtype(0), a).astype(dtype)


def unmix(w, p, k, a, dtype):
    if not p["conv_mix"]:
        return a[:, wf.permutation(k, a.shape[1]), :]
    return np.matmul(np.asarray(w["w_inverse"], dtype), a).astype(dtype)


def flow_cond(w, p, cond_k, mel, L, dtype, perturb=(), x3=False):
    """This flow's [B, 2C*n_layers, L]: the handed-over frames interpolated, or (folded) the k=1 cond layer on the mel, interpolated."""
    if cond_k is not None:
        return interp_cond(cond_k, L, dtype, perturb)
    bias = np.asarray(w["cond_b"], dtype)[None, :, None]
    if x3:                                   # the cond layer is a K segment of the in-layer GEMM there: split operands, on L columns
        return (_mm(np.asarray(w["cond_w"], dtype), interp_cond(mel, L, dtype, perturb), True) + bias).astype(dtype)
    frames = np.matmul(np.asarray(w["cond_w"], dtype), np.asarray(mel, dtype)) + bias
    return interp_cond(frames.astype(dtype), L, dtype, perturb)


def inverse(weights, p, z, cond=None, mel=None, dtype=np.float64, perturb=(), x3=False):
    """z [B, T] fp32, ``cond`` = per flow [B, 2C*n_layers, frames] (or ``mel`` [B, n_mel, frames] with ``cond_w`` / ``cond_b`` in the
    weights) -> audio [B, T] in ``dtype``.  One flow is the plain case; more flows add the early-output re-join."""
    assert dtype in (np.float32, np.float64) and set(perturb) <= set(PERTURBATIONS) and (cond is None) != (mel is None)
    assert not x3 or dtype == np.float64
    z = np.asarray(z, F32)
    G, n_flows = p["n_group"], p["n_flows"]
    B, T = z.shape
    L = T // G
    a = np.ascontiguousarray(z.reshape(B, L, G).transpose(0, 2, 1)).astype(dtype)
    n_rem = active_rows(p)
    n_early = (G - n_rem[-1]) // p["n_early_size"] if n_rem[-1] != G else 0
    remained = [a[:, i * p["n_early_size"]:(i + 1) * p["n_early_size"]] for i in range(n_early)]
    a = a[:, G - n_rem[-1]:]
    for k in reversed(range(n_flows)):
        w = weights[k]
        assert a.shape[1] == n_rem[k]
        if not p["mix_first"]:
            a = unmix(w, p, k, a, dtype)
        c = flow_cond(w, p, None if cond is None else cond[k], mel, L, dtype, perturb, x3)
        stale = None
        if 'first_rows' in perturb:
            stale = []
            wn_rows(w, p, a, c, dtype, (), x3, hist_out=stale)
        a = wn_rows(w, p, a, c, dtype, perturb, x3, stale)
        if p["mix_first"]:
            a = unmix(w, p, k, a, dtype)
        if k > 0 and n_rem[k - 1] > n_rem[k]:
            a = np.concatenate([remained.pop(), a], axis=1)
    assert not remained
    return np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(B, T)


# ------------------------------------------------------------------------------------------------------- the bound ----
def rows_of(audio, G):
    """audio [B, T] -> the latent rows [B, G, L] it un-squeezes from."""
    audio = np.asarray(audio)
    B, T = audio.shape
    return audio.reshape(B, T // G, G).transpose(0, 2, 1)


def row_bounds(y32, y64, G, factor=acr.FACTOR, y_x3=None):
    """Per latent row r over all items and columns: (e_r, bound_r) with bound_r = factor * max(e_r, 4 * 2^-23 * max|y64_r|).
    e_r is the L-inf distance of the restatement's fp32 run from its float64 run - with ``y_x3`` the split-bf16 variant's
    distance, floored by the fp32 one."""
    r64 = rows_of(np.asarray(y64, np.float64), G)
    e = np.abs(rows_of(np.asarray(y32, np.float64), G) - r64).max(axis=(0, 2))
    if y_x3 is not None:
        e = np.maximum(e, np.abs(rows_of(np.asarray(y_x3, np.float64), G) - r64).max(axis=(0, 2)))
    floor = 4 * acr.EPS32 * np.abs(r64).max(axis=(0, 2))
    return e, factor * np.maximum(e, floor)


def worst(got, ref, G):
    """Where the largest deviation of got from ref (both [B, T]) sits: item, latent row, column, the column's distance to either end
    and the column modulo the tile widths."""
    err = np.abs(rows_of(np.asarray(got, np.float64), G) - rows_of(np.asarray(ref, np.float64), G))
    err = np.where(np.isnan(err), np.inf, err)
    b, r, c = np.unravel_index(int(np.argmax(err)), err.shape)
    L = err.shape[2]
    return (f"worst |err| {err[b, r, c]:.3e} at (item {b}, row {r}, column {c}); {c} from the start, {L - 1 - c} from the end; "
            f"column mod 64 / 128 / 256: {c % 64} / {c % 128} / {c % 256}")
