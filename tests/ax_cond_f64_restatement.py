"""numpy restatement of the conditioning path of the ``efficient_model_ax.WaveGlow`` family (WaveFlow 2-D core and the 1-D ax
core) at a chosen precision: ``dtype`` = ``np.float64`` (what the HIP path is judged against) or ``np.float32`` (the
restatement's own rounding, the e32 of every bound).  TEST INFRASTRUCTURE ONLY.

Written from the reference's model code, the lines ``oracle/waveflow_oracle.py`` follows (paths relative to
CookieTTS/_4_mtw/waveglow/; ax = efficient_model_ax.py, gax = glow_ax.py):

  model_cond               ax:280-307   shift :280-281, scale :282-283, speaker rows :286-291, conv stack with the activation
                                        after EVERY layer :293-297, rezero alpha :299-300, residual (1x1 conv :303-304) :302-307
  activation names         ax:100-111 = gax:493-504: 'lrelu' selects F.relu, 'relu' selects LeakyReLU(negative_slope) (as written)
  transposed_upsample_net  gax:201-242  ConvTranspose1d(stride = scale, padding = (k - scale) // 2) :220, LeakyReLU(0.4) :224-225,
                                        residual F.interpolate(scale_factor, 'linear' | 'nearest', align_corners=False) :229-231,
                                        ``x *= res_weight`` on ALL channels :239-240, residual on the first min(in, out) :241
  to_latent_length         ax:174-182 = gax:365-373 (1-D: ``[pad_l : -pad_r]``), gax:548-553 (WN_2d: ``[pad : -(pad + pad % 2)]``);
                                        F.interpolate(size, 'linear', align_corners=True) when the net's factor is not
                                        hop // n_group and the lengths differ (ax:117-125, gax:288-295 / 463-470)
  flow_conds               ax:131-134, 316-317  n_flow_group_conv(cond).chunk(n_flows, dim=1)
  wn_stage                 gax:378-390 / 566-578  WN speaker rows, cond stack, activation after the last layer only with
                                        cond_out_activation_func, the WN's own TransposedUpsampleNet (upsample_first is False)

What is part of the operation's DEFINITION and therefore fp32 at either ``dtype``: the parameters and inputs (fp32 data, cast up),
the scalars the reference applies to fp32 tensors (shift_spect, scale_spect, the LeakyReLU slopes: ATen casts them to the
tensor's type), and the interpolation positions - ATen computes ``scale``, ``real``, ``i0``, ``i1``, ``l1``, ``l0`` (and
``floor(n * (1 / scale))`` for 'nearest') in fp32 for fp32 tensors (UpSample.h: compute_scales_value, area_pixel_compute_scale,
area_pixel_compute_source_index, compute_source_index_and_lambda, nearest_idx).  Only the combination ``l0 * a + l1 * b`` and
every convolution / sum run in ``dtype``.

Two places where the reference's slice arithmetic cannot be followed to the letter, both outside what a running model reaches:
  * a crop by zero columns: ``cond[:, :, 0:-0]`` is EMPTY in Python and the reference's next addition fails; here (as in the
    oracle) it is the identity - the only reading that keeps the length;
  * ``pad_r = -(audio_len-cond_len)//2`` (ax:180) is ``(cond_len - audio_len) // 2`` = pad_l (unary minus binds first): an odd
    difference leaves one column too many and the reference fails; ``to_latent_length`` asserts the length instead.

``cond_frames`` returns what ``WaveGlow._cond_frames`` hands to the cores: per flow ``[B][2C*n_layers][T]`` and T - at the
latent's rate with a model- or WN-level TransposedUpsampleNet, else at frame rate (the cores interpolate inside the library; that
lerp has no stage entry and is not restated here).

``perturb`` (a set of names) breaks the restatement ON PURPOSE, one mistake each - the tests assert on the reference alone that
every mistake they are meant to catch moves the output by far more than the bound:
  'crop_shift'   the centre crop starts one column late
  'last_frame'   the last input frame is zero when the transposed convs read it
  'group_slice'  flow 1 of the grouped per-flow conv reads flow 0's input slice
(a wrong speaker row and a wrong padding mode need no hook: they are other ``speaker_ids`` / another ``cfg``).
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
FACTOR = 8          # the project's factor on e32 (waveglow_f64_restatement.FACTOR, test_tacotron_text_side.FACTOR)
EPS32 = 2.0 ** -23


# ------------------------------------------------------------------------------------------------------- parameters ----
def fold_weightnorm(g, v, dtype):
    """torch.nn.utils.weight_norm: w = v * (g / ||v||), the norm over every dim but 0."""
    v = np.asarray(v, dtype=dtype)
    g = np.asarray(g, dtype=dtype).reshape(-1)
    norm = np.sqrt(np.sum((v * v).reshape(v.shape[0], -1), axis=1, dtype=dtype))
    return (v * (g / norm).reshape((-1,) + (1,) * (v.ndim - 1))).astype(dtype)


def _w(sd, prefix, dtype):
    if prefix + ".weight" in sd:
        return np.asarray(sd[prefix + ".weight"], dtype=dtype)
    return fold_weightnorm(sd[prefix + ".weight_g"], sd[prefix + ".weight_v"], dtype)


def _p(sd, key, dtype):
    return np.asarray(sd[key], dtype=dtype)


def _scalar(value, dtype):
    """A Python scalar the reference applies to an fp32 tensor: fp32 first (ATen casts it), then ``dtype``."""
    return dtype(F32(value))


def activation(name, negative_slope, dtype):
    """ax:100-111 = gax:493-504, the swapped 'relu' / 'lrelu' included."""
    name = (name or 'none').lower()
    if name == 'none':
        return None
    if name == 'lrelu':
        return lambda x: np.maximum(x, dtype(0))
    if name == 'relu':
        slope = _scalar(negative_slope, dtype)
        return lambda x: np.where(x >= 0, x, x * slope).astype(dtype)
    if name == 'tanh':
        return lambda x: np.tanh(x).astype(dtype)
    if name == 'sigmoid':
        return lambda x: (dtype(1) / (dtype(1) + np.exp(-x))).astype(dtype)
    raise NotImplementedError(name)


# ------------------------------------------------------------------------------------------------------ convolutions ----
def conv1d_same(x, w, b, padding_mode, dtype):
    """nn.Conv1d, odd kernel, padding (k - 1) / 2 with zeros or edge values: x [B, Cin, T], w [Cout, Cin, k] -> [B, Cout, T]."""
    x = np.asarray(x, dtype=dtype)
    k, T, h = w.shape[2], x.shape[2], w.shape[2] // 2
    assert k % 2 == 1 and padding_mode in ('zeros', 'replicate'), (k, padding_mode)
    xp = np.pad(x, ((0, 0), (0, 0), (h, h)), mode='edge' if padding_mode == 'replicate' else 'constant')
    y = np.zeros((x.shape[0], w.shape[0], T), dtype) + np.asarray(b, dtype)[None, :, None]
    for j in range(k):
        y = y + np.matmul(np.ascontiguousarray(w[:, :, j]), xp[:, :, j:j + T])
    return y.astype(dtype)


def conv_transpose1d(x, w, b, stride, padding, dtype):
    """nn.ConvTranspose1d: x [B, Cin, T], w [Cin, Cout, k] -> [B, Cout, (T - 1) * stride - 2 * padding + k]:
    out[n] = b + sum over (t, j) with t * stride - padding + j == n of w[:, :, j]^T x[:, t]."""
    x = np.asarray(x, dtype=dtype)
    B, _, T = x.shape
    k = w.shape[2]
    full = np.zeros((B, w.shape[1], (T - 1) * stride + k), dtype)
    for j in range(k):
        full[:, :, j:j + (T - 1) * stride + 1:stride] += np.matmul(np.ascontiguousarray(w[:, :, j].T), x)
    return (full[:, :, padding:full.shape[2] - padding] + np.asarray(b, dtype)[None, :, None]).astype(dtype)


# ---------------------------------------------------------------------------------------------------- interpolation ----
def positions_align_corners(n_in, n_out):
    """'linear', align_corners=True to a given size -> (i0, i1, l0, l1), all in fp32 like ATen: scale = (in - 1) / (out - 1)
    (0 for out == 1), real = scale * n, i0 = int(real), i1 = i0 + (i0 < in - 1), l1 = real - i0, l0 = 1 - l1."""
    scale = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
    real = (scale * np.arange(n_out, dtype=F32)).astype(F32)
    return _lambdas(real, n_in)


def positions_linear_scale(n_in, scale_factor):
    """'linear', align_corners=False with a scale factor: out = floor(in * scale), s = float(1 / scale),
    real = max(s * (n + 0.5) - 0.5, 0) with ``s * (n + 0.5) - 0.5`` as ONE fused multiply-add: ATen's builds contract the
    expression (its CPU kernel hands out weights that only the fused form gives, pinned by the one-hot probes of
    test_ax_cond_frames.py; device compilers contract by default as well).  The fp32 product of two fp32 numbers and the
    subtraction of 0.5 are exact in double at these sizes (< 53 bits between the first and the last set bit), so one rounding
    of the double result to fp32 IS the fused operation."""
    n_out = int(np.floor(float(n_in) * float(scale_factor)))
    s = F32(1.0 / float(scale_factor))
    half = (np.arange(n_out, dtype=F32) + F32(0.5)).astype(F32)
    fused = (np.float64(s) * half.astype(np.float64) - 0.5).astype(F32)
    return _lambdas(np.maximum(fused, F32(0)).astype(F32), n_in)


def _lambdas(real, n_in):
    i0 = real.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (real - i0.astype(F32)).astype(F32)
    l0 = (F32(1) - l1).astype(F32)
    return i0, i1, l0, l1


def positions_nearest_scale(n_in, scale_factor):
    """'nearest' with a scale factor: out = floor(in * scale), index = min(floor(n * float(1 / scale)), in - 1) in fp32."""
    n_out = int(np.floor(float(n_in) * float(scale_factor)))
    s = F32(1.0 / float(scale_factor))
    return np.minimum(np.floor((np.arange(n_out, dtype=F32) * s).astype(F32)).astype(np.int64), n_in - 1)


def _lerp(x, pos, dtype):
    i0, i1, l0, l1 = pos
    x = np.asarray(x, dtype=dtype)
    return (l0.astype(dtype) * x[..., i0] + l1.astype(dtype) * x[..., i1]).astype(dtype)


def lerp_align_corners(x, n_out, dtype):
    """F.interpolate(x, size=n_out, mode='linear', align_corners=True) on the last axis."""
    return _lerp(x, positions_align_corners(x.shape[-1], n_out), dtype)


def interp_scale(x, scale_factor, linear, dtype):
    """F.interpolate(x, scale_factor=..., mode='linear' (align_corners=False) | 'nearest') on the last axis."""
    if linear:
        return _lerp(x, positions_linear_scale(x.shape[-1], scale_factor), dtype)
    return np.asarray(x, dtype=dtype)[..., positions_nearest_scale(x.shape[-1], scale_factor)]


# ------------------------------------------------------------------------------------------------------- the stages ----
def model_cond(sd, cfg, mel, speaker_ids, dtype):
    """ax:280-307 -> [B, c, frames]: what the flows share at frame rate."""
    cond = np.asarray(mel, dtype=dtype)
    if cfg.get("shift_spect", 0.) != 0.:
        cond = cond + _scalar(cfg["shift_spect"], dtype)
    if cfg.get("scale_spect", 1.) != 1.:
        cond = cond * _scalar(cfg["scale_spect"], dtype)
    if cfg["speaker_embed"]:
        emb = _p(sd, "speaker_embed.weight", dtype)[np.asarray(speaker_ids)]
        cond = np.concatenate([cond, np.repeat(emb[:, :, None], cond.shape[2], axis=2)], axis=1)
    cond = cond.astype(dtype)
    if not cfg["cond_layers"]:
        return cond                                                             # empty ModuleList: cond_res is cond
    act = activation(cfg.get("cond_activation_func", 'none'), cfg.get("negative_slope"), dtype)
    res = cond
    for l in range(cfg["cond_layers"]):
        res = conv1d_same(res, _w(sd, f"cond_layers.{l}", dtype), sd[f"cond_layers.{l}.bias"],
                          cfg.get("cond_padding_mode", 'zeros'), dtype)
        if act is not None:
            res = act(res)
    if "alpha" in sd:
        res = res * _p(sd, "alpha", dtype)[0]
    if not cfg["cond_residual"]:
        return res.astype(dtype)
    if "res_conv.weight" in sd:
        cond = np.matmul(_p(sd, "res_conv.weight", dtype)[:, :, 0], cond) + _p(sd, "res_conv.bias", dtype)[None, :, None]
    return (cond + res).astype(dtype)


def transposed_upsample_net(sd, prefix, x, scales, kernel_size, last_act, residual, residual_linear, dtype, perturb=()):
    """gax:228-242 (TransposedUpsampleNet.forward)."""
    x = np.asarray(x, dtype=dtype)
    xi = interp_scale(x, int(np.prod(scales)), residual_linear, dtype) if residual else None
    if 'last_frame' in perturb:
        x = x.copy()
        x[:, :, -1] = 0
    idx = 0
    for i, sc in enumerate(scales):
        k = kernel_size[i] if isinstance(kernel_size, (list, tuple)) else kernel_size
        x = conv_transpose1d(x, _p(sd, f"{prefix}.t_convs.{idx}.weight", dtype), sd[f"{prefix}.t_convs.{idx}.bias"], sc,
                             (k - sc) // 2, dtype)
        idx += 1
        if i + 1 < len(scales) or last_act:
            x = np.where(x >= 0, x, x * _scalar(0.4, dtype)).astype(dtype)
            idx += 1                                                            # the LeakyReLU module's slot in t_convs
    if residual:
        if f"{prefix}.res_weight" in sd:
            x = x * _p(sd, f"{prefix}.res_weight", dtype)[0]
        r = min(xi.shape[1], x.shape[1])
        x[:, :r] = x[:, :r] + xi[:, :r]
    return x.astype(dtype)


def to_latent_length(cond, L, interpolation_required, two_d, dtype, perturb=()):
    """The tail of ``_upsample_mels``: interpolate (align_corners=True) or centre-crop to the latent's L columns."""
    n = cond.shape[2]
    if interpolation_required and n != L:
        return lerp_align_corners(cond, L, dtype)
    if n == L:
        return np.asarray(cond, dtype=dtype)                                    # see the module docstring: [0:-0]
    if two_d:
        pad = (n - L) // 2
        lo, hi = pad, pad + pad % 2
    else:
        lo, hi = (n - L) // 2, (-(L - n)) // 2
    if 'crop_shift' in perturb:
        lo, hi = lo + 1, hi - 1
    out = np.asarray(cond, dtype=dtype)[:, :, lo:n - hi]
    assert out.shape[2] == L, f"a crop of {n} columns by ({lo}, {hi}) does not give {L}: the reference fails here as well"
    return np.ascontiguousarray(out)


def flow_conds(sd, cfg, cond, dtype, perturb=()):
    """ax:316-317: per-flow chunks of the (grouped) 1x1 conv, or the same tensor for every flow."""
    n_flows = cfg["n_flows"]
    if "n_flow_group_conv.weight" not in sd:
        return [cond] * n_flows
    w = _p(sd, "n_flow_group_conv.weight", dtype)[:, :, 0]                       # [out * n_flows, cin / groups]
    b = _p(sd, "n_flow_group_conv.bias", dtype)
    out, cin = w.shape[0] // n_flows, w.shape[1]
    grouped = cin != cond.shape[1]
    assert not grouped or cin * n_flows == cond.shape[1]
    res = []
    for k in range(n_flows):
        src = 0 if ('group_slice' in perturb and k == 1) else k
        x = cond[:, src * cin:(src + 1) * cin] if grouped else cond
        res.append((np.matmul(w[k * out:(k + 1) * out], x) + b[None, k * out:(k + 1) * out, None]).astype(dtype))
    return res


def wn_stage(sd, cfg, k, spect, speaker_ids, L, two_d, dtype, perturb=()):
    """gax:378-390 / 566-578 of flow k -> ([B, 2C*n_layers, T], T)."""
    wn = cfg["WN_config"]
    p = f"WN.{k}.WN"
    spect = np.asarray(spect, dtype=dtype)
    if wn.get("speaker_embed_dim", 0):
        emb = _p(sd, p + ".speaker_embed.weight", dtype)[np.asarray(speaker_ids)]
        spect = np.concatenate([spect, np.repeat(emb[:, :, None], spect.shape[2], axis=2)], axis=1)
    act = activation(wn.get("cond_activation_func", 'none'), wn.get("negative_slope"), dtype)
    for l in range(wn["cond_layers"]):
        spect = conv1d_same(spect, _w(sd, f"{p}.cond_layers.{l}", dtype), sd[f"{p}.cond_layers.{l}.bias"],
                            wn.get("cond_padding_mode", 'zeros'), dtype)
        if act is not None and (wn.get("cond_out_activation_func", True) or l != wn["cond_layers"] - 1):
            spect = act(spect)
    if cfg.get("upsample_first") is not True and f"{p}.upsample_net.t_convs.0.weight" in sd:
        scales = wn["transposed_conv_scales"]
        spect = transposed_upsample_net(sd, p + ".upsample_net", spect, scales, wn.get("transposed_conv_kernel_size", 4), False,
                                        False, False, dtype, perturb)
        required = int(np.prod(scales)) != cfg["hop_length"] // cfg["n_group"]
        spect = to_latent_length(spect, L, required, two_d, dtype, perturb)
    return spect.astype(dtype), spect.shape[2]


def shared_cond(sd, cfg, mel, speaker_ids, L, dtype, perturb=()):
    """Everything in front of the per-flow stage: model_cond, then the model-level net and the way to L columns (ax:313-314;
    ``efficient_model_ax._upsample_mels`` is the 1-D rule for both cores)."""
    cond = model_cond(sd, cfg, mel, speaker_ids, dtype)
    if cfg.get("upsample_first") is True:
        scales = cfg["transposed_conv_scales"]
        cond = transposed_upsample_net(sd, "upsample_net", cond, scales, cfg["transposed_conv_kernel_size"], True,
                                       cfg.get("transposed_conv_residual", False),
                                       cfg.get("transposed_conv_residual_linear", False), dtype, perturb)
        cond = to_latent_length(cond, L, int(np.prod(scales)) != cfg["hop_length"] // cfg["n_group"], False, dtype, perturb)
    return cond


def cond_frames(sd, cfg, mel, speaker_ids, L, dtype, perturb=()):
    """-> ([n_flows] of [B, 2C*n_layers, T], T): what ``WaveGlow._cond_frames(ops, mel, ids, stream, out_steps=L)`` returns in
    its valid columns."""
    assert dtype in (np.float32, np.float64)
    cond = shared_cond(sd, cfg, mel, speaker_ids, L, dtype, perturb)
    per_flow = flow_conds(sd, cfg, cond, dtype, perturb)
    two_d = bool(cfg.get("waveflow", True))
    out = [wn_stage(sd, cfg, k, per_flow[k], speaker_ids, L, two_d, dtype, perturb) for k in range(cfg["n_flows"])]
    T = out[0][1]
    assert all(t == T for _, t in out)
    return [y for y, _ in out], T


# ------------------------------------------------------------------------------------------------ the small kernels ----
def vol_unscale(x, dtype):
    """ax:342-344: x > 0 -> 10 ** log2(x), x < 0 -> -(10 ** log2(-x)), everything else (0, NaN) as it is."""
    x = np.asarray(x, dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        pos = np.power(dtype(10), np.log2(np.where(x > 0, x, dtype(1)))).astype(dtype)
        neg = -np.power(dtype(10), np.log2(np.where(x < 0, -x, dtype(1)))).astype(dtype)
    return np.where(x > 0, pos, np.where(x < 0, neg, x)).astype(dtype)


def deemphasis64(x, p):
    """ax:351-355: scipy.signal.lfilter([1], [1, -p]) in float64, y[n] = x[n] + p * y[n - 1]."""
    x = np.asarray(x, dtype=np.float64)
    y = np.empty_like(x)
    acc = np.zeros(x.shape[:-1], np.float64)
    for n in range(x.shape[-1]):
        acc = x[..., n] + float(p) * acc
        y[..., n] = acc
    return y


def bound(y32, y64, factor=FACTOR):
    """(e32, bound) of one comparison against float64: max(factor * e32, 4 * 2^-23 * max|y64|)."""
    y64 = np.asarray(y64, np.float64)
    e32 = float(np.abs(np.asarray(y32, np.float64) - y64).max()) if y64.size else 0.0
    return e32, max(factor * e32, 4 * EPS32 * float(np.abs(y64).max()))


def worst(got, ref, flow=None):
    """Where the largest deviation of got from ref [B, rows, T] sits, in words."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    err = np.where(np.isnan(err), np.inf, err)
    b, r, c = np.unravel_index(int(np.argmax(err)), err.shape)
    T = err.shape[2]
    head = "" if flow is None else f"flow {flow}, "
    return (f"worst |err| {err[b, r, c]:.3e} at ({head}item {b}, row {r}, column {c}); {c} from the start, {T - 1 - c} from the "
            f"end; got {np.asarray(got)[b, r, c]!r}, want {ref[b, r, c]!r}")
