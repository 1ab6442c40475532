"""numpy restatement of the ANALYSIS direction of the WaveFlow model (``efficient_model_ax.WaveGlow.forward`` with ``waveflow=True``,
ax:184-277) at a chosen precision: ``dtype`` = ``np.float64`` (what ``ctts_waveflow_forward_f32`` / ``_cond_f32`` are judged against)
or ``np.float32`` (the restatement's own rounding: the e32 of every bound).  TEST INFRASTRUCTURE ONLY.

Written from the model's equations on the helpers of ``waveflow_core_f64_restatement`` (``params``, ``flow_weights``, ``gated_unit``,
``_shift``, ``flow_cond``, ``active_rows``) and ``ax_cond_f64_restatement.cond_frames``, not from the kernels:

  pre-emphasis     efficient_loss.py:16-20   y[t] = x[t] - p x[t-1], reflected at t = 0: y[0] = x[0] - p x[1]
  squeeze          ax:225                    a[b, g, l] = y[b, G*l + g]
  early split      ax:237-242                at k % n_early_every == 0, k > 0 the first n_early_size active rows leave to the output
  mix              em:258-267 (W a) / em:360-403 (PermuteHeight), before (mix_first) or after the coupling
  coupling         em:28-40                  row 0 passes; (log_s_r, t_r) = end(WN_2d(rows 0 .. Ga-2)); out[r+1] = a[r+1] exp(log_s_r) + t_r
  WN_2d, no queues gax:556-635               causal height padding (gax:595): tap ah of layer i at row r reads row r - (kh-1-ah) dh_i
  NaN -> 0         ax:253-254
  outputs          ax:266-277                z = cat(early outputs in peel order, rest) un-squeezed; logdet, logdet_w_sum, log_s_sum

``perturb`` breaks the restatement ON PURPOSE, one mistake each:
  'row_shift'      the WN is fed rows 1 .. instead of 0 .. Ga-2
  'affine_dir'     divide instead of multiply
  'mix_transpose'  W^T instead of W
  'early_order'    the early chunks are emitted last-first
  'tap_row', 'halo'   as in the core restatement
  'preemph_edge'   zero instead of the reflection at t = 0
"""
from __future__ import annotations

import os

import numpy as np

import ax_cond_f64_restatement as acr
import waveflow_core_f64_restatement as wcr
from cookietts_amd import synthetic
from oracle import waveflow_oracle as wf

F32 = np.float32
PERTURBATIONS = ('row_shift', 'affine_dir', 'mix_transpose', 'early_order', 'tap_row', 'halo', 'preemph_edge')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# fixture name -> the infer fixture (tests/golden/waveflow_<name>.npz) whose mel, ``inverse_full`` and seed it is made of
CASES = ("toy", "toy_odd", "toy_dilations_h", "toy_merge", "toy_conv_early", "toy_permute_mixfirst_early", "toy_conv_mixlast",
         "full_short", "author_toy", "table_g50_c128", "toy_no_res_skip", "toy_upsample_first")
# the seven cases on which the reference's own forward was seen to return the fixture's z from inverse_full (no pre-emphasis)
RECOVERS_Z = CASES[:7]


def active_rows(cfg):
    """Latent rows each flow runs on (ax:170-189), from the constructor kwargs."""
    return wcr.active_rows(dict(n_group=cfg["n_group"], n_flows=cfg["n_flows"], n_early_every=cfg.get("n_early_every", 0) or 0,
                                n_early_size=cfg.get("n_early_size", 0)))


def case_path(name):
    return os.path.join(GOLDEN, f"waveflow_forward_{name}.npz")


def case_inputs(name):
    """-> (cfg, sd, mel padded by one zero frame as ``infer`` pads it, audio = the fixture's ``inverse_full``, speaker ids, sigma, z)."""
    g = np.load(os.path.join(GOLDEN, f"waveflow_{name}.npz"))
    cfg = synthetic.WAVEFLOW_CONFIGS[str(g["config_key"])]
    sd = synthetic.waveflow_state_dict(cfg, seed=int(g["seed"]))
    ids = g["speaker_ids"] if "speaker_ids" in g.files else None
    melp = np.pad(g["mel"], ((0, 0), (0, 0), (0, 1))).astype(F32)
    return cfg, sd, melp, np.asarray(g["inverse_full"], F32), ids, float(g["sigma"]), np.asarray(g["z"], F32)


def _weights(sd, cfg):
    """``flow_weights`` of every flow + the forward mixing matrix W_k; ``res_skip=False`` as identity res/skip layers with merge."""
    wn = cfg["WN_config"]
    if not wn.get("res_skip", True):
        cfg = dict(cfg, WN_config=dict(wn, res_skip=True, merge_res_skip=True))
        C = wn["n_channels"]
        sd = dict(sd)
        for k in range(cfg["n_flows"]):
            for i in range(wn["n_layers"]):
                sd[f"WN.{k}.WN.res_skip_layers.{i}.weight"] = np.eye(C, dtype=F32)[:, :, None, None]
                sd[f"WN.{k}.WN.res_skip_layers.{i}.bias"] = np.zeros(C, F32)
    p = wcr.params(cfg)
    weights = [wcr.flow_weights(sd, cfg, k) for k in range(p["n_flows"])]
    if p["conv_mix"]:
        for k, w in enumerate(weights):
            w["w_forward"] = np.ascontiguousarray(np.asarray(sd[f"convinv.{k}.weight"], F32)[:, :, 0])
    return p, weights


def preemphasis(x, coef, dtype, perturb=()):
    x = np.asarray(x, F32).astype(dtype)
    prev = np.concatenate([np.zeros_like(x[:, :1]) if 'preemph_edge' in perturb else x[:, 1:2], x[:, :-1]], axis=1)
    return (x - dtype(F32(coef)) * prev).astype(dtype)


def mix(w, p, k, a, dtype, perturb=()):
    if not p["conv_mix"]:
        return a[:, wf.permutation(k, a.shape[1]), :]
    W = np.asarray(w["w_forward"], dtype)
    return np.matmul(W.T if 'mix_transpose' in perturb else W, a).astype(dtype)


def coupling(w, p, a, cond, dtype, perturb=()):
    """One flow's coupling on the rows a [B, Ga, L] with cond [B, 2C*n_layers, L] -> (new rows, log_s [B, Ga-1, L])."""
    B, Ga, L = a.shape
    C, n_layers, kh, kw = p["C"], p["n_layers"], p["kh"], p["kw"]
    edge = 'halo' in perturb
    W = {key: ([np.asarray(v, dtype) for v in val] if isinstance(val, list) else (None if val is None else np.asarray(val, dtype)))
         for key, val in w.items()}
    zeros = np.zeros((B, C, L), dtype)
    src = a[:, 1:] if 'row_shift' in perturb else a[:, :-1]                # the WN's input rows (em:30)
    hist = [[] for _ in range(n_layers)]                                   # hist[i][r]: input of layer i at row r
    y, log_s_rows = [a[:, 0, :]], []
    for r in range(Ga - 1):
        x = W["start_w"][None, :, None] * src[:, r, None, :] + W["start_b"][None, :, None]
        out = None
        for i in range(n_layers):
            dw, dh = p["dil_w"][i], p["dil_h"][i]
            hist[i].append(x)

            def row_of(ah):
                rr = r - (kh - 1 - ah) * dh
                if 'tap_row' in perturb and ah < kh - 1:
                    rr -= 1
                return hist[i][rr] if rr >= 0 else zeros
            bias = W["in_b"][i][None, :, None] + cond[:, 2 * C * i:2 * C * (i + 1), :]
            if p["sep"]:
                d = np.zeros((B, C, L), dtype) + W["dw_b"][i][None, :, None]
                for ah in range(kh):
                    row = row_of(ah)
                    for j in range(kw):
                        d = d + W["dw_w"][i][None, :, ah, j, None] * wcr._shift(row, (j - kw // 2) * dw, edge)
                u = np.matmul(W["in_w"][i], d) + bias
            else:
                u = bias
                for ah in range(kh):
                    row = row_of(ah)
                    for j in range(kw):
                        u = u + np.matmul(W["in_w"][i][:, :, ah, j], wcr._shift(row, (j - kw // 2) * dw, edge))
            act = wcr.gated_unit(p["unit"], u.astype(dtype), C, dtype)
            rs = np.matmul(W["rs_w"][i], act) + W["rs_b"][i][None, :, None]
            if i < n_layers - 1 and not p["merge"]:                                # gax:612-626
                x = (x + rs[:, :C]).astype(dtype)
                skip = rs[:, C:]
            else:
                skip = rs
            out = (skip if out is None else out + skip).astype(dtype)
        e = np.matmul(W["end_w"], out) + W["end_b"][None, :, None]
        log_s, t = e[:, 0, :].astype(dtype), e[:, 1, :].astype(dtype)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            if 'affine_dir' in perturb:
                y.append((a[:, r + 1, :] / np.exp(log_s) + t).astype(dtype))
            else:
                y.append((a[:, r + 1, :] * np.exp(log_s) + t).astype(dtype))
        log_s_rows.append(log_s)
    return np.stack(y, axis=1).astype(dtype), np.stack(log_s_rows, axis=1).astype(dtype)


def log_det_W(p, weights, L, dtype=np.float64):
    """log_det_W_k as the reference defines it: ``L * slogdet(W_k)[1]`` (em:265) or PermuteHeight's ``L * const``, sigma = 1 (em:384)."""
    if p["conv_mix"]:
        return np.array([L * np.linalg.slogdet(np.asarray(w["w_forward"], np.float64))[1] for w in weights], dtype)
    const = -(0.5 * np.log(2 * np.pi) + np.log(1.0)) / p["n_flows"]
    return np.array([L * const] * p["n_flows"], dtype)


def forward(sd, cfg, melp, audio, ids=None, dtype=np.float64, perturb=(), ignore_nan=True):
    """-> dict(z [B, T], log_s [B, S, L], log_s_sum [B, L], sums [B, n_flows], logdet_w [n_flows], logdet [B]) in ``dtype``."""
    assert dtype in (np.float32, np.float64) and set(perturb) <= set(PERTURBATIONS)
    p, weights = _weights(sd, cfg)
    G, n_flows = p["n_group"], p["n_flows"]
    audio = np.asarray(audio, F32)
    B, T = audio.shape
    L = T // G
    x = preemphasis(audio, cfg["preempthasis"], dtype, perturb) if cfg.get("preempthasis") else audio.astype(dtype)
    a = np.ascontiguousarray(x.reshape(B, L, G).transpose(0, 2, 1))
    frames, _ = acr.cond_frames(sd, cfg, melp, ids, L, dtype)
    n_rem = wcr.active_rows(p)
    early, log_s_all, sums = [], [], []
    core_perturb = tuple(h for h in perturb if h in ('tap_row', 'halo'))
    for k in range(n_flows):
        w = weights[k]
        if a.shape[1] > n_rem[k]:
            es = a.shape[1] - n_rem[k]
            early.append(a[:, :es])
            a = a[:, es:]
        if p["mix_first"]:
            a = mix(w, p, k, a, dtype, perturb)
        c = wcr.flow_cond(w, p, frames[k], None, L, dtype, core_perturb)
        a, log_s = coupling(w, p, a, c, dtype, perturb)
        if ignore_nan:
            a = np.where(np.isnan(a), dtype(0), a).astype(dtype)
        if not p["mix_first"]:
            a = mix(w, p, k, a, dtype, perturb)
        log_s_all.append(log_s)
        sums.append(log_s.sum(axis=(1, 2), dtype=dtype))
    if 'early_order' in perturb:
        early = early[::-1]
    rows = np.concatenate(early + [a], axis=1)
    z = np.ascontiguousarray(rows.transpose(0, 2, 1)).reshape(B, T).astype(dtype)
    ldw = log_det_W(p, weights, L, dtype)
    sums = np.stack(sums, axis=1).astype(dtype)
    log_s_sum = sum(ls.sum(axis=1, dtype=dtype) for ls in log_s_all).astype(dtype)
    return dict(z=z, log_s=np.concatenate(log_s_all, axis=1), log_s_sum=log_s_sum, sums=sums, logdet_w=ldw,
                logdet=(ldw[None, :] + sums).sum(axis=1).astype(dtype))


def loss(z, logdet, sigma):
    """``efficient_loss.WaveGlowLoss.forward`` (:33-44) in float64 -> (loss, per item [B])."""
    z, logdet = np.asarray(z, np.float64), np.asarray(logdet, np.float64)
    per_item = ((z ** 2).sum(axis=1) / (2.0 * sigma * sigma) - logdet) / z.shape[1]
    return float(per_item.mean()), per_item


# ------------------------------------------------------------------------------------------------- fixture encoding ----
def pack_delta(x64, ref32):
    """float64 array as a 16-bit delta against the reference's fp32 array: (int16 delta, scale) with x64 ~= ref + delta * scale."""
    d = np.asarray(x64, np.float64) - np.asarray(ref32, np.float64)
    scale = float(np.abs(d).max()) / 32767.0 or 1.0
    return np.round(d / scale).astype(np.int16), np.float64(scale)


def unpack_delta(delta16, scale, ref32):
    return np.asarray(ref32, np.float64) + delta16.astype(np.float64) * float(scale)


def row_linf(a, b):
    """L-inf distance per row (axis 1) of two [B, R, L] arrays."""
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max(axis=(0, 2))
