"""Restatement of ONE flow of the fp32 WaveGlow path (glow.py topology) in numpy, at a chosen precision (helper of
test_wn_fold_algebra.py, test_winograd_algebra.py, test_waveglow_flow_stage_gpu.py and tests/golden/make_golden_wn_flow.py; TEST
INFRASTRUCTURE ONLY - the product path is cookietts_amd.waveglow over csrc/waveglow_api.hip).

Written from the equations, not from the kernels:

    h       = W_c1 (W_c0 [spect; speaker rows] + b_c0) + b_c1                              cond hidden (no nonlinearity)
    cond_i  = W_c2[2C i : 2C (i + 1)] h + b_c2[...]                                        layer i's rows of cond layer 2
    x_0     = W_start a_0 + b_start
    u_i     = b_in,i + cond_i + sum_tap W_in,i[tap] x_i(t + (tap - 1) 2^i)                 x zero outside [0, L)
    act_i   = tanh(u_i[:C]) sigmoid(u_i[C:])
    r_i     = alpha_i (W_rs,i act_i + b_rs,i);  x_{i+1} = x_i + r_i[:C];  out += r_i[C:]   (last layer: out += r_i)
    (b, s)  = W_end out + b_end;  a_1' = (a_1 - b) / exp(s);  audio' = W_inverse [a_0; a_1']

plus the two re-writes the HIP path runs by default: the start / end folds (layer 0 on [a_0; 1; 0], the skip sum seen through
`end`) and the Winograd F(2,3) pair form of the in-layers.  Every function takes the dtype it computes in: float64 gives the
reference, float32 the "reference rounding" run whose distance from float64 scales the GPU tests' bounds.

The weights are the ones the packer receives: weight norm folded in fp32, ReZero's alpha in the res/skip rows.
"""
import functools
import os

import numpy as np

from cookietts_amd import synthetic
from oracle import waveglow_oracle as wo

FOLD_ROWS = 16        # rows of the folded layer-0 input (waveglow_kernels.h)
COND_HIDDEN = 256     # glow.py:153

# The per-flow L-inf bound of the GPU stage tests is FACTOR x the L-inf distance of THIS restatement's fp32 run from its float64
# run on the same inputs (never a figure of the code under test).  Measured on an MI355X over every case of
# test_waveglow_flow_stage_gpu.py (profiles/r13_01_wn_flow_stage_parity.jsonl): HIP L-inf / reference L-inf between 0.67 and 1.81
# (the largest: flow 0 of "full" at L = 288, unfolded stack with Winograd in-layers).  FACTOR = 4 x the largest ratio, rounded up
# to a power of two; the margin is for MFMA K-chunk order against BLAS order.  test_hifigan.py's LINF_FACTOR = 100 is the ceiling: a
# case that needs more is a finding to explain, not a bound to raise.
FACTOR = 8.0


def shift(x, s):
    """y[..., l] = x[..., l + s], zero outside [0, L)."""
    L = x.shape[-1]
    y = np.zeros_like(x)
    if abs(s) < L:
        if s >= 0:
            y[..., :L - s] = x[..., s:]
        else:
            y[..., -s:] = x[..., :L + s]
    return y


def _conv(sd, prefix):
    if prefix + ".weight" in sd:
        return np.asarray(sd[prefix + ".weight"], np.float32)
    return wo.fold_weightnorm(sd[prefix + ".weight_g"], sd[prefix + ".weight_v"])


def flow_weights(sd, k, n_layers, dtype=np.float64):
    """Dense weights of flow k as the packer receives them: weight norm folded (fp32), ReZero alpha in the res/skip rows."""
    p = f"WN.{k}"

    def bias(name):
        return np.asarray(sd[name], np.float64).astype(dtype)
    w = {"start_w": _conv(sd, p + ".start")[:, :, 0].astype(dtype), "start_b": bias(p + ".start.bias"),
         "end_w": np.asarray(sd[p + ".end.weight"], np.float64)[:, :, 0].astype(dtype), "end_b": bias(p + ".end.bias"),
         "in_w": [], "in_b": [], "rs_w": [], "rs_b": [],
         "cond_w": [_conv(sd, f"{p}.cond_layers.{j}")[:, :, 0].astype(dtype) for j in range(3)],
         "cond_b": [bias(f"{p}.cond_layers.{j}.bias") for j in range(3)],
         "spk": np.asarray(sd[p + ".speaker_embed.weight"], np.float64).astype(dtype) if p + ".speaker_embed.weight" in sd else None}
    for i in range(n_layers):
        w["in_w"].append(_conv(sd, f"{p}.in_layers.{i}").astype(dtype))
        w["in_b"].append(bias(f"{p}.in_layers.{i}.bias"))
        alpha = float(sd[f"{p}.alpha_i.{i}"][0]) if f"{p}.alpha_i.{i}" in sd else 1.0
        w["rs_w"].append((_conv(sd, f"{p}.res_skip_layers.{i}")[:, :, 0].astype(np.float64) * alpha).astype(dtype))
        w["rs_b"].append((np.asarray(sd[f"{p}.res_skip_layers.{i}.bias"], np.float64) * alpha).astype(dtype))
    return w


def w_inverse_f32(sd, k):
    """The fp32 inverse of flow k's 1x1 mix computed the way the Python class computes the one it hands the packer (glow.py:90-99:
    W.float().inverse() on the host).  The GPU tests take the class's own tensor instead."""
    import torch
    W = torch.from_numpy(np.ascontiguousarray(sd[f"convinv.{k}.conv.weight"][:, :, 0]))
    return W.float().cpu().inverse().contiguous().numpy()


def _mm(W, x):
    return np.matmul(np.ascontiguousarray(W), x)       # [O][I] x [B][I][L] -> [B][O][L] (a strided tap slice would miss BLAS)


def gate(u, C):
    return np.tanh(u[:, :C]) / (1.0 + np.exp(-u[:, C:]))


# ------------------------------------------------------------------------------------ cond hidden -------------
def speaker_rows(w, speaker_ids, L):
    """[B][sdim][L]: the flow's embedding of each item's speaker, repeated over time (glow.py:193-196)."""
    emb = w["spk"][np.asarray(speaker_ids)]
    return np.repeat(emb[:, :, None], L, axis=2)


def cond_hidden(w, spect, speaker_ids=None):
    """cond layers 0 and 1 of one flow: spect [B][n_mel G][L] (+ speaker rows) -> h [B][256][L]."""
    dtype = w["cond_w"][0].dtype
    c = np.asarray(spect).astype(dtype)
    if w["spk"] is not None:
        c = np.concatenate([c, speaker_rows(w, speaker_ids, c.shape[2])], axis=1)
    h = _mm(w["cond_w"][0], c) + w["cond_b"][0][None, :, None]
    return _mm(w["cond_w"][1], h) + w["cond_b"][1][None, :, None]


def cond_rows(w, h, i, C):
    """Layer i's rows of cond layer 2: [B][2C][L]."""
    sl = slice(2 * C * i, 2 * C * (i + 1))
    return _mm(w["cond_w"][2][sl], h) + w["cond_b"][2][sl][None, :, None]


# ------------------------------------------------------------------------------------ in-layers ---------------
def in_layer(w_in, b_in, x, cond_i, dil):
    ks = w_in.shape[2]
    u = b_in[None, :, None] + cond_i
    for t in range(ks):
        u = u + _mm(w_in[:, :, t], shift(x, (t - ks // 2) * dil))
    return u


def pair_columns(L, d):
    """The Winograd form's pair space of a layer of dilation d, from the comment above winograd_g_kernel: pair column j stands for
    the outputs t_e = (j / d) 2d + j % d and t_o = t_e + d; there are Lp = ceil(L / 2d) d of them.  -> (Lp, t_e[Lp], t_o[Lp])."""
    Lp = -(-L // (2 * d)) * d
    j = np.arange(Lp)
    te = (j // d) * (2 * d) + j % d
    return Lp, te, te + d


def _take(x, t, beyond_zero=True):
    """x[..., t] with zeros where t lies outside [0, L) (the conv's zero padding).  beyond_zero=False is planted fault 4: columns
    at and beyond L read whatever lies there (here: the row again from its start), as a transform without the t < L guard would."""
    L = x.shape[-1]
    out = np.zeros(x.shape[:-1] + (len(t),), x.dtype)
    ok = (t >= 0) & (t < L)
    out[..., ok] = x[..., t[ok]]
    if not beyond_zero:
        over = t >= L
        out[..., over] = x[..., t[over] % L]
    return out


def winograd_g(w_in):
    """G2 = (W0 + W1 + W2) / 2 and G3 = (W0 - W1 + W2) / 2 from float64 sums, rounded once to the weights' dtype."""
    w0, w1, w2 = (w_in[:, :, t].astype(np.float64) for t in range(3))
    return ((w0 + w1 + w2) * 0.5).astype(w_in.dtype), ((w0 - w1 + w2) * 0.5).astype(w_in.dtype)


FAULTS = ("odd_cond_at_te", "drop_last_even_half", "t3_sign", "beyond_L_not_zeroed")


def in_layer_pair(w_in, b_in, x, cond_i, dil, fault=None):
    """The same u as in_layer through the F(2,3) pair form:
        V1 = x[t-d] - x[t+d]   V2 = x[t] + x[t+d]   V3 = x[t+d] - x[t]   V4 = x[t] - x[t+2d]        (t = t_e)
        u[t_e] = W0 V1 + cond[t_e] + b + G2 V2 + G3 V3,   u[t_o] = (-W2) V4 + cond[t_o] + b + G2 V2 - G3 V3
    on the Lp pair columns, scattered to the natural columns t_e and t_o = t_e + d that lie below L.  `fault`: one of FAULTS."""
    assert w_in.shape[2] == 3
    d, L = dil, x.shape[-1]
    Lp, te, to = pair_columns(L, d)
    z = fault != "beyond_L_not_zeroed"
    xm, x0, x1, x2 = _take(x, te - d, z), _take(x, te, z), _take(x, to, z), _take(x, te + 2 * d, z)
    G2, G3 = winograd_g(w_in)
    T2, T3 = _mm(G2, x0 + x1), _mm(G3, x1 - x0)
    if fault == "t3_sign":
        T3 = -T3
    ce = _take(cond_i, te, z)
    co = _take(cond_i, te if fault == "odd_cond_at_te" else to, z)
    b = b_in[None, :, None]
    ue = _mm(w_in[:, :, 0], xm - x1) + ce + b + T2 + T3
    uo = _mm(-w_in[:, :, 2], x0 - x2) + co + b + T2 - T3
    u = np.zeros(x.shape[:1] + (w_in.shape[0], L), x.dtype)
    keep_e, keep_o = te < L, to < L
    if fault == "drop_last_even_half" and L % (2 * d):
        keep_e = keep_e & (te // (2 * d) < L // (2 * d))
    u[..., te[keep_e]] = ue[..., keep_e]
    u[..., to[keep_o]] = uo[..., keep_o]
    return u


# ------------------------------------------------------------------------------------ the two folds -----------
def fold_in0(w, n_half):
    """[2C][FOLD_ROWS][ks]: rows < n_half W_in,0[tap] . W_start, row n_half W_in,0[tap] . b_start, the rest 0."""
    w_in = w["in_w"][0]
    f = np.zeros((w_in.shape[0], FOLD_ROWS, w_in.shape[2]), w_in.dtype)
    for t in range(w_in.shape[2]):
        f[:, :n_half, t] = w_in[:, :, t] @ w["start_w"]
        f[:, n_half, t] = w_in[:, :, t] @ w["start_b"]
    return f


def a16(a):
    B, n_half, L = a.shape
    out = np.zeros((B, FOLD_ROWS, L), a.dtype)
    out[:, :n_half] = a
    out[:, n_half] = 1.0
    return out


def fold_end(w, C, n_layers):
    skip_rows = [w["rs_w"][i][C:] if i < n_layers - 1 else w["rs_w"][i] for i in range(n_layers)]
    skip_bias = [w["rs_b"][i][C:] if i < n_layers - 1 else w["rs_b"][i] for i in range(n_layers)]
    Wf = [w["end_w"] @ s for s in skip_rows]
    bf = w["end_b"] + w["end_w"] @ np.sum(skip_bias, axis=0)
    return Wf, bf


# ------------------------------------------------------------------------------------ one WN stack ------------
def wn_stack(w, a, cond, C, n_layers, fold=False, pair=False, fault=None, fault_layer=None):
    """One WN stack at the precision of `w` and `a`.  cond: [B][2C n_layers][L], or a function i -> layer i's [B][2C][L].
    fold: layer 0 on [a; 1; 0] and the skip sum seen through `end`; pair: the in-layers that read x in the Winograd pair form
    (`fault` planted in layer `fault_layer`, or in every one of them).  -> dict(e, u0, out: the skip sum, x: the last x)."""
    x = _mm(w["start_w"], a) + w["start_b"][None, :, None]
    out = 0.0
    acts = []
    u0 = None
    for i in range(n_layers):
        cond_i = cond(i) if callable(cond) else cond[:, 2 * C * i:2 * C * (i + 1)]
        if fold and i == 0:
            u = in_layer(fold_in0(w, a.shape[1]), w["in_b"][0], a16(a), cond_i, 1)
        elif pair:
            f = fault if fault_layer in (None, i) else None
            u = in_layer_pair(w["in_w"][i], w["in_b"][i], x, cond_i, 2 ** i, f)
        else:
            u = in_layer(w["in_w"][i], w["in_b"][i], x, cond_i, 2 ** i)
        if i == 0:
            u0 = u
        act = gate(u, C)
        acts.append(act)
        r = _mm(w["rs_w"][i], act) + w["rs_b"][i][None, :, None]
        if i < n_layers - 1:
            x = x + r[:, :C]
            out = out + r[:, C:]
        else:
            out = out + r
    if fold:
        Wf, bf = fold_end(w, C, n_layers)
        e = sum(_mm(Wf[i], acts[i]) for i in range(n_layers)) + bf[None, :, None]
    else:
        e = _mm(w["end_w"], out) + w["end_b"][None, :, None]
    return {"e": e, "u0": u0, "out": out, "x": x}


def wn(w, a, cond, C, n_layers, fold):
    """(e, layer-0 input) of one WN stack (test_wn_fold_algebra.py's view of wn_stack)."""
    r = wn_stack(w, a, cond, C, n_layers, fold=fold)
    return r["e"], r["u0"]


# ------------------------------------------------------------------------------------ coupling, mix, un-squeeze
def couple(rows, e):
    """rows [B][n_rem][L] = [a_0; a_1], e = (b, log_s) [B][2 n_half][L] -> [a_0; (a_1 - b) / exp(s)]."""
    h = rows.shape[1] // 2
    return np.concatenate([rows[:, :h], (rows[:, h:] - e[:, :h]) / np.exp(e[:, h:])], axis=1)


def mix(w_inv, rows):
    """The inverse 1x1 conv with the GIVEN inverse (how it was inverted is not part of the flow)."""
    return _mm(np.asarray(w_inv).astype(rows.dtype), rows)


def unsqueeze(audio):
    """[B][G][L] -> [B][L G] (glow.py:349)."""
    return np.ascontiguousarray(audio.transpose(0, 2, 1)).reshape(audio.shape[0], -1)


def flow(w, w_inv, rows, h, C, n_layers, **form):
    """One flow from its inputs: rows [B][n_rem][L] (the flow's rows of the latent), h [B][256][L] its cond hidden.
    -> (e = (b, log_s), the rows after coupling and mix), at the precision of `w`; form: wn_stack's fold / pair / fault."""
    dtype = w["start_w"].dtype
    rows, h = np.asarray(rows).astype(dtype), np.asarray(h).astype(dtype)
    r = wn_stack(w, rows[:, :rows.shape[1] // 2], lambda i: cond_rows(w, h, i, C), C, n_layers, **form)
    return r["e"], mix(w_inv, couple(rows, r["e"]))


def linf(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


# ------------------------------------------------------------------------------------ seeded cases ------------
def flow_dims(cfg, k):
    """(n_rem, n_half, ch_off) of flow k."""
    n_rem, n_half = synthetic.waveglow_flow_channels(cfg)[k]
    return n_rem, n_half, cfg["n_group"] - n_rem


def steps(cfg, F):
    return F * cfg["hop_length"] // cfg["n_group"]


def hidden_scale(cfg, sd, k, F, seed):
    """RMS of flow k's real cond hidden on synthetic.synthetic_mel (the fp32 oracle's upsampling, float64 cond layers)."""
    mel = synthetic.synthetic_mel(2, F, cfg["n_mel_channels"], seed=seed)
    spect = wo.upsample_squeeze(mel, np.asarray(sd["upsample.weight"], np.float32), np.asarray(sd["upsample.bias"], np.float32),
                                cfg["hop_length"], cfg["n_group"])
    w = flow_weights(sd, k, 0)
    ids = np.arange(2) * 7 + 3 if w["spk"] is not None else None
    return float(np.sqrt(np.mean(cond_hidden(w, spect, ids) ** 2)))


def case_inputs(cfg, B, F, seed, h_scale):
    """The seeded inputs of a stage case (numpy generators: the same bits on every machine): the latent [B][n_group][L] drawn as
    the other WaveGlow tests draw it (0.7 N(0,1)) and a cond hidden [B][256][L] = h_scale N(0,1), both fp32."""
    L = steps(cfg, F)
    audio = synthetic.synthetic_noise(B, cfg["n_group"], L, seed=seed) * np.float32(0.7)
    h = np.random.default_rng(seed + 15485863).standard_normal((B, COND_HIDDEN, L), dtype=np.float32) * np.float32(h_scale)
    return audio.astype(np.float32), h.astype(np.float32)


def reference_case(cfg, sd, k, B, F, seed, h_scale=None, w_inv=None):
    """float64 reference of one flow on the seeded inputs, and the fp32 run's distance from it.
    -> dict(e, rows: float64; h_scale; ref_fp32_vs_fp64 = [L-inf of (b, log_s), L-inf of the rows])."""
    wn_cfg = cfg["WN_config"]
    C, n_layers = wn_cfg["n_channels"], wn_cfg["n_layers"]
    n_rem, _, ch_off = flow_dims(cfg, k)
    if h_scale is None:
        h_scale = hidden_scale(cfg, sd, k, F, seed)
    audio, h = case_inputs(cfg, B, F, seed, h_scale)
    w_inv = w_inverse_f32(sd, k) if w_inv is None else np.asarray(w_inv, np.float32)
    rows = audio[:, ch_off:ch_off + n_rem]
    e64, r64 = flow(flow_weights(sd, k, n_layers, np.float64), w_inv, rows, h, C, n_layers)
    e32, r32 = flow(flow_weights(sd, k, n_layers, np.float32), w_inv, rows, h, C, n_layers)
    assert e32.dtype == np.float32 and r32.dtype == np.float32
    return {"e": e64, "rows": r64, "h_scale": h_scale, "ref_fp32_vs_fp64": np.array([linf(e32, e64), linf(r32, r64)])}


@functools.lru_cache(maxsize=None)
def state_dict(name, seed):
    return synthetic.waveglow_state_dict(synthetic.WAVEGLOW_CONFIGS[name], seed=seed)


# The fixtures of tests/golden/make_golden_wn_flow.py: a float64 flow at 512 channels is too slow to recompute inside a GPU test.
# name -> (config key, weight seed, flow, batch, frames, input seed).  "full": C = 512, 8 layers, d up to 128.  Flow 0: n_half 4,
# ch_off 0; flow 11: n_half 2, the largest ch_off.  F = 5: L = 160 < 2d at d = 128, the odd half cut mid-block; F = 9: L = 288,
# one whole pair block at d = 128, then one whose even half is cut and whose odd half lies beyond L; F = 37: L = 1184, no multiple
# of 128 or 256.
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOW_CASES = {f"full_k{k}_f{F}": ("full", 9, k, 2, F, 1000 + 37 * k + F) for k in (0, 11) for F in (5, 9, 37)}
SMALLEST_FLOW_CASE = "full_k11_f5"


def flow_case_path(name):
    return os.path.join(GOLDEN, f"waveglow_flow_f64_{name}.npz")


def compute_flow_case(name, h_scale=None):
    key, wseed, k, B, F, seed = FLOW_CASES[name]
    return reference_case(synthetic.WAVEGLOW_CONFIGS[key], state_dict(key, wseed), k, B, F, seed, h_scale=h_scale)
