"""Restatement of the forward (analysis) direction of the glow.py-class WaveGlow in numpy, at a chosen precision (helper of
test_waveglow_forward.py, test_waveglow_forward_gpu.py and tests/golden/make_golden_waveglow_forward.py; TEST INFRASTRUCTURE ONLY -
the product path is cookietts_amd.WaveGlow.forward over csrc/waveglow_api.hip).

Written from the equations, on waveglow_f64_restatement's flow_weights / cond_hidden / wn_stack:

    y[b,o,t]   = b_up[o] + sum_{i,f} mel[b,i,f] W_up[i,o,t - f hop]    (0 <= t - f hop < win; kept for t < F hop)
    spect      = y squeezed: row o G + g, column l = y[b, o, G l + g];      audio squeezed: row g, column l = wave[b, G l + g]
    per flow k:  every n_early_every flows (k > 0) the first n_early_size rows leave as an early output;
                 rows = W_k rows;   (b, log_s) = WN_k(rows[:h], spect);   rows[h:] = exp(log_s) rows[h:] + b
    z          = [early outputs in the order they left; the rows left at the end]
    loss       = (sum z^2 / (2 sigma^2) - sum_k sum log_s_k - B L sum_k log det W_k) / z.size
                 log det as torch.logdet gives it: NaN for det W_k < 0 (glow.py:105) - the reference's own answer, and with it
                 its loss, for a mix matrix of negative determinant

The synthetic weights (cookietts_amd.synthetic: a Householder QR's Q, slightly perturbed) ALL have det W_k < 0, so on the seven
reference goldens and "full_f9" the reference's log_det_W and loss are NaN, and NaN is what the product must answer there.  The
finite side of log det and of the loss is pinned by one more case, "toy_early_posdet": toy_early's inputs and weights with row 0
of every W_k negated (det > 0, as every trained checkpoint has: glow.py:80-81 starts at +1 and training moves it continuously).

Every function takes the dtype it computes in: float64 gives the reference, float32 the "reference rounding" run whose distance
from float64 scales the GPU tests' bounds (waveglow_f64_restatement.FACTOR).
"""
import os

import numpy as np

import waveglow_f64_restatement as wr
from cookietts_amd import synthetic

# name -> (config key, weight seed, inputs): the seven reference goldens (mel and wave of tests/golden/waveglow_<name>.npz, read by
# name) and "full_f9": config "full", weight seed 9, B = 2, F = 9 (L = 288: one whole Winograd pair block at d = 128, then a cut
# one, as in test_waveglow_flow_stage_gpu.py) with its own seeded waveform, stored in its fixture
GOLDENS = ("toy", "toy_early", "toy_spk_rezero", "toy_hop512_g16", "toy_hop384_g12", "small", "full_short")
CASES = GOLDENS + ("full_f9", "toy_early_posdet")
POSDET = "toy_early_posdet"
FULL_F9 = {"config_key": "full", "seed": 9, "B": 2, "F": 9, "input_seed": 2209, "sigma": 0.6}


def upsample_squeeze(mel, w_up, b_up, hop, n_group, dtype):
    """mel [B][M][F] -> spect [B][M G][F hop / G] at `dtype` (grouped weights [in][out / groups][win] as nn.ConvTranspose1d's)."""
    mel, w_up, b_up = (np.asarray(a).astype(dtype) for a in (mel, w_up, b_up))
    B, M, F = mel.shape
    win = w_up.shape[2]
    taps = win // hop
    opg, n_out = w_up.shape[1], b_up.shape[0]
    groups = n_out // opg
    ipg = M // groups
    y = np.zeros((B, n_out, F + taps - 1, hop), dtype)
    for gi in range(groups):
        m = mel[:, gi * ipg:(gi + 1) * ipg]
        for j in range(taps):
            wj = w_up[gi * ipg:(gi + 1) * ipg, :, j * hop:(j + 1) * hop]                  # frame f lands on output frame f + j
            y[:, gi * opg:(gi + 1) * opg, j:j + F] += np.einsum("bif,iop->bofp", m, wj)
    y = y[:, :, :F].reshape(B, n_out, F * hop) + b_up[None, :, None]
    L = F * hop // n_group
    return np.ascontiguousarray(y.reshape(B, n_out, L, n_group).transpose(0, 1, 3, 2)).reshape(B, n_out * n_group, L)


def squeeze(wave, n_group):
    """[B][L G] -> [B][G][L] (glow.py:284)."""
    B = wave.shape[0]
    return np.ascontiguousarray(wave.reshape(B, -1, n_group).transpose(0, 2, 1))


def mix_weight(sd, k, dtype):
    return np.asarray(sd[f"convinv.{k}.conv.weight"], np.float32)[:, :, 0].astype(dtype)


def forward(sd, cfg, mel, wave, speaker_ids=None, dtype=np.float64):
    """-> dict(z [B][G][L], log_s [B][S][L] (flow k's rows at offset sum_{j<k} n_half_j), logdet [n_flows] = log det W_k, all at
    `dtype`; sums float64 [B][n_flows + 1] = per item: every flow's sum of log_s, then the sum of z^2)."""
    G, wn = cfg["n_group"], cfg["WN_config"]
    C, nl = wn["n_channels"], wn["n_layers"]
    spect = upsample_squeeze(mel, sd["upsample.weight"], sd["upsample.bias"], cfg["hop_length"], G, dtype)
    rows = squeeze(np.asarray(wave).astype(dtype), G)
    assert rows.shape[2] == spect.shape[2], (rows.shape, spect.shape)
    early, log_s, logdet = [], [], []
    for k in range(cfg["n_flows"]):
        if k % cfg["n_early_every"] == 0 and k > 0:
            early.append(rows[:, :cfg["n_early_size"]])
            rows = rows[:, cfg["n_early_size"]:]
        W = mix_weight(sd, k, dtype)
        sign, logabs = np.linalg.slogdet(W)
        logdet.append(logabs if sign > 0 else np.nan)              # torch.logdet's answer (glow.py:105)
        rows = np.matmul(W, rows)
        h = rows.shape[1] // 2
        w = wr.flow_weights(sd, k, nl, dtype)
        hid = wr.cond_hidden(w, spect, speaker_ids)
        e = wr.wn_stack(w, rows[:, :h], lambda i: wr.cond_rows(w, hid, i, C), C, nl)["e"]
        ls = e[:, h:]
        rows = np.concatenate([rows[:, :h], np.exp(ls) * rows[:, h:] + e[:, :h]], axis=1)
        log_s.append(ls)
    z = np.concatenate(early + [rows], axis=1)
    assert z.dtype == dtype and z.shape[1] == G
    sums = np.stack([ls.astype(np.float64).sum(axis=(1, 2)) for ls in log_s] + [(z.astype(np.float64) ** 2).sum(axis=(1, 2))], axis=1)
    return {"z": z, "log_s": np.concatenate(log_s, axis=1), "logdet": np.asarray(logdet, dtype), "sums": sums}


def per_item_nll(sums, logdet, L, n_group, sigma):
    """Item b's (sum z^2 / 2 sigma^2 - sum log_s - L sum_k logdet_k) / (n_group L), float64; the loss is its mean."""
    sums = np.asarray(sums, np.float64)
    return (sums[:, -1] / (2.0 * sigma * sigma) - sums[:, :-1].sum(axis=1) - L * float(np.sum(np.asarray(logdet, np.float64)))) \
        / (n_group * L)


def loss(out, n_group, sigma):
    """WaveGlowLoss(sigma) of a forward() result, in float64 from its values."""
    return float(per_item_nll(out["sums"], out["logdet"], out["z"].shape[2], n_group, sigma).mean())


# ------------------------------------------------------------------------------------ fixtures ----------------
def case_path(name):
    return os.path.join(wr.GOLDEN, f"waveglow_forward_{name}.npz")


def posdet_state_dict(sd):
    """The same weights with row 0 of every 1x1 mix negated: every det W_k changes sign."""
    out = dict(sd)
    for k in [k for k in sd if k.startswith("convinv.")]:
        w = np.array(sd[k], np.float32)
        w[0] = -w[0]
        out[k] = w
    return out


def case_inputs(name):
    """-> (cfg, state dict, mel, wave, speaker ids or None, sigma) of a case; the goldens' inputs are read from the infer fixtures."""
    if name == POSDET:
        cfg, sd, mel, wave, ids, sigma = case_inputs("toy_early")
        return cfg, posdet_state_dict(sd), mel, wave, ids, sigma
    if name == "full_f9":
        c = FULL_F9
        cfg = synthetic.WAVEGLOW_CONFIGS[c["config_key"]]
        mel = synthetic.synthetic_mel(c["B"], c["F"], cfg["n_mel_channels"], seed=c["input_seed"])
        wave = np.load(case_path(name))["wave"]
        return cfg, wr.state_dict(c["config_key"], c["seed"]), mel, wave, None, c["sigma"]
    g = np.load(os.path.join(wr.GOLDEN, f"waveglow_{name}.npz"))
    key = str(g["config_key"])
    ids = g["speaker_ids"] if "speaker_ids" in g.files else None
    return synthetic.WAVEGLOW_CONFIGS[key], wr.state_dict(key, int(g["seed"])), g["mel"], g["wave"], ids, float(g["sigma"])


def full_f9_wave():
    """The seeded waveform of "full_f9": 0.3 N(0,1) from a numpy generator (the generator script stores it)."""
    c = FULL_F9
    cfg = synthetic.WAVEGLOW_CONFIGS[c["config_key"]]
    return (np.random.default_rng(c["input_seed"]).standard_normal((c["B"], c["F"] * cfg["hop_length"]), dtype=np.float32)
            * np.float32(0.3)).astype(np.float32)


# The float64 restatement's z and log_s are stored as their distance from the reference's fp32 values, in IEEE half with one
# scale per array (max |distance| -> 1024): 6 bytes per element for both instead of 12, which keeps the 200-frame "small" case
# under the size limit of a committed file.  What comes back is the float64 value to within 2^-11 of that DISTANCE (itself ~1e-6):
# a few 1e-10 absolute, < 0.05 % of the fp32 rounding distances the bounds are made of.
def pack_delta(v64, ref32):
    d = np.asarray(v64, np.float64) - np.asarray(ref32, np.float64)
    scale = 1024.0 / max(float(np.max(np.abs(d))), 1e-300)
    return (d * scale).astype(np.float16), np.float64(scale)


def unpack_delta(d16, scale, ref32):
    return np.asarray(ref32, np.float64) + d16.astype(np.float64) / float(scale)


def load_case(name):
    """The fixture of a case with the float64 arrays rebuilt: dict(z_ref, log_s_ref, log_det_W_ref, loss_ref: the reference's own
    fp32 results; z_f64, log_s_f64, sums_f64, loss_f64: the float64 restatement's; z_linf32, log_s_linf32, loss_dist32: the fp32
    restatement's distances from float64; sigma)."""
    g = np.load(case_path(name))
    out = {k: g[k] for k in g.files}
    out["z_f64"] = unpack_delta(g["z_f64_delta16"], g["z_f64_scale"], g["z_ref"])
    out["log_s_f64"] = unpack_delta(g["log_s_f64_delta16"], g["log_s_f64_scale"], g["log_s_ref"])
    return out
