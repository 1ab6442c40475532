"""The two WN folds of the fp32 WaveGlow path, restated in float64 on the synthetic weights (no GPU).

1. start into layer 0: sum_tap W_in,0[tap] . x_0(t + tap) with x_0 = W_start a + b_start zero-padded outside [0, L) equals
   sum_tap (W_in,0[tap] . [W_start | b_start | 0]) . [a; 1; 0](t + tap), when the ones row is zero-padded like the conv input.
2. end into the skip sum: end(sum_i W_skip,i act_i + b_skip,i) = sum_i (W_end . W_skip,i) act_i + b', with ReZero's alpha in
   W_skip,i / b_skip,i and b' = b_end + W_end . sum_i b_skip,i.

The first and last columns are checked on their own: a bias folded without the zero padding shows only there.
The restatement itself lives in waveglow_f64_restatement.py, shared with the per-flow stage tests.
"""
import numpy as np
import pytest

from cookietts_amd import synthetic
from waveglow_f64_restatement import FOLD_ROWS, a16 as _a16, flow_weights as _flow_weights, fold_end as _fold_end, \
    fold_in0 as _fold_in0, shift as _shift, wn as _wn

CONFIGS = ["toy", "toy_early", "toy_spk_rezero", "toy_hop512_g16"]
TOL = 1e-11


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _edges(a, b, n=3):
    return max(_rel(a[..., :n], b[..., :n]), _rel(a[..., -n:], b[..., -n:]))


@pytest.mark.parametrize("name", CONFIGS)
def test_start_and_end_folds_match_the_unfolded_wn(name):
    cfg = synthetic.WAVEGLOW_CONFIGS[name]
    sd = synthetic.waveglow_state_dict(cfg, seed=17)
    C, n_layers = cfg["WN_config"]["n_channels"], cfg["WN_config"]["n_layers"]
    rng = np.random.default_rng(3)
    B, L = 2, 37
    for k, (_, n_half) in enumerate(synthetic.waveglow_flow_channels(cfg)):
        assert n_half + 1 <= FOLD_ROWS
        w = _flow_weights(sd, k, n_layers)
        a = rng.standard_normal((B, n_half, L))
        cond = rng.standard_normal((B, 2 * C * n_layers, L)) * 0.3
        e_ref, u_ref = _wn(w, a, cond, C, n_layers, fold=False)
        e_fold, u_fold = _wn(w, a, cond, C, n_layers, fold=True)
        assert _rel(u_fold, u_ref) < TOL and _edges(u_fold, u_ref) < TOL, (name, k)
        assert _rel(e_fold, e_ref) < TOL and _edges(e_fold, e_ref) < TOL, (name, k)


def test_the_ones_row_must_follow_the_zero_padding():
    """A ones row that stays 1 in the halo folds b_start into the edge columns where the reference reads zeros: the edge
    check above would see it (so it is not vacuous)."""
    cfg = synthetic.WAVEGLOW_CONFIGS["toy_early"]
    sd = synthetic.waveglow_state_dict(cfg, seed=17)
    C, n_layers = cfg["WN_config"]["n_channels"], cfg["WN_config"]["n_layers"]
    _, n_half = synthetic.waveglow_flow_channels(cfg)[0]
    w = _flow_weights(sd, 0, n_layers)
    rng = np.random.default_rng(4)
    a = rng.standard_normal((2, n_half, 37))
    cond = rng.standard_normal((2, 2 * C * n_layers, 37)) * 0.3
    _, u_ref = _wn(w, a, cond, C, n_layers, fold=False)
    f = _fold_in0(w, n_half)
    u_bad = w["in_b"][0][None, :, None] + cond[:, :2 * C]
    a16 = _a16(a)
    for t in range(3):
        shifted = _shift(a16, t - 1)
        shifted[:, n_half] = 1.0                           # the bias row without the zero padding
        u_bad = u_bad + np.einsum("or,brl->bol", f[:, :, t], shifted)
    assert _edges(u_bad, u_ref, n=1) > 1e-3
    assert _rel(u_bad[..., 1:-1], u_ref[..., 1:-1]) < TOL


@pytest.mark.parametrize("name", CONFIGS)
def test_folded_sums_are_no_less_accurate(name):
    """sum_k |W'_jk| |act_k| <= sum_c |W_end,jc| sum_k |W_skip,ck| |act_k|: the folded contraction's error bound is never
    above the two-step one's."""
    cfg = synthetic.WAVEGLOW_CONFIGS[name]
    sd = synthetic.waveglow_state_dict(cfg, seed=17)
    C, n_layers = cfg["WN_config"]["n_channels"], cfg["WN_config"]["n_layers"]
    w = _flow_weights(sd, 0, n_layers)
    Wf, _ = _fold_end(w, C, n_layers)
    act = np.abs(np.random.default_rng(5).standard_normal((C, 64)))
    for i in range(n_layers):
        skip = w["rs_w"][i][C:] if i < n_layers - 1 else w["rs_w"][i]
        assert np.all(np.abs(Wf[i]) @ act <= np.abs(w["end_w"]) @ (np.abs(skip) @ act) * (1 + 1e-12))
