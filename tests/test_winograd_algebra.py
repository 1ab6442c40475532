"""The Winograd F(2,3) pair form of the fp32 WaveGlow in-layers, restated in float64 on the synthetic weights (no GPU).

1. the mapping: pair column j of a layer of dilation d stands for t_e = (j / d) 2d + j % d and t_o = t_e + d, with
   Lp = ceil(L / 2d) d pair columns; the GATE epilogue stores a member at its natural column when that lies below L.  Even and
   odd members together must hit every column of [0, L) exactly once, and drop nothing below L.
2. the algebra: a WN stack whose in-layers run in the pair form equals the direct 3-tap form to rounding, overall and in the
   first and last 2d columns of the widest dilation on their own (a wrong zero padding or a wrong last block shows there).
3. the per-flow bound of test_waveglow_flow_stage_gpu.py (FACTOR x the fp32 restatement's own distance from float64) tells four
   planted faults of the pair form apart, each by at least 100x: the bound is not vacuous.
"""
import numpy as np
import pytest

import waveglow_f64_restatement as wr
from cookietts_amd import synthetic

TOL = 1e-11                                                    # test_wn_fold_algebra.py's
DILATIONS = [1 << i for i in range(8)]
_C128_L8 = synthetic.waveglow_config(n_flows=1, n_channels=128, n_layers=8)


@pytest.mark.parametrize("d", DILATIONS)
def test_pair_columns_cover_every_column_once(d):
    for L in sorted({1, d, 2 * d - 1, 2 * d, 2 * d + 1, 3 * d, 160, 288, 1184}):
        Lp, te, to = wr.pair_columns(L, d)
        assert Lp == (L + 2 * d - 1) // (2 * d) * d and len(te) == len(to) == Lp
        # the kernel's rule, (q / d) 2d + q % d + par d < L, spelled out column by column
        hits = np.zeros(L + 2 * d + 1, dtype=int)
        dropped = []
        for q in range(Lp):
            for par in (0, 1):
                ns = (q // d) * 2 * d + q % d + par * d
                assert ns == (te, to)[par][q]
                if ns < L:
                    hits[ns] += 1
                else:
                    dropped.append(ns)
        assert (hits[:L] == 1).all() and (hits[L:] == 0).all(), (d, L)
        assert all(ns >= L for ns in dropped) and len(dropped) == 2 * Lp - L, (d, L)
        assert Lp * 2 - L < 2 * d, (d, L)                       # never a whole pair block beyond the end


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _edges(a, b, n):
    n = min(n, a.shape[-1])
    return max(_rel(a[..., :n], b[..., :n]), _rel(a[..., -n:], b[..., -n:]))


def _cases():
    for name in ("toy", "toy_spk_rezero", "toy_hop512_g16"):
        yield name, synthetic.WAVEGLOW_CONFIGS[name], 37
    yield "c128_l8-160", _C128_L8, 160
    yield "c128_l8-288", _C128_L8, 288


@pytest.mark.parametrize("name,cfg,L", list(_cases()), ids=[c[0] for c in _cases()])
@pytest.mark.parametrize("fold", [False, True])
def test_pair_form_matches_the_direct_form(name, cfg, L, fold):
    sd = synthetic.waveglow_state_dict(cfg, seed=17)
    C, n_layers = cfg["WN_config"]["n_channels"], cfg["WN_config"]["n_layers"]
    rng = np.random.default_rng(3)
    B, edge = 2, 2 << (n_layers - 1)
    for k, (_, n_half) in enumerate(synthetic.waveglow_flow_channels(cfg)):
        w = wr.flow_weights(sd, k, n_layers)
        a = rng.standard_normal((B, n_half, L))
        cond = rng.standard_normal((B, 2 * C * n_layers, L)) * 0.3
        ref = wr.wn_stack(w, a, cond, C, n_layers)
        got = wr.wn_stack(w, a, cond, C, n_layers, fold=fold, pair=True)
        for key in ("e", "out", "x"):
            assert _rel(got[key], ref[key]) < TOL and _edges(got[key], ref[key], edge) < TOL, (name, k, key)
        if not fold:                                          # layer 0 itself in the pair form (d = 1)
            assert _rel(got["u0"], ref["u0"]) < TOL and _edges(got["u0"], ref["u0"], 2) < TOL, (name, k)


def test_fp32_pair_form_rounds_like_the_direct_form():
    """The pair form's subtractions do not call for a looser bound: in fp32 it stays within 2x of the direct form's own distance
    from float64 (and is not suspiciously better either)."""
    cfg, L, k = _C128_L8, 288, 0
    sd = synthetic.waveglow_state_dict(cfg, seed=17)
    C, n_layers = 128, 8
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((2, 8, L)) * 0.7
    h = rng.standard_normal((2, wr.COND_HIDDEN, L))
    w_inv = wr.w_inverse_f32(sd, k)
    w64, w32 = wr.flow_weights(sd, k, n_layers), wr.flow_weights(sd, k, n_layers, np.float32)
    _, r64 = wr.flow(w64, w_inv, rows.astype(np.float32), h.astype(np.float32), C, n_layers)
    _, direct = wr.flow(w32, w_inv, rows.astype(np.float32), h.astype(np.float32), C, n_layers)
    _, pair = wr.flow(w32, w_inv, rows.astype(np.float32), h.astype(np.float32), C, n_layers, fold=True, pair=True)
    ratio = wr.linf(pair, r64) / wr.linf(direct, r64)
    print(f"fp32 pair / direct distance from float64: {ratio:.2f}")
    assert 0.25 < ratio < 2.0


# (config, flow, F): a three-layer toy flow at L = 160 (d = 4: 160 = 20 blocks, whole) does not run the partial last block, so the
# eight-layer stack at L = 160 and 288 (d = 64: partial even half; d = 128: L < 2d) stands beside it
_FAULT_CASES = [("toy", synthetic.WAVEGLOW_CONFIGS["toy"], 1, 5, ("odd_cond_at_te", "t3_sign", "beyond_L_not_zeroed")),
                ("c128_l8", _C128_L8, 0, 5, wr.FAULTS), ("c128_l8", _C128_L8, 0, 9, wr.FAULTS)]


@pytest.mark.parametrize("name,cfg,k,F,faults", _FAULT_CASES, ids=[f"{c[0]}-F{c[3]}" for c in _FAULT_CASES])
def test_the_bound_tells_planted_faults_apart(name, cfg, k, F, faults):
    sd = synthetic.waveglow_state_dict(cfg, seed=17)
    C, n_layers = cfg["WN_config"]["n_channels"], cfg["WN_config"]["n_layers"]
    n_rem, _, ch_off = wr.flow_dims(cfg, k)
    ref = wr.reference_case(cfg, sd, k, 2, F, seed=11)
    audio, h = wr.case_inputs(cfg, 2, F, 11, ref["h_scale"])
    bound = wr.FACTOR * ref["ref_fp32_vs_fp64"][1]
    w, w_inv = wr.flow_weights(sd, k, n_layers), wr.w_inverse_f32(sd, k)
    rows = audio[:, ch_off:ch_off + n_rem]
    _, good = wr.flow(w, w_inv, rows, h, C, n_layers, fold=True, pair=True)
    assert wr.linf(good, ref["rows"]) < 1e-11
    for fault in faults:
        # one layer is enough: the widest dilation for the faults of the utterance's end, the middle one for the others
        layer = n_layers - 1 if fault in ("drop_last_even_half", "beyond_L_not_zeroed") else n_layers // 2
        _, bad = wr.flow(w, w_inv, rows, h, C, n_layers, fold=True, pair=True, fault=fault, fault_layer=layer)
        err = wr.linf(bad, ref["rows"])
        print(f"{name} F={F} {fault} in layer {layer}: L-inf {err:.3e} = {err / bound:.0f} x the bound {bound:.3e}")
        assert err > 100 * bound, (fault, err, bound)
