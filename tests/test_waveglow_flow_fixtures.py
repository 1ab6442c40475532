"""The float64 per-flow fixtures of tests/golden/make_golden_wn_flow.py (no GPU): present, small, what the case table says, and
reproducible - the smallest case is recomputed live from the restatement and the seeds."""
import os

import numpy as np

import waveglow_f64_restatement as wr


def test_fixtures_are_present_and_small():
    total = 0
    for name, (key, wseed, k, B, F, seed) in wr.FLOW_CASES.items():
        path = wr.flow_case_path(name)
        size = os.path.getsize(path)
        assert size < 1 << 20, (name, size)
        total += size
        z = np.load(path)
        cfg = wr.synthetic.WAVEGLOW_CONFIGS[key]
        n_rem, n_half, _ = wr.flow_dims(cfg, k)
        L = wr.steps(cfg, F)
        assert (str(z["config"]), int(z["weight_seed"]), int(z["flow"]), int(z["batch"]), int(z["frames"]), int(z["seed"])) == \
            (key, wseed, k, B, F, seed)
        assert z["e"].dtype == z["rows"].dtype == np.float64
        assert z["e"].shape == (B, 2 * n_half, L) and z["rows"].shape == (B, n_rem, L)
        assert np.isfinite(z["e"]).all() and np.isfinite(z["rows"]).all()
        # the fp32 restatement's own rounding: a few ulp of |rows| <= 3; a value far outside says the fixture is not what it claims
        assert 0.5 < float(z["h_scale"]) < 2.0
        assert all(5e-8 < v < 2e-6 for v in z["ref_fp32_vs_fp64"]), z["ref_fp32_vs_fp64"]
    assert total < 2 << 20, total


def test_smallest_fixture_is_reproduced_live():
    name = wr.SMALLEST_FLOW_CASE
    z = np.load(wr.flow_case_path(name))
    r = wr.compute_flow_case(name, h_scale=float(z["h_scale"]))
    assert wr.linf(r["e"], z["e"]) < 1e-12 and wr.linf(r["rows"], z["rows"]) < 1e-12
    live = wr.hidden_scale(wr.synthetic.WAVEGLOW_CONFIGS["full"], wr.state_dict("full", 9), wr.FLOW_CASES[name][2], wr.FLOW_CASES[name][4],
                           wr.FLOW_CASES[name][5])
    assert abs(live - float(z["h_scale"])) < 1e-9 * live
    # the fp32 run is BLAS-order dependent: the same figure to a factor, not to the bit
    assert np.all(r["ref_fp32_vs_fp64"] < 3 * z["ref_fp32_vs_fp64"]) and np.all(z["ref_fp32_vs_fp64"] < 3 * r["ref_fp32_vs_fp64"])
