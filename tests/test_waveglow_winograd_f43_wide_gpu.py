"""The three kernels of the Winograd F(4,3) in-layer of the fp32 WaveGlow (wn_winograd_layer.hip) are one arithmetic.

  default               64 quad columns per workgroup, two chunks per stage (what the launcher takes at every size)
  CTTS_F32_FORCE_SMALL  64 quad columns, one chunk per stage, chunk table read by a plain load (the kernel of the rounds before)
  CTTS_F32_NO_SMALL     128 quad columns, one workgroup per CU with 512 registers per lane, two chunks per stage

Every column's products are summed in the same order by the same instruction in all three, so whole-model outputs are equal bit for
bit, and the float64 ratios of a flow are the same number.  ctts_last_winograd_f43_width() tells which width the last layer ran.
The 128-column shape is an A/B arm only (slower on the headline, profiles/r26_01_f43_wide_gonogo.txt): the launcher never picks it by
grid size, so no peel exists and none is tested.  All cases use the `full` channel counts (C = 512, H = 256), with the three
thresholds CTTS_F32_WINOGRAD_MIN, _FUSED_MIN and _F43_MIN at 0.
"""
import numpy as np
import pytest
import torch

import waveglow_f64_restatement as wr
from cookietts_amd import WaveGlow, _lib, synthetic
from test_waveglow_flow_stage_gpu import Stage, _check_flow

pytestmark = pytest.mark.gpu

ARMS = {"default": (None, 64), "force_small": ("CTTS_F32_FORCE_SMALL", 64), "no_small": ("CTTS_F32_NO_SMALL", 128)}


@pytest.fixture(scope="module")
def full(hip_lib_path):
    return Stage("full", 9)


@pytest.fixture(scope="module")
def model(hip_lib_path):
    cfg = synthetic.WAVEGLOW_CONFIGS["full"]
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(synthetic.waveglow_state_dict(cfg, seed=5)))
    return m.cuda().eval(), cfg


def _f43(tuning):
    tuning.set("CTTS_F32_WINOGRAD_MIN", "0")
    tuning.set("CTTS_F32_WINOGRAD_FUSED_MIN", "0")
    tuning.set("CTTS_F32_WINOGRAD_F43_MIN", "0")


def _inputs(cfg, B, F, seed):
    G = cfg["n_group"]
    mel = torch.from_numpy(synthetic.synthetic_mel(B, F, seed=seed)).cuda()
    z = torch.from_numpy(synthetic.synthetic_noise(B, G, F * cfg["hop_length"] // G, seed=seed) * np.float32(0.7)).cuda()
    return mel, z


def _run_arm(tuning, arm, fn):
    """fn() under one arm's knob; checks through the width query that the arm's kernel is the one that ran."""
    knob, width = ARMS[arm]
    if knob:
        tuning.set(knob)
    try:
        out = fn()
        torch.cuda.synchronize()
        assert _lib.lib().ctts_last_winograd_f43_width() == width, (arm, _lib.lib().ctts_last_winograd_f43_width())
    finally:
        if knob:
            tuning.clear(knob)
    return out


# ------------------------------------------------------------------------------------------ 1. bits ------------------------
@pytest.mark.parametrize("F", [37, 5])
def test_three_arms_equal_bits(model, tuning, F):
    """B = 2.  F = 37: L = 1184, a ragged last 128-column tile at every d (2.3 of them at d = 1).  F = 5: L = 160 < 4 d at d = 64
    and 128, one quad block hanging past the end, mapped cond reads clamped."""
    m, cfg = model
    mel, z = _inputs(cfg, 2, F, seed=F)
    _f43(tuning)
    out = {arm: _run_arm(tuning, arm, lambda: m.infer_from_noise(mel, z)) for arm in ARMS}
    assert torch.isfinite(out["default"]).all()
    assert torch.equal(out["default"], out["force_small"])
    assert torch.equal(out["default"], out["no_small"])


def test_three_arms_equal_bits_in_a_batch_and_alone(model, tuning):
    """B = 3, F = 292 (several rounds of workgroups in every arm): the arms agree, and items 0 and 2 equal the same utterances
    run alone in the 128-column arm (alone they are a different grid)."""
    m, cfg = model
    B, F = 3, 292
    mel, z = _inputs(cfg, B, F, seed=3)
    _f43(tuning)
    out = {arm: _run_arm(tuning, arm, lambda: m.infer_from_noise(mel, z)) for arm in ARMS}
    assert torch.isfinite(out["default"]).all()
    assert torch.equal(out["default"], out["force_small"])
    assert torch.equal(out["default"], out["no_small"])
    for b in (0, B - 1):
        alone = _run_arm(tuning, "no_small", lambda: m.infer_from_noise(mel[b:b + 1], z[b:b + 1]))
        assert torch.equal(alone[0], out["default"][b])


def test_workspace_reuse(model, tuning):
    """F = 37 and then F = 5 on one model, so that the columns behind L hold the longer utterance's data: the 128-column arm is
    finite and equal to the default."""
    m, cfg = model
    _f43(tuning)
    for F in (37, 5):
        mel, z = _inputs(cfg, 2, F, seed=100 + F)
        wide = _run_arm(tuning, "no_small", lambda: m.infer_from_noise(mel, z))
        assert torch.isfinite(wide).all()
        assert torch.equal(wide, _run_arm(tuning, "default", lambda: m.infer_from_noise(mel, z)))


# ------------------------------------------------------------------------------------------ 2. one flow against float64 ----
@pytest.mark.parametrize("case", [f"full_k{k}_f{F}" for k in (0, 11) for F in (37, 9, 5)])
def test_flow_matches_float64_in_every_arm(full, tuning, case):
    """The committed float64 fixtures of the `full` channel counts, B = 2, held to the bound of every form of the flow (wr.FACTOR)
    in the 128-column arm and in the default; the ratios are the same number, since the bits are."""
    key, wseed, k, B, F, seed = wr.FLOW_CASES[case]
    z = np.load(wr.flow_case_path(case))
    n_rem, _, ch_off = wr.flow_dims(full.cfg, k)
    audio, h = wr.case_inputs(full.cfg, B, F, seed, float(z["h_scale"]))
    rows_in = audio[:, ch_off:ch_off + n_rem].astype(np.float64)
    ref_rows = wr.mix(full.w_inv(k).astype(np.float64), wr.couple(rows_in, z["e"]))
    _f43(tuning)
    ratio = {arm: _run_arm(tuning, arm, lambda: _check_flow(full, k, audio, h, F, ref_rows, z["ref_fp32_vs_fp64"][1],
                                                             {"case": case, "form": "winograd_f43", "variant": arm}))
             for arm in ARMS}
    print(f"{case}: L-inf / reference L-inf = {ratio} (bound {wr.FACTOR})")
    assert ratio["no_small"] == ratio["default"] == ratio["force_small"]
