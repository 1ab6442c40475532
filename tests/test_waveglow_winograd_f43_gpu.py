"""The Winograd F(4,3) form of the one-launch in-layer of the fp32 WaveGlow (wn_winograd_layer.hip, WNWG_F43).

A workgroup owns 128 packed rows x 64 quad columns and runs the four interior products, their in-register combination (exact
multipliers 1, 2, 4, 8) and the two end products with the cond rows through one chunk stream: 1.5 C products per output and row
where F(2,3) spends 2 C.  Other products than F(2,3), so the form is held to float64 per flow with the bound of every other form
(wr.FACTOR), to the direct form on whole models, and bit for bit to itself across batches and runs.  All three thresholds at 0
(CTTS_F32_WINOGRAD_MIN, CTTS_F32_WINOGRAD_FUSED_MIN, CTTS_F32_WINOGRAD_F43_MIN) take the form at every size;
CTTS_F32_WINOGRAD_NO_F43 is the F(2,3) one-launch layer.

Measured ratios (L-inf against float64 / the fp32 restatement's own, bound 8): 0.92 - 2.49 over the twelve cases below
(profiles/r23_03_f43_tests.log).
"""
import os

import numpy as np
import pytest
import torch

import waveglow_f64_restatement as wr
from conftest import GOLDEN, rms_rel_err
from cookietts_amd import WaveGlow, synthetic
from test_waveglow_flow_stage_gpu import Stage, _check_flow

pytestmark = pytest.mark.gpu

REORDERED_SUM = 1e-5       # tests/test_waveglow_winograd_gpu.py: Winograd against direct, and against the goldens


@pytest.fixture(scope="module")
def full(hip_lib_path):
    return Stage("full", 9)


def _f43(tuning):
    tuning.set("CTTS_F32_WINOGRAD_MIN", "0")
    tuning.set("CTTS_F32_WINOGRAD_FUSED_MIN", "0")
    tuning.set("CTTS_F32_WINOGRAD_F43_MIN", "0")


def _model(key, seed):
    cfg = synthetic.WAVEGLOW_CONFIGS[key] if isinstance(key, str) else key
    sd = synthetic.waveglow_state_dict(cfg, seed=seed)
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(sd))
    return m.cuda().eval(), cfg


def _inputs(cfg, B, F, seed):
    G = cfg["n_group"]
    mel = torch.from_numpy(synthetic.synthetic_mel(B, F, seed=seed)).cuda()
    z = torch.from_numpy(synthetic.synthetic_noise(B, G, F * cfg["hop_length"] // G, seed=seed) * np.float32(0.7)).cuda()
    return mel, z


# ------------------------------------------------------------------------------------------ 1. one flow against float64 ----
VARIANTS = {"default": [], "unfolded": ["CTTS_F32_NO_WN_FOLD"]}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", [f"full_k{k}_f{F}" for k in (0, 11) for F in (37, 9, 5)])
def test_f43_flow_matches_float64(full, tuning, case, variant):
    """The committed float64 fixtures of the `full` channel counts, B = 2.  F = 5 gives L = 160 < 4 d at d = 64 and 128: one quad
    block whose later members hang past the end, with mapped cond reads beyond L; F = 37 gives L = 1184, a multiple of neither 64
    nor 4 d for the large dilations.  `unfolded`: layer 0 reads x, d = 1 takes the cond copies (d = 2 does in every variant).
    Bound: the one every form of the flow is held to; _check_flow prints the ratio."""
    key, wseed, k, B, F, seed = wr.FLOW_CASES[case]
    z = np.load(wr.flow_case_path(case))
    n_rem, _, ch_off = wr.flow_dims(full.cfg, k)
    audio, h = wr.case_inputs(full.cfg, B, F, seed, float(z["h_scale"]))
    rows_in = audio[:, ch_off:ch_off + n_rem].astype(np.float64)
    ref_rows = wr.mix(full.w_inv(k).astype(np.float64), wr.couple(rows_in, z["e"]))
    _f43(tuning)
    for knob in VARIANTS[variant]:
        tuning.set(knob)
    ratio = _check_flow(full, k, audio, h, F, ref_rows, z["ref_fp32_vs_fp64"][1], {"case": case, "form": "winograd_f43", "variant": variant})
    print(f"{case} {variant}: L-inf / reference L-inf = {ratio:.3f} (bound {wr.FACTOR})")


# ------------------------------------------------------------------------------------------ 2. bits ------------------------
def test_two_runs_and_batch_items(hip_lib_path, tuning):
    """Two runs are equal, and items 0 and B - 1 of a batch of three equal the same utterances run alone."""
    m, cfg = _model("full", 5)
    B, F = 3, 292
    mel, z = _inputs(cfg, B, F, seed=3)
    _f43(tuning)
    full = m.infer_from_noise(mel, z)
    assert torch.isfinite(full).all()
    assert torch.equal(full, m.infer_from_noise(mel, z))
    for b in (0, B - 1):
        assert torch.equal(m.infer_from_noise(mel[b:b + 1], z[b:b + 1])[0], full[b])


def test_utterance_edges(hip_lib_path, tuning):
    """F = 37 and then F = 5 on the same model, so the halo and the columns behind L hold the longer utterance's data: finite, and
    the direct form as a re-ordered sum, the first and last samples included."""
    m, cfg = _model("full", 9)
    G = cfg["n_group"]
    for F in (37, 5):
        mel, z = _inputs(cfg, 2, F, seed=F)
        _f43(tuning)
        quad = m.infer_from_noise(mel, z)
        tuning.set("CTTS_F32_NO_WINOGRAD")
        direct = m.infer_from_noise(mel, z)
        tuning.clear("CTTS_F32_NO_WINOGRAD")
        assert torch.isfinite(quad).all()
        a, d = quad.cpu().numpy().astype(np.float64), direct.cpu().numpy().astype(np.float64)
        n = 2 * G
        for b in range(2):
            rms = np.sqrt(np.mean(d[b] ** 2))
            head, tail = np.max(np.abs(a[b, :n] - d[b, :n])) / rms, np.max(np.abs(a[b, -n:] - d[b, -n:])) / rms
            print(f"F={F} item {b}: head {head:.3e} tail {tail:.3e}")
            assert head < 1e-4 and tail < 1e-4, (F, b, head, tail)
        e = rms_rel_err(a, d)
        print(f"F={F}: F(4,3) vs direct {e:.3e}")
        assert e < REORDERED_SUM


def test_multi_round_grid(hip_lib_path, tuning):
    """("full", 7, 292): 2072 workgroups on 256 CUs - several rounds, and a tile count that is no multiple of 8, so the grid is
    rounded up and the workgroups beyond the last tile leave (gt >= kt_total)."""
    m, cfg = _model("full", 77)
    mel, z = _inputs(cfg, 7, 292, seed=7)
    _f43(tuning)
    first = m.infer_from_noise(mel, z)
    assert torch.isfinite(first).all()
    assert torch.equal(first, m.infer_from_noise(mel, z))


# ------------------------------------------------------------------------------------------ 3. the arms --------------------
def test_no_f43_arm_is_the_f23_one_launch_layer(hip_lib_path, tuning):
    """All three thresholds at 0: CTTS_F32_WINOGRAD_NO_F43 equals the one-launch F(2,3) form (the F(4,3) threshold unset keeps a
    short utterance on it) bit for bit; the F(4,3) form differs from it, within a re-ordered sum's distance."""
    m, cfg = _model("full", 9)
    mel, z = _inputs(cfg, 2, 37, seed=37)
    tuning.set("CTTS_F32_WINOGRAD_MIN", "0")
    tuning.set("CTTS_F32_WINOGRAD_FUSED_MIN", "0")
    f23 = m.infer_from_noise(mel, z)
    tuning.set("CTTS_F32_WINOGRAD_F43_MIN", "0")
    f43 = m.infer_from_noise(mel, z)
    tuning.set("CTTS_F32_WINOGRAD_NO_F43")
    arm = m.infer_from_noise(mel, z)
    assert torch.equal(arm, f23)
    e = rms_rel_err(f43.cpu().numpy(), f23.cpu().numpy())
    print(f"F(4,3) vs F(2,3) one-launch layer: {e:.3e}")
    assert 0.0 < e < REORDERED_SUM             # (0 would mean the form did not engage)


def test_default_threshold_keeps_short_utterances(hip_lib_path, tuning):
    """With no knob a 37-frame utterance is below every threshold: bit-equal to its CTTS_F32_WINOGRAD_NO_F43 run."""
    m, cfg = _model("full", 9)
    mel, z = _inputs(cfg, 1, 37, seed=4)
    default = m.infer_from_noise(mel, z)
    tuning.set("CTTS_F32_WINOGRAD_NO_F43")
    assert torch.equal(default, m.infer_from_noise(mel, z))


# ------------------------------------------------------------------------------------------ 4. whole models ----------------
@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("name", ["full_short", "toy_early", "toy_spk_rezero", "toy_hop512_g16", "toy_hop384_g12", "small"])
def test_f43_matches_the_golden_and_the_direct_form(hip_lib_path, tuning, name, fold):
    g = np.load(os.path.join(GOLDEN, f"waveglow_{name}.npz"))
    m, _ = _model(str(g["config_key"]), int(g["seed"]))
    ids = torch.from_numpy(g["speaker_ids"]).cuda() if "speaker_ids" in g.files else None
    mel, z = torch.from_numpy(g["mel"]).cuda(), torch.from_numpy(g["z_scaled"]).cuda()
    if not fold:
        tuning.set("CTTS_F32_NO_WN_FOLD")       # layer 0 reads x too: d = 1 on the cond copies
    _f43(tuning)
    quad = m.infer_from_noise(mel, z, speaker_id=ids).cpu().numpy()
    tuning.set("CTTS_F32_NO_WINOGRAD")
    direct = m.infer_from_noise(mel, z, speaker_id=ids).cpu().numpy()
    e = (rms_rel_err(quad, g["wave"]), rms_rel_err(quad, direct))
    print(f"{name} fold={fold}: F(4,3) vs reference {e[0]:.3e}, F(4,3) vs direct {e[1]:.3e}")
    assert np.isfinite(quad).all()
    assert e[0] < REORDERED_SUM and e[1] < REORDERED_SUM
