"""The one-launch Winograd layer of the fp32 WaveGlow (wn_winograd_layer.hip: T2 / T3 stay in registers).

One workgroup runs the four products of a pair block through one chunk stream, ((S2 +- S3) + products) + b, where the paired
launches (CTTS_F32_WINOGRAD_NO_FUSED) round ((products + b) + T2) +- T3: a re-ordered sum, so the form is held to float64 per flow
with the bound of the other forms, to the direct form on whole models, and bit for bit to itself across its two kernel widths,
the round peel, batches and runs.  Both thresholds at 0 (CTTS_F32_WINOGRAD_MIN, CTTS_F32_WINOGRAD_FUSED_MIN) take the form at
every size; CTTS_F32_FORCE_SMALL / CTTS_F32_NO_SMALL pin the 64- / 128-column kernel.
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


def _fused(tuning):
    tuning.set("CTTS_F32_WINOGRAD_MIN", "0")
    tuning.set("CTTS_F32_WINOGRAD_FUSED_MIN", "0")


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
VARIANTS = {"narrow": ["CTTS_F32_FORCE_SMALL"], "wide": ["CTTS_F32_NO_SMALL"], "unfolded": ["CTTS_F32_NO_WN_FOLD"]}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", [f"full_k{k}_f{F}" for k in (0, 11) for F in (37, 9, 5)])
def test_fused_flow_matches_float64(full, tuning, case, variant):
    """The committed float64 fixtures of the `full` channel counts, B = 2; F = 5 gives L = 160 < 2 d at d = 128: one pair block
    whose odd half hangs past the end, with mapped cond reads beyond L.  `unfolded`: layer 0 reads x, d = 1 takes the cond copies
    (d = 2 does in every variant).  Bound: the one every form of the flow is held to; _check_flow prints the ratio."""
    key, wseed, k, B, F, seed = wr.FLOW_CASES[case]
    z = np.load(wr.flow_case_path(case))
    n_rem, _, ch_off = wr.flow_dims(full.cfg, k)
    audio, h = wr.case_inputs(full.cfg, B, F, seed, float(z["h_scale"]))
    rows_in = audio[:, ch_off:ch_off + n_rem].astype(np.float64)
    ref_rows = wr.mix(full.w_inv(k).astype(np.float64), wr.couple(rows_in, z["e"]))
    _fused(tuning)
    for knob in VARIANTS[variant]:
        tuning.set(knob)
    ratio = _check_flow(full, k, audio, h, F, ref_rows, z["ref_fp32_vs_fp64"][1], {"case": case, "form": "winograd_fused", "variant": variant})
    print(f"{case} {variant}: L-inf / reference L-inf = {ratio:.3f} (bound {wr.FACTOR})")


# ------------------------------------------------------------------------------------------ 2. bit-equality ----------------
def test_utterance_edges_both_widths(hip_lib_path, tuning):
    """F = 37 (L = 1184, a multiple of neither 128 nor 64) and then F = 5 on the same model, so the halo and the columns behind L
    hold the longer utterance's data: the two kernel widths agree bit for bit, and with the direct form as a re-ordered sum, the
    first and last samples included."""
    m, cfg = _model("full", 9)
    G = cfg["n_group"]
    _fused(tuning)
    for F in (37, 5):
        mel, z = _inputs(cfg, 2, F, seed=F)
        tuning.set("CTTS_F32_FORCE_SMALL")
        narrow = m.infer_from_noise(mel, z)
        tuning.clear("CTTS_F32_FORCE_SMALL")
        tuning.set("CTTS_F32_NO_SMALL")
        wide = m.infer_from_noise(mel, z)
        tuning.clear("CTTS_F32_NO_SMALL")
        tuning.set("CTTS_F32_NO_WINOGRAD")
        direct = m.infer_from_noise(mel, z)
        tuning.clear("CTTS_F32_NO_WINOGRAD")
        assert torch.isfinite(narrow).all()
        assert torch.equal(narrow, wide), F
        a, d = narrow.cpu().numpy().astype(np.float64), direct.cpu().numpy().astype(np.float64)
        n = 2 * G
        for b in range(2):
            rms = np.sqrt(np.mean(d[b] ** 2))
            head, tail = np.max(np.abs(a[b, :n] - d[b, :n])) / rms, np.max(np.abs(a[b, -n:] - d[b, -n:])) / rms
            print(f"F={F} item {b}: head {head:.3e} tail {tail:.3e}")
            assert head < 1e-4 and tail < 1e-4, (F, b, head, tail)
        assert rms_rel_err(a, d) < REORDERED_SUM


# the peel shapes of tests/test_waveglow_winograd_gpu.py.  ("full", 7, 292): 259 pair-space tiles x 8 channel blocks = 2072 workgroups =
# 4 rounds + 24 on 256 CUs: the 128-column kernel with 3 tiles of the last item peeled into the 64-column one.  2 x 8 x 512 at
# 5 x 823: 515 tiles x 8 = 4120 = 8 rounds + 24.
_PEEL_CFG = synthetic.waveglow_config(n_flows=2, n_channels=512, n_layers=8, n_early_every=4)


@pytest.mark.parametrize("key,B,F", [("full", 7, 292), (_PEEL_CFG, 5, 823)], ids=["full-7x292", "2x8x512-5x823"])
def test_round_peel_and_both_widths(hip_lib_path, tuning, key, B, F):
    """The peeled launch, the single launch (CTTS_F32_NO_ROUND_SPLIT), the 128-column kernel alone, the 64-column kernel alone and
    a second run: the same bits."""
    m, cfg = _model(key, 77)
    mel, z = _inputs(cfg, B, F, seed=7)
    _fused(tuning)
    peeled = m.infer_from_noise(mel, z)
    again = m.infer_from_noise(mel, z)
    tuning.set("CTTS_F32_NO_ROUND_SPLIT")
    one = m.infer_from_noise(mel, z)
    tuning.clear("CTTS_F32_NO_ROUND_SPLIT")
    tuning.set("CTTS_F32_NO_SMALL")
    wide = m.infer_from_noise(mel, z)
    tuning.clear("CTTS_F32_NO_SMALL")
    tuning.set("CTTS_F32_FORCE_SMALL")
    narrow = m.infer_from_noise(mel, z)
    assert torch.isfinite(peeled).all()
    assert torch.equal(peeled, again)
    assert torch.equal(peeled, one)
    assert torch.equal(peeled, wide)
    assert torch.equal(peeled, narrow)


def test_fused_layer_does_not_mix_batch_items(hip_lib_path, tuning):
    """Items 0 and B - 1 of a batch of three equal the same utterances run alone."""
    m, cfg = _model("full", 5)
    B, F = 3, 292
    mel, z = _inputs(cfg, B, F, seed=3)
    _fused(tuning)
    full = m.infer_from_noise(mel, z)
    assert torch.isfinite(full).all()
    for b in (0, B - 1):
        assert torch.equal(m.infer_from_noise(mel[b:b + 1], z[b:b + 1])[0], full[b])


# ------------------------------------------------------------------------------------------ 3. the arms --------------------
def test_no_fused_arm_is_the_paired_form(hip_lib_path, tuning):
    """CTTS_F32_WINOGRAD_NO_FUSED with the fused threshold at 0 = the paired launches (CTTS_F32_WINOGRAD_MIN=0 alone: the fused
    threshold keeps short utterances on them) = the five-launch form, bit for bit; the fused form differs from them by a
    re-ordered sum only."""
    m, cfg = _model("full", 9)
    mel, z = _inputs(cfg, 2, 37, seed=37)
    tuning.set("CTTS_F32_WINOGRAD_MIN", "0")
    lean = m.infer_from_noise(mel, z)
    tuning.set("CTTS_F32_WINOGRAD_PLAIN")
    plain = m.infer_from_noise(mel, z)
    tuning.clear("CTTS_F32_WINOGRAD_PLAIN")
    tuning.set("CTTS_F32_WINOGRAD_FUSED_MIN", "0")
    fused = m.infer_from_noise(mel, z)
    tuning.set("CTTS_F32_WINOGRAD_NO_FUSED")
    arm = m.infer_from_noise(mel, z)
    assert torch.equal(arm, lean) and torch.equal(lean, plain)
    e = rms_rel_err(fused.cpu().numpy(), lean.cpu().numpy())
    print(f"fused vs paired launches: {e:.3e}")
    assert 0.0 < e < REORDERED_SUM             # (0 would mean the fused form did not engage)


def test_default_thresholds_keep_short_utterances(hip_lib_path, tuning):
    """With no knob a 37-frame utterance is below both thresholds: bit-equal to its CTTS_F32_WINOGRAD_NO_FUSED run."""
    m, cfg = _model("full", 9)
    mel, z = _inputs(cfg, 1, 37, seed=4)
    default = m.infer_from_noise(mel, z)
    tuning.set("CTTS_F32_WINOGRAD_NO_FUSED")
    assert torch.equal(default, m.infer_from_noise(mel, z))


# ------------------------------------------------------------------------------------------ 4. whole model -----------------
@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("name", ["full_short", "toy_early", "toy_spk_rezero", "toy_hop512_g16", "toy_hop384_g12", "small"])
def test_fused_matches_the_golden_and_the_direct_form(hip_lib_path, tuning, name, fold):
    g = np.load(os.path.join(GOLDEN, f"waveglow_{name}.npz"))
    m, _ = _model(str(g["config_key"]), int(g["seed"]))
    ids = torch.from_numpy(g["speaker_ids"]).cuda() if "speaker_ids" in g.files else None
    mel, z = torch.from_numpy(g["mel"]).cuda(), torch.from_numpy(g["z_scaled"]).cuda()
    if not fold:
        tuning.set("CTTS_F32_NO_WN_FOLD")       # layer 0 reads x too: d = 1 on the cond copies
    _fused(tuning)
    fused = m.infer_from_noise(mel, z, speaker_id=ids).cpu().numpy()
    tuning.set("CTTS_F32_NO_WINOGRAD")
    direct = m.infer_from_noise(mel, z, speaker_id=ids).cpu().numpy()
    e = (rms_rel_err(fused, g["wave"]), rms_rel_err(fused, direct))
    print(f"{name} fold={fold}: fused vs reference {e[0]:.3e}, fused vs direct {e[1]:.3e}")
    assert np.isfinite(fused).all()
    assert e[0] < REORDERED_SUM and e[1] < REORDERED_SUM
