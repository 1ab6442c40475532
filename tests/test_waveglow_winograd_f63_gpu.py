"""The Winograd F(6,3) form of the one-launch in-layer of the fp32 WaveGlow (wn_winograd_layer.hip, WNWG_F63).

Where the F(4,3) layer engages, the layers of dilation d % 4 == 0 run on 64 HEX columns (384 natural columns) per workgroup: six
interior products, their in-register combination (exact multipliers 2^-5 .. 2^5), and the two end products with the cond rows read
in place through the hex map - 8/6 C products per output and row where F(4,3) spends 1.5 C.  Other products than F(4,3), so the form
is held to float64 per flow with the bound of every other form (wr.FACTOR = 8 x the fp32 restatement's own error), to the direct
form on whole models, and bit for bit to itself across batches.  All four thresholds at 0 (CTTS_F32_WINOGRAD_MIN, _FUSED_MIN,
_F43_MIN, _F63_MIN) take the form at every size; CTTS_F32_WINOGRAD_NO_F63 is the F(4,3) form.

Lengths (L = 32 F columns): F = 5 gives L = 160 < 6 d from d = 32 on (one hex block whose later members hang past the end, mapped
cond reads beyond L); F = 13 gives L = 416, no multiple of 6 d for any d, and at d = 4 Lh = 72 hex columns: one 64-column tile plus
the two d-blocks behind it (Lh is a multiple of d, so one tile plus a single column does not exist where the form runs); F = 37
gives L = 1184, no multiple of 6 d either, several tiles at the small dilations.

Measured ratios (L-inf against float64 / the fp32 restatement's own, bound 8): see profiles/r34_03_f63_tests.log.
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


_STAGES, _LIVE = {}, {}


@pytest.fixture(scope="module")
def stage(hip_lib_path):
    def get(name):
        if name not in _STAGES:
            _STAGES[name] = Stage(name, 17)
        return _STAGES[name]
    yield get
    _STAGES.clear()
    _LIVE.clear()


def _live_reference(st, k, B, F, seed):
    """float64 and the fp32 restatement's own distance from it, once per case (shared by the fold variants)."""
    key = (st.name, k, B, F, seed)
    if key not in _LIVE:
        _LIVE[key] = wr.reference_case(st.cfg, st.sd, k, B, F, seed, w_inv=st.w_inv(k))
    return _LIVE[key]


def _f63(tuning):
    tuning.set("CTTS_F32_WINOGRAD_MIN", "0")
    tuning.set("CTTS_F32_WINOGRAD_FUSED_MIN", "0")
    tuning.set("CTTS_F32_WINOGRAD_F43_MIN", "0")
    tuning.set("CTTS_F32_WINOGRAD_F63_MIN", "0")


def _model(key, seed):
    cfg = synthetic.WAVEGLOW_CONFIGS[key]
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
@pytest.mark.parametrize("B,F", [(1, 13), (3, 5), (3, 13), (1, 37)])
@pytest.mark.parametrize("name", ["toy", "small"])
def test_f63_toy_flows_match_float64(stage, tuning, name, B, F, variant):
    """n_channels 128 (`toy`: d = 1, 2, 4 - one F(6,3) layer) and 256 (`small`: d up to 128 - six of them), fold on and off, batch 1
    and 3, the first and the last flow; references computed live, once per case.  Bound: the one every form of the flow is held
    to; _check_flow prints the ratio."""
    st = stage(name)
    seed = 23
    _f63(tuning)
    for knob in VARIANTS[variant]:
        tuning.set(knob)
    for k in (0, st.n_flows - 1):
        ref = _live_reference(st, k, B, F, seed)
        audio, h = wr.case_inputs(st.cfg, B, F, seed, ref["h_scale"])
        ratio = _check_flow(st, k, audio, h, F, ref["rows"], ref["ref_fp32_vs_fp64"][1],
                            {"case": f"{name}_k{k}_b{B}_f{F}", "form": "winograd_f63", "variant": variant})
        print(f"{name} k{k} B{B} F{F} {variant}: L-inf / reference L-inf = {ratio:.3f} (bound {wr.FACTOR})")


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", [f"full_k{k}_f{F}" for k in (0, 11) for F in (37, 9, 5)])
def test_f63_full_flow_matches_float64(full, tuning, case, variant):
    """The committed float64 fixtures of the `full` channel counts (C = 512: the chunk stream of the headline, 352 chunks), B = 2."""
    key, wseed, k, B, F, seed = wr.FLOW_CASES[case]
    z = np.load(wr.flow_case_path(case))
    n_rem, _, ch_off = wr.flow_dims(full.cfg, k)
    audio, h = wr.case_inputs(full.cfg, B, F, seed, float(z["h_scale"]))
    rows_in = audio[:, ch_off:ch_off + n_rem].astype(np.float64)
    ref_rows = wr.mix(full.w_inv(k).astype(np.float64), wr.couple(rows_in, z["e"]))
    _f63(tuning)
    for knob in VARIANTS[variant]:
        tuning.set(knob)
    ratio = _check_flow(full, k, audio, h, F, ref_rows, z["ref_fp32_vs_fp64"][1], {"case": case, "form": "winograd_f63", "variant": variant})
    print(f"{case} {variant}: L-inf / reference L-inf = {ratio:.3f} (bound {wr.FACTOR})")


# ------------------------------------------------------------------------------------------ 2. bits ------------------------
@pytest.mark.parametrize("key,F", [("small", 13), ("full", 292)])
def test_two_runs_and_batch_items(hip_lib_path, tuning, key, F):
    """Two runs are equal, and every item of a batch of three equals the same utterance run alone.  ("full", 292): 25 hex tiles per
    item at d = 4 - several rounds of workgroups, and a tile count that is no multiple of 8 (the grid is rounded up)."""
    m, cfg = _model(key, 5)
    B = 3
    mel, z = _inputs(cfg, B, F, seed=3)
    _f63(tuning)
    batch = m.infer_from_noise(mel, z)
    assert torch.isfinite(batch).all()
    assert torch.equal(batch, m.infer_from_noise(mel, z))
    for b in range(B):
        assert torch.equal(m.infer_from_noise(mel[b:b + 1], z[b:b + 1])[0], batch[b])


def test_utterance_edges(hip_lib_path, tuning):
    """F = 37 and then F = 5 on the same model, so the halo and the columns behind L hold the longer utterance's data: finite, and
    the direct form as a re-ordered sum, the first and last samples included."""
    m, cfg = _model("full", 9)
    G = cfg["n_group"]
    for F in (37, 5):
        mel, z = _inputs(cfg, 2, F, seed=F)
        _f63(tuning)
        hexf = m.infer_from_noise(mel, z)
        tuning.set("CTTS_F32_NO_WINOGRAD")
        direct = m.infer_from_noise(mel, z)
        tuning.clear("CTTS_F32_NO_WINOGRAD")
        assert torch.isfinite(hexf).all()
        a, d = hexf.cpu().numpy().astype(np.float64), direct.cpu().numpy().astype(np.float64)
        n = 2 * G
        for b in range(2):
            rms = np.sqrt(np.mean(d[b] ** 2))
            head, tail = np.max(np.abs(a[b, :n] - d[b, :n])) / rms, np.max(np.abs(a[b, -n:] - d[b, -n:])) / rms
            print(f"F={F} item {b}: head {head:.3e} tail {tail:.3e}")
            assert head < 1e-4 and tail < 1e-4, (F, b, head, tail)
        e = rms_rel_err(a, d)
        print(f"F={F}: F(6,3) vs direct {e:.3e}")
        assert e < REORDERED_SUM


# ------------------------------------------------------------------------------------------ 3. the arms --------------------
@pytest.mark.parametrize("B", [1, 3])
def test_no_f63_arm_is_the_f43_form(hip_lib_path, tuning, B):
    """All four thresholds at 0: CTTS_F32_WINOGRAD_NO_F63 equals the F(4,3) form (the F(6,3) threshold unset keeps a short utterance
    on it) bit for bit; the F(6,3) form differs from it, within a re-ordered sum's distance."""
    m, cfg = _model("full", 9)
    mel, z = _inputs(cfg, B, 37, seed=37)
    tuning.set("CTTS_F32_WINOGRAD_MIN", "0")
    tuning.set("CTTS_F32_WINOGRAD_FUSED_MIN", "0")
    tuning.set("CTTS_F32_WINOGRAD_F43_MIN", "0")
    f43 = m.infer_from_noise(mel, z)
    tuning.set("CTTS_F32_WINOGRAD_F63_MIN", "0")
    f63 = m.infer_from_noise(mel, z)
    tuning.set("CTTS_F32_WINOGRAD_NO_F63")
    arm = m.infer_from_noise(mel, z)
    assert torch.equal(arm, f43)
    e = rms_rel_err(f63.cpu().numpy(), f43.cpu().numpy())
    print(f"B={B}: F(6,3) vs F(4,3): {e:.3e}")
    assert 0.0 < e < REORDERED_SUM             # (0 would mean the form did not engage)


def test_default_threshold_keeps_short_utterances(hip_lib_path, tuning):
    """With no knob a 37-frame utterance is below every threshold: bit-equal to its CTTS_F32_WINOGRAD_NO_F63 run."""
    m, cfg = _model("full", 9)
    mel, z = _inputs(cfg, 1, 37, seed=4)
    default = m.infer_from_noise(mel, z)
    tuning.set("CTTS_F32_WINOGRAD_NO_F63")
    assert torch.equal(default, m.infer_from_noise(mel, z))


# ------------------------------------------------------------------------------------------ 4. whole models ----------------
@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("name", ["full_short", "toy_spk_rezero", "small"])
def test_f63_matches_the_golden_and_the_direct_form(hip_lib_path, tuning, name, fold):
    """The goldens whose models have a layer the form runs at (n_layers >= 3)."""
    g = np.load(os.path.join(GOLDEN, f"waveglow_{name}.npz"))
    m, _ = _model(str(g["config_key"]), int(g["seed"]))
    ids = torch.from_numpy(g["speaker_ids"]).cuda() if "speaker_ids" in g.files else None
    mel, z = torch.from_numpy(g["mel"]).cuda(), torch.from_numpy(g["z_scaled"]).cuda()
    if not fold:
        tuning.set("CTTS_F32_NO_WN_FOLD")
    _f63(tuning)
    hexf = m.infer_from_noise(mel, z, speaker_id=ids).cpu().numpy()
    tuning.set("CTTS_F32_NO_WINOGRAD")
    direct = m.infer_from_noise(mel, z, speaker_id=ids).cpu().numpy()
    e = (rms_rel_err(hexf, g["wave"]), rms_rel_err(hexf, direct))
    print(f"{name} fold={fold}: F(6,3) vs reference {e[0]:.3e}, F(6,3) vs direct {e[1]:.3e}")
    assert np.isfinite(hexf).all()
    assert e[0] < REORDERED_SUM and e[1] < REORDERED_SUM
