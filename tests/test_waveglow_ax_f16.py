"""IEEE-half storage path of the 1-D ax WaveGlow (``waveflow=False``): ``WaveGlow.set_compute_dtype(torch.float16)`` ->
``ctts_wgax_inverse_f16``, what ``WaveGlowVocoder.half()`` selects for such a model.

References: the reference's own ``inverse`` outputs (tests/golden/waveglow_ax_*.npz) at the project's waveform bound, and the
CPU restatement of the path's rounding points (ax_f16_restatement.py) at the bound the glow.py half path is held to against
its restatement.

Two goldens cannot run in half mode as they are: ``toy_merge`` (merge_res_skip) is a GTRU model and ``toy_c160`` (160 channels,
k = 5) a GTLRU model, and half storage refuses every unit but GTU.  Both refusals are asserted, and what those two configs are
there to cover runs on the SAME configs with the GTU unit (the units have no parameters: same state dict), against the
restatement and - no reference output exists for that variant - the fp32 oracle, which is within 6.5e-7 of the reference on
every golden.  merge_res_skip with a reference golden is covered by ``toy_no_res_skip`` (the same merged launches).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ax_f16_restatement as rs
from conftest import GOLDEN, rms_rel_err
from cookietts_amd import synthetic
from oracle import waveglow_ax_oracle as ao

WAVE_TOL = 1e-3                  # BASELINE.json: waveform RMS relative error
F16_VS_F16_ORACLE_TOL = 1e-3     # GPU half path vs its CPU restatement (same bound as the glow.py half path)
FORMAT_FACTOR = 2.5              # f16 must be this much closer than bf16 at the same points / bf16x3 than f16 (glow.py f16 test)

# GTU goldens of the issue's table (CPU) ...
GTU_TOYS = ["notebook_toy", "untts_toy", "toy_conv", "toy_conv_mixlast", "toy_permute", "toy_permute_mixfirst",
            "toy_g32_permute", "toy_dilations_const", "toy_c96", "toy_g32", "toy_dilations", "toy_no_res_skip",
            "toy_sigmoid_vol", "toy_wn_tconv", "toy_groupconv"]
NON_GTU_TOYS = ["toy_merge", "toy_c160"]         # GTRU, GTLRU: restated on the CPU like the others, refused by the library
FULL = ["notebook", "untts"]
# ... and the cases of the GPU runs
GPU_GOLDENS = ["notebook_toy", "notebook", "untts_toy", "untts", "toy_conv", "toy_conv_mixlast", "toy_permute",
               "toy_permute_mixfirst", "toy_no_res_skip", "toy_c96", "toy_g32", "toy_dilations", "toy_wn_tconv"]
GATES = sorted(k for k in synthetic.WAVEGLOW_AX_CONFIGS if k.startswith("toy_gate_"))       # the 13 non-GTU units


def _load(key):
    g = np.load(os.path.join(GOLDEN, f"waveglow_ax_{key}.npz"))
    cfg = synthetic.WAVEGLOW_AX_CONFIGS[str(g["config_key"])]
    return g, cfg, synthetic.waveglow_ax_state_dict(cfg, seed=int(g["seed"]))


def _ids(g):
    return g["speaker_ids"] if "speaker_ids" in g.files else None


def _melp(g):
    return np.pad(g["mel"], ((0, 0), (0, 0), (0, 1)))


# ------------------------------------------------------------------------------------------------ CPU ----
@pytest.mark.parametrize("key", GTU_TOYS + NON_GTU_TOYS + FULL)
def test_f16_restatement_matches_reference_golden(key):
    """The rounding points themselves fit the bound (measured: 2.5e-5 .. 1.7e-4 on the toys, 5.0e-4 notebook, 3.5e-4
    untts), and the same points in bf16 are several times further away (7-9x measured): the restatement rounds."""
    g, cfg, sd = _load(key)
    e16 = rms_rel_err(rs.inverse(sd, cfg, g["z"], _melp(g), _ids(g), "f16"), g["inverse_full"])
    eb = rms_rel_err(rs.inverse(sd, cfg, g["z"], _melp(g), _ids(g), "bf16"), g["inverse_full"])
    print(f"ax f16 restatement {key}: f16 {e16:.3e}, bf16 at the same points {eb:.3e}")
    assert e16 < WAVE_TOL
    assert eb > FORMAT_FACTOR * e16


def test_f16_restatement_of_a_sin16_unit_leaves_the_bound():
    """Why the four sin(16 x) units are refused: half activations in front of sin(16 x) cost 2.8e-3."""
    g, cfg, sd = _load("toy_gate_gsirru")
    e16 = rms_rel_err(rs.inverse(sd, cfg, g["z"], _melp(g), _ids(g), "f16"), g["inverse_full"])
    print(f"ax f16 restatement toy_gate_gsirru: {e16:.3e}")
    assert e16 > WAVE_TOL


def test_rounding_helper():
    v = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65520.0, 1e-8, -0.1], np.float32)
    h = rs.round_to(v, "f16")
    assert h[0] == 1.0 and h[1] == 1.0 and h[2] == np.float32(1.0 + 2.0 ** -9) and np.isinf(h[3]) and h[4] == 0
    b = rs.round_to(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.14159], np.float32), "bf16")
    assert b[0] == 1.0 and b[1] == np.float32(1.0 + 2.0 ** -6) and b[2] == np.float32(3.140625)


def _c_cfg(cfg):
    from cookietts_amd.waveglow_ax import WaveGlow
    return WaveGlow(**cfg).c_config_1d()


def test_library_exports_the_f16_entry_points_and_plans_on_the_host(hip_lib_path):
    from cookietts_amd import _lib
    lib = _lib.lib()
    for name in ("ctts_wgax_packed_f16_bytes", "ctts_wgax_pack_flow_f16", "ctts_wgax_workspace_f16_bytes", "ctts_wgax_inverse_f16"):
        assert hasattr(lib, name), name
    cfgs = synthetic.WAVEGLOW_AX_CONFIGS
    for key, cfg in (("notebook", cfgs["notebook"]), ("notebook_toy", cfgs["notebook_toy"]), ("toy_c96", cfgs["toy_c96"]),
                     ("toy_merge with GTU", rs.with_gtu(cfgs["toy_merge"])), ("toy_c160 with GTU", rs.with_gtu(cfgs["toy_c160"]))):
        c = _c_cfg(cfg)
        samples = c.n_group * 1000
        packed, ws = lib.ctts_wgax_packed_f16_bytes(C.byref(c)), lib.ctts_wgax_workspace_f16_bytes(C.byref(c), 2, samples)
        assert packed > 0 and ws > 0, key
        # 16-bit weights and C-row tensors: about half of the fp32 form (the fp32 parts - start / end, biases, latent rows - stay)
        assert packed < 0.6 * lib.ctts_wgax_packed_bytes(C.byref(c)), key
        assert ws < 0.6 * lib.ctts_wgax_workspace_bytes(C.byref(c), 2, samples), key
        assert lib.ctts_wgax_workspace_f16_bytes(C.byref(c), 2, samples + 1) == 0             # not a multiple of n_group
    for key in GATES + NON_GTU_TOYS:                                                          # every non-GTU unit is refused
        c = _c_cfg(cfgs[key])
        assert c.gated_unit != 0
        assert lib.ctts_wgax_packed_f16_bytes(C.byref(c)) == 0, key
        assert b"GTU" in lib.ctts_last_error(), key
        assert lib.ctts_wgax_workspace_f16_bytes(C.byref(c), 1, c.n_group * 100) == 0, key
        assert lib.ctts_wgax_packed_bytes(C.byref(c)) > 0, key                                # the fp32 path takes them all
        assert lib.ctts_wgax_inverse_f16(C.byref(c), None, None, None, 0, 0, 0, None, 1, 0, None, 0, None) == -1    # CTTS_E_ARG
    # K of the in-layer GEMM beyond the 16-bit GEMM's chunk table: 11 taps x 768 / 32 = 264 chunks > 253
    c = _c_cfg(cfgs["notebook_toy"])
    c.kernel_size, c.n_channels = 11, 768
    assert lib.ctts_wgax_packed_bytes(C.byref(c)) > 0 and lib.ctts_wgax_packed_f16_bytes(C.byref(c)) == 0
    assert b"K chunks" in lib.ctts_last_error()
    c.n_channels = 736                                                                        # 11 x 23 = 253: the last that fits
    assert lib.ctts_wgax_packed_f16_bytes(C.byref(c)) > 0


def test_set_compute_dtype_and_vocoder_half_select_the_mode_without_a_launch(hip_lib_path):
    from cookietts_amd import WaveGlowVocoder
    from cookietts_amd.waveglow_ax import WaveGlow
    cfgs = synthetic.WAVEGLOW_AX_CONFIGS
    m = WaveGlow(**cfgs["notebook_toy"])
    assert m._compute_dtype == torch.float32
    m._packed, m._ws = "stale", {"k": 1}
    assert m.set_compute_dtype(torch.float16) is m and m._compute_dtype == torch.float16
    assert m._packed is None and m._ws == {}                                     # blob and workspaces are per format
    assert all(p.dtype == torch.float32 for p in m.parameters())                 # fp32 masters
    m._packed = "kept"
    m.set_compute_dtype(torch.float16)                                           # no change: nothing is thrown away
    assert m._packed == "kept"
    m.set_compute_dtype(torch.float32)
    assert m._compute_dtype == torch.float32 and m._packed is None
    with pytest.raises(ValueError):
        m.set_compute_dtype(torch.bfloat16)
    for key in GATES + NON_GTU_TOYS:
        g = WaveGlow(**cfgs[key])
        with pytest.raises(NotImplementedError, match="GTU"):
            g.set_compute_dtype(torch.float16)
        assert g._compute_dtype == torch.float32
        g.set_compute_dtype(torch.float32)                                       # always fine
    wf = WaveGlow(**synthetic.WAVEFLOW_CONFIGS["toy"])
    assert wf.waveflow
    with pytest.raises(NotImplementedError, match="waveflow=True"):
        wf.set_compute_dtype(torch.float16)
    big = WaveGlow(**dict(cfgs["toy_conv"], WN_config=dict(cfgs["toy_conv"]["WN_config"], n_channels=768, kernel_size_w=11)))
    with pytest.raises(NotImplementedError, match="K chunks"):
        big.set_compute_dtype(torch.float16)
    # .half(): IEEE-half storage for the 1-D GTU model, split bf16 for every other ax model
    v = WaveGlowVocoder(WaveGlow(**cfgs["notebook_toy"])).half()
    assert v.waveglow._compute_dtype == torch.float16 and v.waveglow._f32_gemm_mode is None
    assert next(v.waveglow.parameters()).dtype == torch.float32
    v = WaveGlowVocoder(wf).half()
    assert v.waveglow._compute_dtype == torch.float32 and v.waveglow._f32_gemm_mode == "bf16x3"
    v = WaveGlowVocoder(WaveGlow(**cfgs["toy_merge"])).half()                    # GTRU
    assert v.waveglow._compute_dtype == torch.float32 and v.waveglow._f32_gemm_mode == "bf16x3"


# ------------------------------------------------------------------------------------------------ GPU ----
def _model(cfg, seed):
    from cookietts_amd.waveglow_ax import WaveGlow
    sd = synthetic.waveglow_ax_state_dict(cfg, seed=seed)
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(sd))
    return m.cuda().eval(), sd


def _run(m, z, melp, ids):
    out, _ = m.inverse(torch.from_numpy(z).cuda(), torch.from_numpy(melp).cuda(),
                       speaker_ids=None if ids is None else torch.from_numpy(ids).cuda())
    return out.numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("key", GPU_GOLDENS)
def test_hip_f16_matches_reference_golden(hip_lib_path, key):
    """One launch of ``inverse`` per mode.  On the 2-6 flow toys the restatement figure is tight (a misplaced rounding point
    shows there); on the 48 / 24-flow models two correct half runs differ by about as much as each differs from the golden
    (fp32 noise in front of the gate flips half roundings), so both figures sit near 5e-4 there."""
    g, cfg, sd = _load(key)
    m, _ = _model(cfg, int(g["seed"]))
    z, melp, ids = g["z"], _melp(g), _ids(g)
    never = _run(m, z, melp, ids)                                              # a model that was never switched
    m.set_compute_dtype(torch.float16)
    got = _run(m, z, melp, ids)
    e_gold = rms_rel_err(got, g["inverse_full"])
    e_rest = rms_rel_err(got, rs.inverse(sd, cfg, z, melp, ids, "f16"))
    m.set_compute_dtype(torch.float32)
    back = _run(m, z, melp, ids)
    m.set_f32_gemm_mode("bf16x3")
    e_x3 = rms_rel_err(_run(m, z, melp, ids), g["inverse_full"])
    print(f"waveglow_ax f16 {key}: vs reference golden {e_gold:.3e}, vs f16 restatement {e_rest:.3e}; bf16x3 vs golden {e_x3:.3e}")
    assert np.isfinite(got).all()
    assert e_rest < F16_VS_F16_ORACLE_TOL
    assert e_gold < WAVE_TOL
    assert FORMAT_FACTOR * e_x3 < e_gold                    # half storage is not bf16x3 under another name
    assert np.array_equal(back, never)                      # back to fp32: bit for bit the path that was never switched


@pytest.mark.gpu
@pytest.mark.parametrize("key", NON_GTU_TOYS)
def test_hip_f16_merge_and_c160_configs_with_the_gtu_unit(hip_lib_path, key):
    """toy_merge (merge_res_skip: every layer's C rows are skip rows) and toy_c160 (160 channels: ragged last M-block, split row
    160, k = 5) as they are carry GTRU / GTLRU and are refused; with GTU they run - against the restatement and the fp32 oracle."""
    g, cfg0, _ = _load(key)
    m0, _ = _model(cfg0, int(g["seed"]))
    with pytest.raises(NotImplementedError, match="GTU"):
        m0.set_compute_dtype(torch.float16)
    cfg = rs.with_gtu(cfg0)
    m, sd = _model(cfg, int(g["seed"]))
    z, melp, ids = g["z"], _melp(g), _ids(g)
    ref32 = ao.waveglow_ax_inverse(sd, cfg, z, melp, ids)
    e_f32 = rms_rel_err(_run(m, z, melp, ids), ref32)
    m.set_compute_dtype(torch.float16)
    got = _run(m, z, melp, ids)
    e_rest = rms_rel_err(got, rs.inverse(sd, cfg, z, melp, ids, "f16"))
    e_ref = rms_rel_err(got, ref32)
    print(f"waveglow_ax f16 {key} with GTU: vs fp32 oracle {e_ref:.3e}, vs f16 restatement {e_rest:.3e}; fp32 path vs oracle {e_f32:.3e}")
    assert np.isfinite(got).all()
    assert e_rest < F16_VS_F16_ORACLE_TOL and e_ref < WAVE_TOL
    assert FORMAT_FACTOR * e_f32 < e_ref


@pytest.mark.gpu
@pytest.mark.parametrize("knob", ["CTTS_BF16_NO_PS", "CTTS_BF16_NO_PP", "CTTS_BF16_NO_WIDE"])
def test_hip_f16_block_shapes_agree(hip_lib_path, tuning, knob):
    """The addend epilogue rounds alike in the persistent, skewed, wide and narrow kernels: notebook_toy at batch 8 and 6200
    latent columns (25 wide tiles per utterance with a ragged last one, enough tiles for the wide shapes), identical bits."""
    cfg = synthetic.WAVEGLOW_AX_CONFIGS["notebook_toy"]
    m, _ = _model(cfg, 5)
    m.set_compute_dtype(torch.float16)
    B, Fr = 8, 621                                            # L = 620 * 120 / 12
    mel = torch.from_numpy(synthetic.synthetic_mel(B, Fr, cfg["n_mel_channels"], seed=6)).cuda()
    z = torch.from_numpy(np.random.default_rng(6).standard_normal((B, (Fr - 1) * 120)).astype(np.float32) * np.float32(0.7)).cuda()
    ids = torch.arange(B, dtype=torch.int64).cuda() * 3
    default, _ = m.inverse(z, mel, speaker_ids=ids, return_CPU=False)
    assert torch.isfinite(default).all()
    one, _ = m.inverse(z[5:6], mel[5:6], speaker_ids=ids[5:6], return_CPU=False)     # (a single utterance: narrow kernels)
    assert torch.equal(one[0], default[5])
    tuning.set(knob)
    again, _ = m.inverse(z, mel, speaker_ids=ids, return_CPU=False)
    assert torch.equal(default, again)


@pytest.mark.gpu
def test_hip_f16_ragged_batch_independent_and_repeatable(hip_lib_path):
    cfg = synthetic.WAVEGLOW_AX_CONFIGS["notebook_toy"]
    m, sd = _model(cfg, 9)
    m.set_compute_dtype(torch.float16)
    B, Fr = 3, 46                                              # L = 45 * 10 = 450: ragged against the 128- and 256-column tiles
    melp = synthetic.synthetic_mel(B, Fr, cfg["n_mel_channels"], seed=3)
    z = np.random.default_rng(5).standard_normal((B, (Fr - 1) * 120)).astype(np.float32) * np.float32(0.8)
    ids = np.array([5, 400, 77], np.int64)
    tz, tm, ti = torch.from_numpy(z).cuda(), torch.from_numpy(melp).cuda(), torch.from_numpy(ids).cuda()
    got, _ = m.inverse(tz, tm, speaker_ids=ti, return_CPU=False)
    err = rms_rel_err(got.cpu().numpy(), rs.inverse(sd, cfg, z, melp, ids, "f16"))
    print(f"waveglow_ax f16 notebook_toy B=3 L=450: vs f16 restatement {err:.3e}")
    assert torch.isfinite(got).all() and err < F16_VS_F16_ORACLE_TOL
    for b in range(B):                                         # utterances do not interact; workspace reuse across shapes
        one, _ = m.inverse(tz[b:b + 1], tm[b:b + 1], speaker_ids=ti[b:b + 1], return_CPU=False)
        assert torch.equal(one[0], got[b])
    again, _ = m.inverse(tz, tm, speaker_ids=ti, return_CPU=False)
    assert torch.equal(again, got)


@pytest.mark.gpu
def test_hip_f16_one_frame_mel(hip_lib_path):
    """A one-frame mel: two conditioning frames after ``infer``'s padding, interpolated to 10 latent columns."""
    cfg = synthetic.WAVEGLOW_AX_CONFIGS["notebook_toy"]
    m, sd = _model(cfg, 4)
    m.set_compute_dtype(torch.float16)
    melp = np.pad(synthetic.synthetic_mel(2, 1, cfg["n_mel_channels"], seed=8), ((0, 0), (0, 0), (0, 1)))
    z = np.random.default_rng(8).standard_normal((2, 120)).astype(np.float32) * np.float32(0.7)
    ids = np.array([1, 300], np.int64)
    got = _run(m, z, melp, ids)
    err = rms_rel_err(got, rs.inverse(sd, cfg, z, melp, ids, "f16"))
    print(f"waveglow_ax f16 notebook_toy one frame: vs f16 restatement {err:.3e}")
    assert np.isfinite(got).all() and err < F16_VS_F16_ORACLE_TOL
    out = m.infer(torch.from_numpy(melp[:, :, :1]).cuda(), speaker_ids=torch.from_numpy(ids).cuda(), sigma=0.7)
    assert out.shape == (2, 0)                                 # infer trims the padding frame's hop again
