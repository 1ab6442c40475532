"""HiFi-GAN generator (cookietts_amd.hifigan over csrc/hifigan.hip) against the reference's own outputs.

The goldens (tests/golden/hifigan_*.npz, written by tests/golden/make_golden_hifigan.py) hold the reference generator's fp32
waveform on a recorded mel, the seed of the numpy weight recipe, and the reference's own rounding ``ref_fp32_vs_fp64``
(relative RMS, L-inf of its fp32 forward against its fp64 forward).  Bounds:

* CPU restatement (fp64) vs golden: relative RMS < max(ORACLE_TOL, 4 x ref_fp32_vs_fp64) - the golden itself carries the
  reference's fp32 rounding, the margin is for its summation order.
* HIP path vs golden: relative RMS < WAVE_TOL (BASELINE.json's waveform bound) AND L-inf < 100 x the fixture's
  ref_fp32_vs_fp64 L-inf: a wrong halo column at an utterance edge is an O(0.1) fault on a few samples, which an RMS over
  230 400 samples would hide; a different summation order (MFMA K chunks against MKL) stays within a few times the
  reference's own rounding.  Measured values are printed and appended to profiles/r9_01_hifigan_parity.jsonl.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import REPO, rms_rel_err
from cookietts_amd import HiFiGANGenerator, _lib, load_hifigan, synthetic
from cookietts_amd import hifigan as hg
import hifigan_restatement as hr

ORACLE_TOL = 5e-6
WAVE_TOL = 1e-3
LINF_FACTOR = 100.0
SHIPPED = ("v1", "v2", "v3", "v1_48khz")
CASES = hr.golden_cases()
PARITY_LOG = os.path.join(REPO, "profiles", "r9_01_hifigan_parity.jsonl")


def _case(name):
    z = hr.load_case(name)
    key = str(z["config"])
    cfg = synthetic.HIFIGAN_CONFIGS[key]
    return cfg, synthetic.hifigan_state_dict(cfg, seed=int(z["seed"])), z


def _model(cfg, sd, device="cuda:0"):
    m = HiFiGANGenerator(hg.AttrDict(cfg))
    m.load_state_dict(synthetic.to_torch(sd))
    return m.to(device).eval()


# --------------------------------------------------------------------------- without a GPU ----
def test_golden_set_is_complete():
    assert set(CASES) >= {"toy_rb1", "toy_rb2", "toy_rate4", "v1", "v2", "v3", "v1_48khz", "v1_full_length"}
    assert CASES[-1] == "v1_full_length"
    frames = {hr.load_case(n)["mel"].shape[2] for n in CASES}
    assert {3, 33, 129, 900} <= frames


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference_golden(name):
    cfg, sd, z = _case(name)
    out = hr.generator_np(cfg, sd, z["mel"])
    err = rms_rel_err(out, z["audio"])
    bound = max(ORACLE_TOL, 4.0 * float(z["ref_fp32_vs_fp64"][0]))
    print(f"{name}: restatement vs golden rel rms {err:.3e} (bound {bound:.3e})")
    assert out.shape == z["audio"].shape
    assert err < bound


def test_goldens_tell_the_final_slope_apart():
    """conv_post's input LeakyReLU has slope 0.01 (F.leaky_relu's default), not the 0.1 used everywhere else."""
    cfg, sd, z = _case("v1")
    wrong = hr.generator_np(cfg, sd, z["mel"], final_slope=0.1)
    assert rms_rel_err(wrong, z["audio"]) > 0.02


@pytest.mark.parametrize("key", SHIPPED)
def test_module_tree_matches_reference_state_dict(key, hip_lib_path):
    shapes = json.load(open(os.path.join(REPO, "tests", "golden", "hifigan_state_shapes.json")))[key]
    m = HiFiGANGenerator(hg.AttrDict(synthetic.HIFIGAN_CONFIGS[key]))
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == shapes
    assert {k: list(v.shape) for k, v in synthetic.hifigan_state_dict(synthetic.HIFIGAN_CONFIGS[key]).items()} == shapes


def test_remove_weight_norm_leaves_the_folded_weights(hip_lib_path):
    cfg = synthetic.HIFIGAN_CONFIGS["toy_rb1"]
    sd = synthetic.hifigan_state_dict(cfg, seed=5)
    m = HiFiGANGenerator(hg.AttrDict(cfg))
    m.load_state_dict(synthetic.to_torch(sd))
    before = m.folded_weights()
    m.remove_weight_norm()
    keys = set(m.state_dict())
    assert not any(k.endswith(("weight_g", "weight_v")) for k in keys)
    want = hr.folded_weights(cfg, sd, torch.float64)
    for prefix, (w, b) in want.items():
        got = m.state_dict()[prefix + ".weight"]
        assert got.shape == w.shape
        assert float((got.double() - w).abs().max()) <= 1e-6 * float(w.abs().max())
        assert torch.equal(m.state_dict()[prefix + ".bias"].double(), b)
    for (w0, b0), (w1, b1) in zip(before, m.folded_weights()):
        assert float((w0 - w1).abs().max()) <= 1e-6 * float(w0.abs().max()) and torch.equal(b0, b1)


def _write_checkpoint(tmp_path, cfg, sd):
    path = os.path.join(str(tmp_path), "g_00001000")
    torch.save({"generator": synthetic.to_torch(sd)}, path)
    with open(os.path.join(str(tmp_path), "config.json"), "w") as f:
        json.dump(cfg, f)
    return path


def test_load_hifigan_round_trip(tmp_path, hip_lib_path):
    cfg = synthetic.HIFIGAN_CONFIGS["toy_rb2"]
    sd = synthetic.hifigan_state_dict(cfg, seed=9)
    gen, h = load_hifigan(_write_checkpoint(tmp_path, cfg, sd), device="cpu")
    assert h.upsample_rates == cfg["upsample_rates"] and h["resblock"] == "2"
    assert isinstance(gen, HiFiGANGenerator) and not gen.training
    want = hr.folded_weights(cfg, sd, torch.float64)
    assert set(gen.state_dict()) == {p + s for p in want for s in (".weight", ".bias")}
    for prefix, (w, _) in want.items():
        assert float((gen.state_dict()[prefix + ".weight"].double() - w).abs().max()) <= 1e-6 * float(w.abs().max())
    with pytest.raises(_lib.HipLibraryError):
        gen(torch.zeros(1, 80, 4))                                        # CPU tensors raise: no fallback


@pytest.mark.parametrize("field,value,word", [
    ("resblock", "3", "resblock"),
    ("resblock_kernel_sizes", [3, 4], "resblock_kernel_sizes"),
    ("upsample_kernel_sizes", [5, 4], "upsample_kernel_sizes"),
    ("resblock_kernel_sizes", [3, 13], "resblock_kernel_sizes"),
    ("resblock_dilation_sizes", [[1, 3, 5], [1, 3, 40]], "resblock_dilation_sizes"),
    ("upsample_rates", [2] * 9, "upsample_rates"),
    ("upsample_initial_channel", 66, "upsample_initial_channel"),
])
def test_constructor_refuses_by_name(field, value, word, hip_lib_path):
    cfg = dict(synthetic.HIFIGAN_CONFIGS["toy_rb1"])
    cfg[field] = value
    if field == "upsample_rates":
        cfg["upsample_kernel_sizes"] = [4] * 9
        cfg["upsample_initial_channel"] = 1024
    with pytest.raises(NotImplementedError, match=word):
        HiFiGANGenerator(hg.AttrDict(cfg))


def test_size_queries_without_gpu(hip_lib_path):
    lib = _lib.lib()
    for key in SHIPPED:
        c = hg.c_config(synthetic.HIFIGAN_CONFIGS[key])
        assert lib.ctts_hifigan_packed_bytes(ctypes.byref(c)) > 0
        assert lib.ctts_hifigan_weight_floats(ctypes.byref(c)) > 0
        assert lib.ctts_hifigan_workspace_bytes(ctypes.byref(c), 16, 900) > 0

    def refused(word, **edit):
        c = hg.c_config(synthetic.HIFIGAN_CONFIGS["v1"])
        for k, v in edit.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        assert lib.ctts_hifigan_packed_bytes(ctypes.byref(c)) == 0
        assert word in lib.ctts_last_error(), lib.ctts_last_error()
        assert lib.ctts_hifigan_workspace_bytes(ctypes.byref(c), 1, 10) == 0
    refused(b"resblock", resblock=3)
    refused(b"resblock_kernel_sizes", resblock_kernel_sizes=(1, 6))
    refused(b"resblock_kernel_sizes", resblock_kernel_sizes=(2, 13))
    refused(b"upsample_kernel_sizes", upsample_kernel_sizes=(0, 17))
    refused(b"upsample_rates", n_ups=9)
    refused(b"resblock_kernel_sizes", n_kernels=5)
    refused(b"upsample_initial_channel", upsample_initial_channel=520)
    refused(b"num_mels", num_mels=0)
    c = hg.c_config(synthetic.HIFIGAN_CONFIGS["v1"])
    c.resblock_dilation_sizes[2][2] = 13                                    # k 11: halo 130 > 128
    assert lib.ctts_hifigan_packed_bytes(ctypes.byref(c)) == 0 and b"resblock_dilation_sizes" in lib.ctts_last_error()
    c = hg.c_config(synthetic.HIFIGAN_CONFIGS["v1"])
    assert lib.ctts_hifigan_workspace_bytes(ctypes.byref(c), 0, 10) == 0 and b"batch" in lib.ctts_last_error()
    assert lib.ctts_hifigan_workspace_bytes(ctypes.byref(c), 1, 0) == 0 and b"frames" in lib.ctts_last_error()


def test_forward_refuses_bad_arguments_before_any_launch(hip_lib_path):
    """Every check of ctts_hifigan_forward_f32 / _pack_f32 is host code in front of the first launch: the pointers below are
    never dereferenced (no GPU is needed, none is touched)."""
    lib = _lib.lib()
    c = hg.c_config(synthetic.HIFIGAN_CONFIGS["toy_rb1"])
    need = lib.ctts_hifigan_workspace_bytes(ctypes.byref(c), 2, 8)
    fake = ctypes.c_void_p(4096)
    ok = dict(packed=fake, mel=fake, mel_ld=8, audio=fake, batch=2, frames=8, ws=fake, ws_bytes=need)

    def call(**edit):
        a = dict(ok, **edit)
        return lib.ctts_hifigan_forward_f32(ctypes.byref(c), a["packed"], a["mel"], a["mel_ld"], a["audio"], a["batch"], a["frames"],
                                            a["ws"], a["ws_bytes"], None)
    assert call(mel=None) == -1 and b"NULL" in lib.ctts_last_error()
    assert call(audio=None) == -1
    assert call(mel_ld=7) == -1 and b"mel_ld" in lib.ctts_last_error()
    assert call(batch=0) == -1 and b"batch" in lib.ctts_last_error()
    assert call(frames=0) == -1 and b"frames" in lib.ctts_last_error()
    assert call(ws_bytes=need - 4) == -3 and b"workspace" in lib.ctts_last_error()
    assert call(ws=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.ctts_last_error()
    bad = hg.c_config(synthetic.HIFIGAN_CONFIGS["toy_rb1"])
    bad.resblock = 7
    assert lib.ctts_hifigan_forward_f32(ctypes.byref(bad), fake, fake, 8, fake, 2, 8, fake, need, None) == -1
    n = lib.ctts_hifigan_weight_floats(ctypes.byref(c))
    assert lib.ctts_hifigan_pack_f32(ctypes.byref(c), fake, n - 1, fake, None) == -1 and b"weight floats" in lib.ctts_last_error()
    assert lib.ctts_hifigan_pack_f32(ctypes.byref(c), None, n, fake, None) == -1


def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(REPO, "include", "cookietts_hip.h")).read()
    for name in ("ctts_hifigan_config", "ctts_hifigan_weight_floats", "ctts_hifigan_packed_bytes", "ctts_hifigan_pack_f32",
                 "ctts_hifigan_workspace_bytes", "ctts_hifigan_forward_f32"):
        assert name in header
        assert name == "ctts_hifigan_config" or name in _lib.SIGNATURES
    assert "#define CTTS_ABI_VERSION 7" in header


def test_macs_from_the_shapes():
    """The bench row's FLOP count: v1 is about 0.3 G MAC per mel frame."""
    per_frame = hr.generator_macs(synthetic.HIFIGAN_CONFIGS["v1"], 900) / 900
    assert 0.25e9 < per_frame < 0.35e9


# --------------------------------------------------------------------------- on the GPU ----
def _linf(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _check_golden(name):
    cfg, sd, z = _case(name)
    m = _model(cfg, sd)
    with torch.no_grad():
        out = m(torch.from_numpy(z["mel"]).to("cuda:0"))
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == z["audio"].shape
    out = out.cpu().numpy()
    err, linf = rms_rel_err(out, z["audio"]), _linf(out, z["audio"])
    ref_rel, ref_linf = (float(v) for v in z["ref_fp32_vs_fp64"])
    rec = {"case": name, "config": str(z["config"]), "batch": int(z["mel"].shape[0]), "frames": int(z["mel"].shape[2]),
           "rel_rms": err, "linf": linf, "ref_fp32_vs_fp64_rel_rms": ref_rel, "ref_fp32_vs_fp64_linf": ref_linf,
           "linf_over_ref": linf / ref_linf, "bound_rel_rms": WAVE_TOL, "bound_linf": LINF_FACTOR * ref_linf}
    print(json.dumps(rec))
    try:
        with open(PARITY_LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass
    assert np.isfinite(out).all()
    assert err < WAVE_TOL
    assert linf < LINF_FACTOR * ref_linf


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASES if "full_length" not in n])
def test_hifigan_matches_reference_golden(name):
    _check_golden(name)


@pytest.mark.gpu
def test_hifigan_batch_item_equals_single_call():
    """Item i of a B=16 call equals the B=1 call on the same mel: batch items never see each other."""
    cfg, sd, z = _case("v1")
    m = _model(cfg, sd)
    mel = torch.from_numpy(synthetic.synthetic_mel(16, 21, 80, seed=77)).to("cuda:0")
    bound = LINF_FACTOR * float(z["ref_fp32_vs_fp64"][1])
    with torch.no_grad():
        full = m(mel).cpu().numpy()
        for i in (0, 7, 15):
            one = m(mel[i:i + 1]).cpu().numpy()
            d = _linf(full[i:i + 1], one)
            print(f"item {i}: L-inf {d:.3e} (bound {bound:.3e})")
            assert d < bound


@pytest.mark.gpu
def test_hifigan_wide_block_shapes_equal_the_narrow_ones_bit_for_bit():
    """The wide shapes engage from HG_NARROW_BELOW = 1024 workgroups (hg_launch in hifigan_plan.h, one rule for the three
    formats).  toy_rate4 at B=64 x 4096 frames: conv_pre (64 rows, 256-column tiles) starts 1 x 16 x 64 = 1024 workgroups ->
    64 x 256; ups.0 (128 rows, 128-column tiles) 1 x 32 x 64 = 2048 -> 128 x 128.  A single item starts 16 / 32 and stays
    narrow.  Same packed weights and same K order either way, so the items are equal bit for bit."""
    cfg, sd, _ = _case("toy_rate4")
    B, T = 64, 4096
    assert (T + 255) // 256 * B >= 1024 and (T + 127) // 128 * B >= 1024 and (T + 127) // 128 < 1024
    m = _model(cfg, sd)
    mel = torch.from_numpy(synthetic.synthetic_mel(B, T, cfg["num_mels"], seed=64)).to("cuda:0")
    with torch.no_grad():
        full = m(mel)
        for i in (0, 63):
            one = m(mel[i:i + 1])
            assert torch.equal(full[i:i + 1], one), i
    assert torch.isfinite(full).all()


@pytest.mark.gpu
def test_hifigan_is_deterministic_and_models_do_not_disturb_each_other():
    cfg1, sd1, z1 = _case("toy_rb1")
    cfg2, sd2, z2 = _case("v3")
    m1 = _model(cfg1, sd1)
    mel1 = torch.from_numpy(z1["mel"]).to("cuda:0")
    with torch.no_grad():
        a = m1(mel1).clone()
        b = m1(mel1).clone()
        m2 = _model(cfg2, sd2)
        other = m2(torch.from_numpy(z2["mel"]).to("cuda:0")).cpu().numpy()
        c = m1(mel1).clone()
    assert torch.equal(a, b) and torch.equal(a, c)
    assert rms_rel_err(other, z2["audio"]) < WAVE_TOL
    assert rms_rel_err(a.cpu().numpy(), z1["audio"]) < WAVE_TOL


@pytest.mark.gpu
def test_hifigan_repacks_when_a_parameter_changes():
    cfg, sd, z = _case("toy_rb2")
    m = _model(cfg, sd)
    mel = torch.from_numpy(z["mel"]).to("cuda:0")
    with torch.no_grad():
        a = m(mel).clone()
        m.conv_post.bias.add_(0.25)
        b = m(mel).clone()
        m.load_state_dict(synthetic.to_torch(sd))
        c = m(mel).clone()
        m.remove_weight_norm()
        d = m(mel).cpu().numpy()
    assert not torch.equal(a, b)
    assert torch.equal(a, c)
    assert _linf(d, a.cpu().numpy()) < LINF_FACTOR * float(z["ref_fp32_vs_fp64"][1])


@pytest.mark.gpu
def test_hifigan_half_means_fp16_parameters_fp32_products():
    """``.half()`` (text2speech.py:262): fp16 parameters, fp16 mel in, fp16 out, equal - after the one rounding of the
    waveform to fp16 - to the fp32 path run on the fp16-rounded weights and the fp16-rounded mel."""
    cfg, sd, z = _case("toy_rate4")
    m16 = _model(cfg, sd).half()
    assert next(m16.parameters()).dtype == torch.float16
    mel16 = torch.from_numpy(z["mel"]).to("cuda:0").to(next(m16.parameters()).dtype)
    sd_rounded = {k: v.astype(np.float16).astype(np.float32) for k, v in sd.items()}
    m32 = _model(cfg, sd_rounded)
    with torch.no_grad():
        out16 = m16(mel16)
        out32 = m32(mel16.float())
    assert out16.dtype == torch.float16 and out32.dtype == torch.float32
    assert torch.equal(out16, out32.half())
    assert rms_rel_err(out16.float().cpu().numpy(), z["audio"]) < 2e-2        # fp16-rounded weights: still the same waveform


@pytest.mark.gpu
def test_hifigan_matches_reference_golden_full_length():
    _check_golden("v1_full_length")
