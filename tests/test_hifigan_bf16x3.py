"""Split-bf16 products of the HiFi-GAN generator (``set_f32_gemm_mode("bf16x3")`` over csrc/hifigan_bf16x3.hip).

Bounds are test_hifigan.py's for the fp32 path, unchanged: relative RMS < WAVE_TOL (1e-3) against the reference's fp32 golden
and L-inf < LINF_FACTOR (100) x the fixture's ``ref_fp32_vs_fp64`` L-inf.  The restatement of the documented arithmetic
(tests/hifigan_bf16x3_restatement.py: split operands, float64 sums, fp32 stored activations) sits at 1.0e-5 .. 1.5e-5 relative RMS
and 18 x .. 31 x the reference's L-inf on the CPU; two correct evaluations (fp32 against float64 accumulation) differ by up to
39 x; a dropped cross term or hi * hi alone is 5 000 x or more.  Every measured ratio is printed and appended to
profiles/r13_01_hifigan_bf16x3_parity.jsonl.

Bit-exactness: the K order of a column's sum is a function of the layer and its K chunk only, so a batch item equals its
single-item call in the narrow block shapes (any small launch) and in the wide ones (>= HG_NARROW_BELOW = 1024 workgroups).
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import REPO, rms_rel_err
from cookietts_amd import HiFiGANGenerator, _lib, load_hifigan, synthetic
from cookietts_amd import hifigan as hg
import hifigan_bf16x3_restatement as h3
import hifigan_restatement as hr

WAVE_TOL = 1e-3           # tests/test_hifigan.py
LINF_FACTOR = 100.0       # tests/test_hifigan.py
FAULT_FACTOR = 10.0       # a planted fault must be this far OUTSIDE the L-inf bound
SHORT = ("toy_rate4", "toy_rb1", "v1", "v3", "v1_48khz", "toy_rb2", "v2")
FAULTS = {"no x_lo w_hi": ("hh", "lh"), "no x_hi w_lo": ("hh", "hl"), "hi hi only": ("hh",)}
NEW_SYMBOLS = ("ctts_hifigan_packed_bf16x3_bytes", "ctts_hifigan_pack_bf16x3", "ctts_hifigan_workspace_bf16x3_bytes",
               "ctts_hifigan_forward_bf16x3")
PARITY_LOG = os.path.join(REPO, "profiles", "r13_01_hifigan_bf16x3_parity.jsonl")
# v1's size queries before the split format existed (the layer list, KC and the offsets of the fp32 and f16 plans feed these)
V1_PACKED_F32, V1_PACKED_F16 = 61_070_336, 30_561_280
V1_WS_F32, V1_WS_F16 = 2_359_296_000, 1_179_648_000          # batch 16 x 900 frames


def _case(name):
    z = hr.load_case(name)
    cfg = synthetic.HIFIGAN_CONFIGS[str(z["config"])]
    return cfg, synthetic.hifigan_state_dict(cfg, seed=int(z["seed"])), z


@functools.lru_cache(maxsize=None)
def _restated(name):
    """The restatement's waveform of a golden case: computed once, shared by the CPU and the GPU tests, never modified."""
    cfg, sd, z = _case(name)
    out = h3.generator_np(cfg, sd, z["mel"])
    out.setflags(write=False)
    return out


def _model(cfg, sd, device="cuda:0"):
    m = HiFiGANGenerator(hg.AttrDict(cfg))
    m.load_state_dict(synthetic.to_torch(sd))
    return m.to(device).eval()


def _linf(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _log(rec):
    print(json.dumps(rec))
    try:
        with open(PARITY_LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


# --------------------------------------------------------------------------- without a GPU ----
def test_short_cases_are_the_goldens_but_the_full_length_one():
    assert sorted(SHORT) == sorted(n for n in hr.golden_cases() if "full_length" not in n)


def test_bf16x3_symbols_are_declared_bound_and_exported(hip_lib_path):
    header = open(os.path.join(REPO, "include", "cookietts_hip.h")).read()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in header and name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        assert ctypes.cast(getattr(ctypes.CDLL(hip_lib_path), name), ctypes.c_void_p).value
    assert "#define CTTS_ABI_VERSION 7" in header
    assert lib.ctts_abi_version() == 7


def test_bf16x3_size_queries_without_gpu(hip_lib_path):
    """A hi | lo pair is the 4 bytes of the fp32 value: the blob has the fp32 blob's size (its documented size) and the workspace
    IS the fp32 workspace.  The fp32 and f16 plans are where they were.  Refusals are the fp32 plan's, with the same word."""
    lib = _lib.lib()
    for key, cfg in synthetic.HIFIGAN_CONFIGS.items():
        c = hg.c_config(cfg)
        p32, p3 = lib.ctts_hifigan_packed_bytes(ctypes.byref(c)), lib.ctts_hifigan_packed_bf16x3_bytes(ctypes.byref(c))
        assert p3 > 0 and p3 == p32, key
        for batch, frames in ((1, 3), (2, 33), (16, 900)):
            w32 = lib.ctts_hifigan_workspace_bytes(ctypes.byref(c), batch, frames)
            assert w32 > 0 and lib.ctts_hifigan_workspace_bf16x3_bytes(ctypes.byref(c), batch, frames) == w32, key
    # the other two plans did not move (figures of the parent commit)
    c = hg.c_config(synthetic.HIFIGAN_CONFIGS["v1"])
    assert lib.ctts_hifigan_packed_bytes(ctypes.byref(c)) == V1_PACKED_F32
    assert lib.ctts_hifigan_packed_f16_bytes(ctypes.byref(c)) == V1_PACKED_F16
    assert lib.ctts_hifigan_workspace_bytes(ctypes.byref(c), 16, 900) == V1_WS_F32
    assert lib.ctts_hifigan_workspace_f16_bytes(ctypes.byref(c), 16, 900) == V1_WS_F16

    def refused(word, **edit):
        c = hg.c_config(synthetic.HIFIGAN_CONFIGS["v1"])
        for k, v in edit.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        assert lib.ctts_hifigan_packed_bytes(ctypes.byref(c)) == 0 and word in lib.ctts_last_error()
        assert lib.ctts_hifigan_packed_bf16x3_bytes(ctypes.byref(c)) == 0
        assert word in lib.ctts_last_error(), lib.ctts_last_error()
        assert lib.ctts_hifigan_workspace_bf16x3_bytes(ctypes.byref(c), 1, 10) == 0
        assert word in lib.ctts_last_error(), lib.ctts_last_error()
    refused(b"resblock", resblock=3)
    refused(b"resblock_kernel_sizes", resblock_kernel_sizes=(1, 6))
    refused(b"resblock_kernel_sizes", resblock_kernel_sizes=(2, 13))
    refused(b"upsample_kernel_sizes", upsample_kernel_sizes=(0, 17))
    refused(b"upsample_rates", n_ups=9)
    refused(b"resblock_kernel_sizes", n_kernels=5)
    refused(b"upsample_initial_channel", upsample_initial_channel=520)
    refused(b"num_mels", num_mels=0)
    refused(b"resblock_dilation_sizes", resblock_dilation_sizes=(2, (ctypes.c_int32 * 3)(1, 3, 13)))     # k 11: halo 130 > 128
    c = hg.c_config(synthetic.HIFIGAN_CONFIGS["v1"])
    assert lib.ctts_hifigan_workspace_bf16x3_bytes(ctypes.byref(c), 0, 10) == 0 and b"batch" in lib.ctts_last_error()
    assert lib.ctts_hifigan_workspace_bf16x3_bytes(ctypes.byref(c), 1, 0) == 0 and b"frames" in lib.ctts_last_error()


def test_bf16x3_forward_refuses_bad_arguments_before_any_launch(hip_lib_path):
    """Every check of ctts_hifigan_forward_bf16x3 / _pack_bf16x3 is host code in front of the first launch: the pointers below are
    never dereferenced (no GPU is needed, none is touched)."""
    lib = _lib.lib()
    c = hg.c_config(synthetic.HIFIGAN_CONFIGS["toy_rb1"])
    need = lib.ctts_hifigan_workspace_bf16x3_bytes(ctypes.byref(c), 2, 8)
    assert need > 0
    fake = ctypes.c_void_p(4096)
    ok = dict(packed=fake, mel=fake, mel_ld=8, audio=fake, batch=2, frames=8, ws=fake, ws_bytes=need)

    def call(**edit):
        a = dict(ok, **edit)
        return lib.ctts_hifigan_forward_bf16x3(ctypes.byref(c), a["packed"], a["mel"], a["mel_ld"], a["audio"], a["batch"], a["frames"],
                                               a["ws"], a["ws_bytes"], None)
    assert call(mel=None) == -1 and b"NULL" in lib.ctts_last_error()
    assert call(audio=None) == -1
    assert call(packed=None) == -1
    assert call(ws=None) == -1
    assert call(mel_ld=7) == -1 and b"mel_ld" in lib.ctts_last_error()
    assert call(batch=0) == -1 and b"batch" in lib.ctts_last_error()
    assert call(frames=0) == -1 and b"frames" in lib.ctts_last_error()
    assert call(ws_bytes=need - 4) == -3 and b"workspace" in lib.ctts_last_error()
    assert call(ws=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.ctts_last_error()
    assert call(packed=ctypes.c_void_p(4104)) == -1 and b"aligned" in lib.ctts_last_error()
    bad = hg.c_config(synthetic.HIFIGAN_CONFIGS["toy_rb1"])
    bad.resblock = 7
    assert lib.ctts_hifigan_forward_bf16x3(ctypes.byref(bad), fake, fake, 8, fake, 2, 8, fake, need, None) == -1
    assert b"resblock" in lib.ctts_last_error()
    n = lib.ctts_hifigan_weight_floats(ctypes.byref(c))
    assert lib.ctts_hifigan_pack_bf16x3(ctypes.byref(c), fake, n - 1, fake, None) == -1 and b"weight floats" in lib.ctts_last_error()
    assert lib.ctts_hifigan_pack_bf16x3(ctypes.byref(c), None, n, fake, None) == -1
    assert lib.ctts_hifigan_pack_bf16x3(ctypes.byref(c), fake, n, None, None) == -1
    assert lib.ctts_hifigan_pack_bf16x3(ctypes.byref(c), fake, n, ctypes.c_void_p(4104), None) == -1 and b"aligned" in lib.ctts_last_error()
    assert lib.ctts_hifigan_pack_bf16x3(ctypes.byref(bad), fake, n, fake, None) == -1


def test_set_f32_gemm_mode_selects_and_invalidates_without_a_launch(hip_lib_path, tmp_path):
    cfg = synthetic.HIFIGAN_CONFIGS["toy_rb1"]
    m = HiFiGANGenerator(hg.AttrDict(cfg))
    assert m._f32_gemm_mode is None and m._path() == "f32"
    m._packed, m._ws = "stale", {"k": 1}
    assert m.set_f32_gemm_mode("bf16x3") is m and m._f32_gemm_mode == "bf16x3" and m._path() == "bf16x3"
    assert m._packed is None and m._ws == {}                                     # the blob is per format
    m._packed = "kept"
    m.set_f32_gemm_mode("bf16x3")                                                # no change: nothing is thrown away
    assert m._packed == "kept"
    for same in (None, "default", "f32"):                                        # three names of the fp32 MFMA
        m.set_f32_gemm_mode("bf16x3")
        m._packed = "stale"
        assert m.set_f32_gemm_mode(same) is m and m._path() == "f32" and m._packed is None
    m._packed = "kept"
    m.set_f32_gemm_mode("default").set_f32_gemm_mode(None)                       # fp32 by another name: kept
    assert m._packed == "kept"
    for bad in ("bf16", "f16", "bf16x4", 3, torch.float32):
        with pytest.raises(ValueError):
            m.set_f32_gemm_mode(bad)
    with pytest.raises(NotImplementedError, match="bf16x6"):
        m.set_f32_gemm_mode("bf16x6")
    assert m._path() == "f32" and m._packed == "kept"
    # inert under the f16 compute dtype, remembered, acting again afterwards; set_compute_dtype keeps its values and errors
    m.set_compute_dtype(torch.float16)
    m._packed = "f16 blob"
    assert m.set_f32_gemm_mode("bf16x3")._path() == "f16" and m._packed == "f16 blob"
    assert m.set_compute_dtype(torch.float32)._path() == "bf16x3" and m._packed is None
    for bad in (torch.bfloat16, torch.float64, None, "float16", "bf16x3"):
        with pytest.raises(ValueError):
            m.set_compute_dtype(bad)
    # .half() keeps its meaning: fp16 parameters, then the selected products
    h = HiFiGANGenerator(hg.AttrDict(cfg)).set_f32_gemm_mode("bf16x3").half()
    assert next(h.parameters()).dtype == torch.float16 and h._path() == "bf16x3" and h._compute_dtype == torch.float32
    # a config the library refuses is refused here, by name, and the mode stays
    m.set_f32_gemm_mode("f32")
    m._cfg.resblock_kernel_sizes[0] = 13
    with pytest.raises(NotImplementedError, match="resblock_kernel_sizes"):
        m.set_f32_gemm_mode("bf16x3")
    assert m._path() == "f32" and m._f32_gemm_mode == "f32"
    # load_model hands the mode on
    sd = synthetic.hifigan_state_dict(cfg, seed=9)
    path = os.path.join(str(tmp_path), "g_00001000")
    torch.save({"generator": synthetic.to_torch(sd)}, path)
    with open(os.path.join(str(tmp_path), "config.json"), "w") as f:
        json.dump(cfg, f)
    gen, _ = load_hifigan(path, device="cpu", f32_gemm_mode="bf16x3")
    assert gen._path() == "bf16x3" and gen._compute_dtype == torch.float32 and next(gen.parameters()).dtype == torch.float32
    gen, _ = load_hifigan(path, device="cpu")
    assert gen._path() == "f32"
    with pytest.raises(_lib.HipLibraryError):
        gen.set_f32_gemm_mode("bf16x3")(torch.zeros(1, cfg["num_mels"], 4))      # CPU tensors raise in every mode


@pytest.mark.parametrize("name", SHORT)
def test_bf16x3_restatement_is_inside_the_fp32_bounds_and_faults_are_far_outside(name):
    cfg, sd, z = _case(name)
    ref_linf = float(z["ref_fp32_vs_fp64"][1])
    out = _restated(name)
    assert out.shape == z["audio"].shape and out.dtype == np.float32 and np.isfinite(out).all()
    err, linf = rms_rel_err(out, z["audio"]), _linf(out, z["audio"])
    rec = {"case": name, "what": "restatement vs fp32 golden", "rel_rms": err, "linf": linf, "linf_over_ref": linf / ref_linf,
           "bound_rel_rms": WAVE_TOL, "bound_linf": LINF_FACTOR * ref_linf, "faults_linf_over_ref": {}}
    for what, terms in FAULTS.items():
        bad = h3.generator_np(cfg, sd, z["mel"], terms=terms)
        rec["faults_linf_over_ref"][what] = _linf(bad, z["audio"]) / ref_linf
    _log(rec)
    assert err < WAVE_TOL
    assert linf < LINF_FACTOR * ref_linf
    for what, ratio in rec["faults_linf_over_ref"].items():
        assert ratio > FAULT_FACTOR * LINF_FACTOR, what


# --------------------------------------------------------------------------- on the GPU ----
def _check_golden(name, against_restatement=True):
    cfg, sd, z = _case(name)
    ref_linf = float(z["ref_fp32_vs_fp64"][1])
    m = _model(cfg, sd).set_f32_gemm_mode("bf16x3")
    with torch.no_grad():
        out = m(torch.from_numpy(z["mel"]).to("cuda:0"))
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == z["audio"].shape
    out = out.cpu().numpy()
    err, linf = rms_rel_err(out, z["audio"]), _linf(out, z["audio"])
    rec = {"case": name, "what": "hip bf16x3 vs fp32 golden", "config": str(z["config"]), "batch": int(z["mel"].shape[0]),
           "frames": int(z["mel"].shape[2]), "rel_rms": err, "linf": linf, "linf_over_ref": linf / ref_linf,
           "bound_rel_rms": WAVE_TOL, "bound_linf": LINF_FACTOR * ref_linf}
    if against_restatement:
        want = _restated(name)
        rec["vs_restatement_rel_rms"], rec["vs_restatement_linf"] = rms_rel_err(out, want), _linf(out, want)
        rec["vs_restatement_linf_over_ref"] = rec["vs_restatement_linf"] / ref_linf
    _log(rec)
    assert np.isfinite(out).all()
    assert err < WAVE_TOL
    assert linf < LINF_FACTOR * ref_linf
    if against_restatement:
        assert rec["vs_restatement_linf"] < LINF_FACTOR * ref_linf


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHORT)
def test_hifigan_bf16x3_matches_reference_golden(name):
    _check_golden(name)


@pytest.mark.gpu
def test_hifigan_bf16x3_matches_reference_golden_full_length():
    _check_golden("v1_full_length", against_restatement=False)


@pytest.mark.gpu
@pytest.mark.parametrize("key,batch,frames", [("toy_rate4", 2, 3), ("toy_rb1", 3, 13), ("v3", 1, 67), ("toy_rb2", 2, 300)])
def test_hifigan_bf16x3_odd_lengths(key, batch, frames):
    """A 3-frame call, T % 4 != 0, a ragged last tile: against the restatement, under the L-inf bound of the golden of the same
    config (and the RMS bound)."""
    cfg = synthetic.HIFIGAN_CONFIGS[key]
    _, _, z = _case(key)
    ref_linf = float(z["ref_fp32_vs_fp64"][1])
    sd = synthetic.hifigan_state_dict(cfg, seed=int(z["seed"]))
    mel = synthetic.synthetic_mel(batch, frames, cfg["num_mels"], seed=500 + frames)
    want = h3.generator_np(cfg, sd, mel)
    m = _model(cfg, sd).set_f32_gemm_mode("bf16x3")
    with torch.no_grad():
        out = m(torch.from_numpy(mel).to("cuda:0")).cpu().numpy()
    err, linf = rms_rel_err(out, want), _linf(out, want)
    _log({"case": f"{key} B={batch} T={frames}", "what": "hip bf16x3 vs restatement", "rel_rms": err, "linf": linf,
          "linf_over_ref": linf / ref_linf, "bound_rel_rms": WAVE_TOL, "bound_linf": LINF_FACTOR * ref_linf})
    assert out.shape == want.shape and np.isfinite(out).all()
    assert err < WAVE_TOL and linf < LINF_FACTOR * ref_linf


@pytest.mark.gpu
def test_hifigan_bf16x3_batch_item_equals_single_call_bit_for_bit():
    """Narrow block shapes: item i of a B=16 call equals the B=1 call on the same mel bit for bit, and two calls of one shape are
    bit-identical."""
    cfg, sd, _ = _case("v1")
    m = _model(cfg, sd).set_f32_gemm_mode("bf16x3")
    mel = torch.from_numpy(synthetic.synthetic_mel(16, 21, 80, seed=77)).to("cuda:0")
    with torch.no_grad():
        full = m(mel).clone()
        again = m(mel).clone()
        assert torch.equal(full, again)
        for i in (0, 7, 15):
            one = m(mel[i:i + 1]).clone()
            print(f"item {i}: L-inf {_linf(full[i:i + 1].cpu().numpy(), one.cpu().numpy()):.3e}")
            assert torch.equal(full[i:i + 1], one)
    assert torch.isfinite(full).all()


@pytest.mark.gpu
def test_hifigan_bf16x3_wide_block_shapes_equal_the_narrow_ones_bit_for_bit():
    """The wide shapes engage from HG_NARROW_BELOW = 1024 workgroups (the launch rule of hifigan_bf16x3.hip is hifigan.hip's).
    toy_rate4 at B=64 x 4096 frames: conv_pre (64 rows, 256-column tiles) starts 1 x 16 x 64 = 1024 workgroups -> 64 x 256; ups.0
    (128 rows, 128-column tiles) 1 x 32 x 64 = 2048 -> 128 x 128.  A single item starts 16 / 32 and stays narrow."""
    cfg, sd, _ = _case("toy_rate4")
    B, T = 64, 4096
    assert (T + 255) // 256 * B >= 1024 and (T + 127) // 128 * B >= 1024 and (T + 127) // 128 < 1024
    m = _model(cfg, sd).set_f32_gemm_mode("bf16x3")
    mel = torch.from_numpy(synthetic.synthetic_mel(B, T, cfg["num_mels"], seed=64)).to("cuda:0")
    with torch.no_grad():
        full = m(mel)
        for i in (0, 63):
            one = m(mel[i:i + 1])
            assert torch.equal(full[i:i + 1], one), i
    assert torch.isfinite(full).all()


@pytest.mark.gpu
def test_hifigan_bf16x3_is_its_own_path_and_the_other_two_switch_back_bit_for_bit():
    cfg, sd, z = _case("v1")
    mel = torch.from_numpy(z["mel"]).to("cuda:0")
    never = _model(cfg, sd)
    m = _model(cfg, sd)
    with torch.no_grad():
        base = never(mel).clone()
        h_before = m.set_compute_dtype(torch.float16)(mel).clone()
        o32 = m.set_compute_dtype(torch.float32)(mel).clone()
        o3 = m.set_f32_gemm_mode("bf16x3")(mel).clone()
        h_after = m.set_compute_dtype(torch.float16)(mel).clone()              # the mode is inert here
        back = m.set_compute_dtype(torch.float32).set_f32_gemm_mode("f32")(mel).clone()
    assert o3.dtype == torch.float32 and not torch.equal(o3, o32)
    e32, e3 = rms_rel_err(o32.cpu().numpy(), z["audio"]), rms_rel_err(o3.cpu().numpy(), z["audio"])
    print(f"fp32 mode {e32:.3e}, bf16x3 mode {e3:.3e} ({e3 / e32:.1f} x)")
    assert e3 > e32
    assert torch.equal(back, base) and torch.equal(o32, base)
    assert torch.equal(h_before, h_after) and not torch.equal(h_before, o3)


@pytest.mark.gpu
def test_hifigan_bf16x3_half_parameters_fp16_in_fp16_out_and_repack():
    cfg, sd, z = _case("toy_rb2")
    m16 = _model(cfg, sd).half().set_f32_gemm_mode("bf16x3")
    dtype = next(m16.parameters()).dtype
    assert dtype == torch.float16
    mel16 = torch.from_numpy(z["mel"]).to("cuda:0").to(dtype)
    sd_rounded = {k: v.astype(np.float16).astype(np.float32) for k, v in sd.items()}
    m32 = _model(cfg, sd_rounded).set_f32_gemm_mode("bf16x3")
    with torch.no_grad():
        out16 = m16(mel16)
        out32 = m32(mel16.float())
        assert out16.dtype == torch.float16 and out32.dtype == torch.float32
        assert torch.equal(out16, out32.half())
        a = m32(mel16.float()).clone()
        m32.conv_post.bias.add_(0.25)
        b = m32(mel16.float()).clone()
        m32.load_state_dict(synthetic.to_torch(sd_rounded))
        c = m32(mel16.float()).clone()
    assert not torch.equal(a, b)
    assert torch.equal(a, c)
