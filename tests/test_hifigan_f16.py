"""IEEE-half storage mode of the HiFi-GAN generator (``set_compute_dtype(torch.float16)`` over csrc/hifigan_f16.hip).

Fixtures: tests/golden/hgf16_<case>.npz (tests/golden/make_golden_hifigan_f16.py) hold the REFERENCE'S OWN half-mode waveform
(``remove_weight_norm(); .half()`` on the CPU, half mel) for every case of the fp32 goldens, and ``ref_half_vs_fp32`` =
(relative RMS, L-inf) of that waveform against the fp32 golden ``audio``: what the reference itself loses by running in half.

Bounds, all scaled from the reference's own half-mode error and never from the code under test:

* f16 restatement (tests/hifigan_f16_restatement.py) and the HIP half mode, each against the fp32 golden: relative RMS
  < RMS_FACTOR (2) x and L-inf < LINF_FACTOR (4) x the fixture's ``ref_half_vs_fp32``.  Two correct half evaluations that round
  at different places scatter (the restatement sits at 1.05-1.45 x the reference's half error in RMS, 0.8-1.5 x in L-inf on the
  CPU); the faults the test is for - a wrong halo column, the 0.1 slope in front of conv_post, bf16 by another name - are 7 x
  to 100 x.
* the same rounding points in bf16 are more than FORMAT_FACTOR (2.5, the project's figure) further from the golden than in f16.
* HIP half mode against the f16 restatement: the same two bounds (measured figures are printed and appended to
  profiles/r10_01_hifigan_f16_parity.jsonl; DESIGN.md quotes them).
* batch item against the single call, two calls of one shape: bit for bit - the K order of a column's sum (chunks, taps inside
  a chunk, the MFMA's own order inside a K16 step) is the same for every block shape and launch size.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, rms_rel_err
from cookietts_amd import HiFiGANGenerator, _lib, load_hifigan, synthetic
from cookietts_amd import hifigan as hg
import hifigan_f16_restatement as h16
import hifigan_restatement as hr

RMS_FACTOR = 2.0
LINF_FACTOR = 4.0
FORMAT_FACTOR = 2.5
SHIPPED = ("v1", "v2", "v3", "v1_48khz")
CASES = hr.golden_cases()
NEW_SYMBOLS = ("ctts_hifigan_packed_f16_bytes", "ctts_hifigan_pack_f16", "ctts_hifigan_workspace_f16_bytes",
               "ctts_hifigan_forward_f16")
PARITY_LOG = os.path.join(REPO, "profiles", "r10_01_hifigan_f16_parity.jsonl")


def _case(name):
    z = hr.load_case(name)
    cfg = synthetic.HIFIGAN_CONFIGS[str(z["config"])]
    z.update(np.load(os.path.join(GOLDEN, f"hgf16_{name}.npz")))
    return cfg, synthetic.hifigan_state_dict(cfg, seed=int(z["seed"])), z


def _model(cfg, sd, device="cuda:0"):
    m = HiFiGANGenerator(hg.AttrDict(cfg))
    m.load_state_dict(synthetic.to_torch(sd))
    return m.to(device).eval()


def _linf(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


# --------------------------------------------------------------------------- without a GPU ----
def test_f16_fixtures_cover_every_case():
    for name in CASES:
        z = np.load(os.path.join(GOLDEN, f"hgf16_{name}.npz"))
        gold = hr.load_case(name)["audio"]
        assert z["audio_half"].dtype == np.float16 and z["audio_half"].shape == gold.shape
        assert np.isfinite(z["audio_half"]).all()
        rel, linf = (float(v) for v in z["ref_half_vs_fp32"])
        assert 1e-4 < rel < 5e-3 and 1e-4 < linf < 1e-2                     # a bound scaled from it is neither vacuous nor zero
        assert abs(rms_rel_err(z["audio_half"], gold) - rel) < 1e-9 and abs(_linf(z["audio_half"], gold) - linf) < 1e-9


def test_f16_symbols_are_declared_bound_and_exported(hip_lib_path):
    header = open(os.path.join(REPO, "include", "cookietts_hip.h")).read()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in header and name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        assert ctypes.cast(getattr(ctypes.CDLL(hip_lib_path), name), ctypes.c_void_p).value
    assert "#define CTTS_ABI_VERSION 7" in header
    assert lib.ctts_abi_version() == 7


def test_f16_size_queries_without_gpu(hip_lib_path):
    """Weights halve and biases do not; the workspace halves (the resblock sum is stored as half like every other tensor, no
    fp32 stream is kept).  The f16 plan refuses exactly what the fp32 plan refuses, with the same word."""
    lib = _lib.lib()
    for key in SHIPPED:
        c = hg.c_config(synthetic.HIFIGAN_CONFIGS[key])
        p32, p16 = lib.ctts_hifigan_packed_bytes(ctypes.byref(c)), lib.ctts_hifigan_packed_f16_bytes(ctypes.byref(c))
        w32, w16 = lib.ctts_hifigan_workspace_bytes(ctypes.byref(c), 16, 900), lib.ctts_hifigan_workspace_f16_bytes(ctypes.byref(c), 16, 900)
        print(f"{key}: packed {p16} / {p32} = {p16 / p32:.3f}, workspace {w16} / {w32} = {w16 / w32:.3f}")
        assert 0 < p16 < 0.6 * p32
        assert 0 < w16 < 0.6 * w32

    def refused(word, **edit):
        c = hg.c_config(synthetic.HIFIGAN_CONFIGS["v1"])
        for k, v in edit.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        assert lib.ctts_hifigan_packed_bytes(ctypes.byref(c)) == 0 and word in lib.ctts_last_error()
        assert lib.ctts_hifigan_packed_f16_bytes(ctypes.byref(c)) == 0
        assert word in lib.ctts_last_error(), lib.ctts_last_error()
        assert lib.ctts_hifigan_workspace_f16_bytes(ctypes.byref(c), 1, 10) == 0
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
    assert lib.ctts_hifigan_workspace_f16_bytes(ctypes.byref(c), 0, 10) == 0 and b"batch" in lib.ctts_last_error()
    assert lib.ctts_hifigan_workspace_f16_bytes(ctypes.byref(c), 1, 0) == 0 and b"frames" in lib.ctts_last_error()
    # every config the fp32 plan accepts, the f16 plan accepts (toys included)
    for key, cfg in synthetic.HIFIGAN_CONFIGS.items():
        c = hg.c_config(cfg)
        assert (lib.ctts_hifigan_packed_bytes(ctypes.byref(c)) > 0) == (lib.ctts_hifigan_packed_f16_bytes(ctypes.byref(c)) > 0), key


def test_f16_forward_refuses_bad_arguments_before_any_launch(hip_lib_path):
    """Every check of ctts_hifigan_forward_f16 / _pack_f16 is host code in front of the first launch: the pointers below are
    never dereferenced (no GPU is needed, none is touched)."""
    lib = _lib.lib()
    c = hg.c_config(synthetic.HIFIGAN_CONFIGS["toy_rb1"])
    need = lib.ctts_hifigan_workspace_f16_bytes(ctypes.byref(c), 2, 8)
    assert need > 0
    fake = ctypes.c_void_p(4096)
    ok = dict(packed=fake, mel=fake, mel_ld=8, audio=fake, batch=2, frames=8, ws=fake, ws_bytes=need)

    def call(**edit):
        a = dict(ok, **edit)
        return lib.ctts_hifigan_forward_f16(ctypes.byref(c), a["packed"], a["mel"], a["mel_ld"], a["audio"], a["batch"], a["frames"],
                                            a["ws"], a["ws_bytes"], None)
    assert call(mel=None) == -1 and b"NULL" in lib.ctts_last_error()
    assert call(audio=None) == -1
    assert call(packed=None) == -1
    assert call(ws=None) == -1
    assert call(mel_ld=7) == -1 and b"mel_ld" in lib.ctts_last_error()
    assert call(batch=0) == -1 and b"batch" in lib.ctts_last_error()
    assert call(frames=0) == -1 and b"frames" in lib.ctts_last_error()
    assert call(ws_bytes=need - 2) == -3 and b"workspace" in lib.ctts_last_error()
    assert call(ws=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.ctts_last_error()
    assert call(packed=ctypes.c_void_p(4104)) == -1 and b"aligned" in lib.ctts_last_error()
    bad = hg.c_config(synthetic.HIFIGAN_CONFIGS["toy_rb1"])
    bad.resblock = 7
    assert lib.ctts_hifigan_forward_f16(ctypes.byref(bad), fake, fake, 8, fake, 2, 8, fake, need, None) == -1
    assert b"resblock" in lib.ctts_last_error()
    n = lib.ctts_hifigan_weight_floats(ctypes.byref(c))
    assert lib.ctts_hifigan_pack_f16(ctypes.byref(c), fake, n - 1, fake, None) == -1 and b"weight floats" in lib.ctts_last_error()
    assert lib.ctts_hifigan_pack_f16(ctypes.byref(c), None, n, fake, None) == -1
    assert lib.ctts_hifigan_pack_f16(ctypes.byref(c), fake, n, None, None) == -1
    assert lib.ctts_hifigan_pack_f16(ctypes.byref(bad), fake, n, fake, None) == -1


def test_set_compute_dtype_selects_and_invalidates_without_a_launch(hip_lib_path, tmp_path):
    cfg = synthetic.HIFIGAN_CONFIGS["toy_rb1"]
    m = HiFiGANGenerator(hg.AttrDict(cfg))
    assert m._compute_dtype == torch.float32
    m._packed, m._ws = "stale", {"k": 1}
    assert m.set_compute_dtype(torch.float16) is m and m._compute_dtype == torch.float16
    assert m._packed is None and m._ws == {}                                     # blob and workspaces are per format
    assert all(p.dtype == torch.float32 for p in m.parameters())                 # independent of the parameter dtype
    m._packed = "kept"
    m.set_compute_dtype(torch.float16)                                           # no change: nothing is thrown away
    assert m._packed == "kept"
    assert m.set_compute_dtype(torch.float32) is m
    assert m._compute_dtype == torch.float32 and m._packed is None
    for bad in (torch.bfloat16, torch.float64, None, "float16"):
        with pytest.raises(ValueError):
            m.set_compute_dtype(bad)
    assert m._compute_dtype == torch.float32
    # .half() keeps its meaning: fp16 parameters, fp32 products
    h = HiFiGANGenerator(hg.AttrDict(cfg)).half()
    assert next(h.parameters()).dtype == torch.float16 and h._compute_dtype == torch.float32
    h.set_compute_dtype(torch.float16)
    assert next(h.float().parameters()).dtype == torch.float32 and h._compute_dtype == torch.float16   # ... and the mode its own
    # a config the library refuses in half storage is refused here, by name, and the mode stays
    m._cfg.resblock_kernel_sizes[0] = 13
    with pytest.raises(NotImplementedError, match="resblock_kernel_sizes"):
        m.set_compute_dtype(torch.float16)
    assert m._compute_dtype == torch.float32
    # load_model hands compute_dtype on
    sd = synthetic.hifigan_state_dict(cfg, seed=9)
    path = os.path.join(str(tmp_path), "g_00001000")
    torch.save({"generator": synthetic.to_torch(sd)}, path)
    with open(os.path.join(str(tmp_path), "config.json"), "w") as f:
        json.dump(cfg, f)
    gen, _ = load_hifigan(path, device="cpu", compute_dtype=torch.float16)
    assert gen._compute_dtype == torch.float16 and next(gen.parameters()).dtype == torch.float32
    gen, _ = load_hifigan(path, device="cpu")
    assert gen._compute_dtype == torch.float32
    with pytest.raises(_lib.HipLibraryError):
        gen.set_compute_dtype(torch.float16)(torch.zeros(1, cfg["num_mels"], 4))   # CPU tensors raise in either mode


@pytest.mark.parametrize("name", CASES)
def test_f16_restatement_matches_reference_golden(name):
    """The rounding points the library documents, restated on the CPU, lose no more than 2 x / 4 x what the reference's own
    half mode loses; with an 8-bit mantissa at the same points the error is more than FORMAT_FACTOR larger."""
    cfg, sd, z = _case(name)
    ref_rel, ref_linf = (float(v) for v in z["ref_half_vs_fp32"])
    out = h16.generator_np(cfg, sd, z["mel"], "f16")
    assert out.shape == z["audio"].shape and out.dtype == np.float32 and np.isfinite(out).all()
    e16, l16 = rms_rel_err(out, z["audio"]), _linf(out, z["audio"])
    eb = rms_rel_err(h16.generator_np(cfg, sd, z["mel"], "bf16"), z["audio"])
    d_rel, d_linf = rms_rel_err(out, z["audio_half"].astype(np.float32)), _linf(out, z["audio_half"])
    print(f"{name}: f16 restatement vs fp32 golden rel rms {e16:.3e} ({e16 / ref_rel:.2f} x ref half) linf {l16:.3e} "
          f"({l16 / ref_linf:.2f} x); bf16 {eb:.3e} ({eb / e16:.1f} x f16); vs the reference's half output {d_rel:.3e} / {d_linf:.3e}")
    assert e16 < RMS_FACTOR * ref_rel
    assert l16 < LINF_FACTOR * ref_linf
    assert eb > FORMAT_FACTOR * e16


def test_f16_restatement_tells_the_final_slope_apart():
    cfg, sd, z = _case("v1")
    wrong = h16.generator_np(cfg, sd, z["mel"], "f16", final_slope=0.1)
    assert rms_rel_err(wrong, z["audio"]) > 7 * RMS_FACTOR * float(z["ref_half_vs_fp32"][0])


def test_bytes_from_the_shapes():
    """The half row's HBM figure: at B=16 x 900 one C-row tensor of the 128-, 64- and 32-channel stages is 236 MB in half and
    the call moves roughly 40 GB."""
    cfg = synthetic.HIFIGAN_CONFIGS["v1"]
    assert 128 * 900 * 64 * 2 * 16 == 235_929_600
    total = 16 * h16.generator_bytes(cfg, 900, 2)
    assert 30e9 < total < 50e9
    assert 1.9 < h16.generator_bytes(cfg, 900, 4) / h16.generator_bytes(cfg, 900, 2) <= 2.0


# --------------------------------------------------------------------------- on the GPU ----
def _check_f16_golden(name):
    cfg, sd, z = _case(name)
    ref_rel, ref_linf = (float(v) for v in z["ref_half_vs_fp32"])
    m = _model(cfg, sd).set_compute_dtype(torch.float16)
    with torch.no_grad():
        out = m(torch.from_numpy(z["mel"]).to("cuda:0"))
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == z["audio"].shape
    out = out.cpu().numpy()
    want = h16.generator_np(cfg, sd, z["mel"], "f16")
    err, linf = rms_rel_err(out, z["audio"]), _linf(out, z["audio"])
    r_err, r_linf = rms_rel_err(out, want), _linf(out, want)
    rec = {"case": name, "config": str(z["config"]), "batch": int(z["mel"].shape[0]), "frames": int(z["mel"].shape[2]),
           "vs_fp32_golden_rel_rms": err, "vs_fp32_golden_linf": linf, "ref_half_vs_fp32_rel_rms": ref_rel,
           "ref_half_vs_fp32_linf": ref_linf, "rel_rms_over_ref": err / ref_rel, "linf_over_ref": linf / ref_linf,
           "vs_f16_restatement_rel_rms": r_err, "vs_f16_restatement_linf": r_linf,
           "bound_rel_rms": RMS_FACTOR * ref_rel, "bound_linf": LINF_FACTOR * ref_linf}
    print(json.dumps(rec))
    try:
        with open(PARITY_LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass
    assert np.isfinite(out).all()
    assert err < RMS_FACTOR * ref_rel
    assert linf < LINF_FACTOR * ref_linf
    assert r_err < RMS_FACTOR * ref_rel
    assert r_linf < LINF_FACTOR * ref_linf


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASES if "full_length" not in n])
def test_hifigan_f16_matches_reference_golden(name):
    _check_f16_golden(name)


@pytest.mark.gpu
def test_hifigan_f16_is_not_the_fp32_path_and_switches_back_bit_for_bit():
    cfg, sd, z = _case("v1")
    mel = torch.from_numpy(z["mel"]).to("cuda:0")
    never = _model(cfg, sd)
    m = _model(cfg, sd)
    with torch.no_grad():
        base = never(mel).clone()
        o32 = m(mel).clone()
        o16 = m.set_compute_dtype(torch.float16)(mel).clone()
        back = m.set_compute_dtype(torch.float32)(mel).clone()
    assert o16.dtype == torch.float32 and not torch.equal(o16, o32)
    e32, e16 = rms_rel_err(o32.cpu().numpy(), z["audio"]), rms_rel_err(o16.cpu().numpy(), z["audio"])
    print(f"fp32 mode {e32:.3e}, f16 mode {e16:.3e} ({e16 / e32:.0f} x)")
    assert e16 > FORMAT_FACTOR * e32
    assert torch.equal(back, base) and torch.equal(o32, base)


@pytest.mark.gpu
def test_hifigan_f16_batch_item_equals_single_call_bit_for_bit():
    """Item i of a B=16 call equals the B=1 call on the same mel bit for bit: items never see each other, and the K order of a
    sum does not change with the block shape the launch size selects.  Two calls of one shape are bit-identical too."""
    cfg, sd, z = _case("v1")
    m = _model(cfg, sd).set_compute_dtype(torch.float16)
    mel = torch.from_numpy(synthetic.synthetic_mel(16, 21, 80, seed=77)).to("cuda:0")
    with torch.no_grad():
        full = m(mel).clone()
        again = m(mel).clone()
        assert torch.equal(full, again)
        for i in (0, 7, 15):
            one = m(mel[i:i + 1]).clone()
            d = _linf(full[i:i + 1].cpu().numpy(), one.cpu().numpy())
            print(f"item {i}: L-inf {d:.3e}")
            assert torch.equal(full[i:i + 1], one)
    assert torch.isfinite(full).all()


@pytest.mark.gpu
def test_hifigan_f16_wide_block_shapes_equal_the_narrow_ones_bit_for_bit():
    """The wide shapes engage from HG_NARROW_BELOW = 1024 workgroups (hg_launch in hifigan_plan.h, one rule for the three
    formats).  toy_rate4 at B=64 x 4096 frames: conv_pre (64 rows, 256-column tiles) starts 1 x 16 x 64 = 1024 workgroups ->
    64 x 256; ups.0 (128 rows, 128-column tiles) 1 x 32 x 64 = 2048 -> 128 x 128.  A single item starts 16 / 32 and stays
    narrow.  Same packed weights and same K order either way, so the items are equal bit for bit."""
    cfg, sd, _ = _case("toy_rate4")
    B, T = 64, 4096
    assert (T + 255) // 256 * B >= 1024 and (T + 127) // 128 * B >= 1024 and (T + 127) // 128 < 1024
    m = _model(cfg, sd).set_compute_dtype(torch.float16)
    mel = torch.from_numpy(synthetic.synthetic_mel(B, T, cfg["num_mels"], seed=64)).to("cuda:0")
    with torch.no_grad():
        full = m(mel)
        for i in (0, 63):
            one = m(mel[i:i + 1])
            assert torch.equal(full[i:i + 1], one), i
    assert torch.isfinite(full).all()


@pytest.mark.gpu
@pytest.mark.parametrize("key,batch,frames", [("toy_rate4", 2, 3), ("toy_rb1", 3, 13), ("v3", 1, 67), ("toy_rb2", 2, 300)])
def test_hifigan_f16_odd_lengths(key, batch, frames):
    """A 3-frame call, T % 8 != 0, a ragged last tile (T prod(u) not a multiple of the 128 / 256-column tiles): against the f16
    restatement under the bounds of the case of the same config."""
    cfg = synthetic.HIFIGAN_CONFIGS[key]
    _, _, z = _case(key)
    ref_rel, ref_linf = (float(v) for v in z["ref_half_vs_fp32"])
    sd = synthetic.hifigan_state_dict(cfg, seed=int(z["seed"]))
    mel = synthetic.synthetic_mel(batch, frames, cfg["num_mels"], seed=500 + frames)
    want = h16.generator_np(cfg, sd, mel, "f16")
    m = _model(cfg, sd).set_compute_dtype(torch.float16)
    with torch.no_grad():
        out = m(torch.from_numpy(mel).to("cuda:0")).cpu().numpy()
    err, linf = rms_rel_err(out, want), _linf(out, want)
    print(f"{key} B={batch} T={frames}: vs f16 restatement rel rms {err:.3e} linf {linf:.3e}")
    assert out.shape == want.shape and np.isfinite(out).all()
    assert err < RMS_FACTOR * ref_rel and linf < LINF_FACTOR * ref_linf


@pytest.mark.gpu
def test_hifigan_f16_half_parameters_fp16_in_fp16_out_and_repack():
    """What the server does: ``.half()`` parameters plus the f16 mode, mel cast to the vocoder's dtype -> fp16 waveform, equal
    to the f16 mode run on the fp16-rounded parameters.  A parameter change repacks."""
    cfg, sd, z = _case("toy_rb2")
    m16 = _model(cfg, sd).half().set_compute_dtype(torch.float16)
    dtype = next(m16.parameters()).dtype
    assert dtype == torch.float16
    mel16 = torch.from_numpy(z["mel"]).to("cuda:0").to(dtype)
    sd_rounded = {k: v.astype(np.float16).astype(np.float32) for k, v in sd.items()}
    m32 = _model(cfg, sd_rounded).set_compute_dtype(torch.float16)
    with torch.no_grad():
        out16 = m16(mel16)
        out32 = m32(mel16.float())
        assert out16.dtype == torch.float16 and out32.dtype == torch.float32
        assert torch.equal(out16, out32.half())
        assert rms_rel_err(out16.float().cpu().numpy(), z["audio"]) < 2e-2
        a = m32(mel16.float()).clone()
        m32.conv_post.bias.add_(0.25)
        b = m32(mel16.float()).clone()
        m32.load_state_dict(synthetic.to_torch(sd_rounded))
        c = m32(mel16.float()).clone()
    assert not torch.equal(a, b)
    assert torch.equal(a, c)


@pytest.mark.gpu
def test_hifigan_f16_matches_reference_golden_full_length():
    _check_f16_golden("v1_full_length")
