"""CPU side of the forward (analysis) direction of the glow.py-class WaveGlow: the numpy restatement against the reference's own
forward outputs (tests/golden/make_golden_waveglow_forward.py), the ABI of the new entry points, the host-side size queries, the
refusals of ``WaveGlow.forward`` / ``nll`` by name, and ``WaveGlowLoss`` against the formula.  The device side is
test_waveglow_forward_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import waveglow_forward_restatement as fr
from conftest import REPO, rms_rel_err
from cookietts_amd import WaveFlow, WaveGlow, WaveGlowLoss, _lib, synthetic
from test_oracle_golden import ORACLE_TOL

FORWARD_SYMBOLS = ("ctts_waveglow_forward_packed_bytes", "ctts_waveglow_pack_forward_mix", "ctts_waveglow_forward_workspace_bytes",
                   "ctts_waveglow_forward_spk_f32", "ctts_waveglow_flow_forward_f32")


# ------------------------------------------------------------------ the restatement against the reference ----
@pytest.mark.parametrize("name", fr.CASES)
def test_fp32_restatement_matches_reference_forward_goldens(name):
    """z, log_s, log_det_W and the loss of the reference's own forward, at the bound test_oracle_golden.py gives the numpy oracle
    (RMS relative; log det and the loss: relative).  NaN where the reference says NaN (det W_k < 0: every synthetic model but the
    "posdet" case), and there the loss is NaN too."""
    cfg, sd, mel, wave, ids, sigma = fr.case_inputs(name)
    g = fr.load_case(name)
    r = fr.forward(sd, cfg, mel, wave, ids, np.float32)
    assert r["z"].shape == g["z_ref"].shape and r["log_s"].shape == g["log_s_ref"].shape
    assert rms_rel_err(r["z"], g["z_ref"]) < ORACLE_TOL
    assert rms_rel_err(r["log_s"], g["log_s_ref"]) < ORACLE_TOL
    B, _, L = r["z"].shape
    ref_ld = g["log_det_W_ref"].astype(np.float64)
    got_ld = B * L * r["logdet"].astype(np.float64)
    assert np.array_equal(np.isnan(got_ld), np.isnan(ref_ld))
    fin = ~np.isnan(ref_ld)
    assert name != fr.POSDET or fin.all()
    # log det of a near-orthonormal matrix is a small difference of O(1) terms: absolute, against B L
    assert np.all(np.abs(got_ld[fin] - ref_ld[fin]) <= ORACLE_TOL * B * L)
    loss = fr.loss(r, cfg["n_group"], sigma)
    assert np.isnan(loss) == np.isnan(float(g["loss_ref"]))
    if name == fr.POSDET:
        assert abs(loss - float(g["loss_ref"])) <= ORACLE_TOL * abs(float(g["loss_ref"]))
    # the stored float64 values: the reference sits at fp32 rounding distance from them, and so does the fp32 run
    assert rms_rel_err(g["z_f64"], g["z_ref"]) < ORACLE_TOL and rms_rel_err(g["log_s_f64"], g["log_s_ref"]) < ORACLE_TOL
    assert float(g["z_linf32"]) > 0 and float(g["log_s_linf32"]) > 0


@pytest.mark.parametrize("name", fr.GOLDENS)
def test_reference_forward_recovers_the_noise_its_infer_drew(name):
    """The fixtures agree with the infer goldens they extend: the reference's forward z is the z_scaled its infer started from."""
    g = fr.load_case(name)
    z_scaled = np.load(os.path.join(fr.wr.GOLDEN, f"waveglow_{name}.npz"))["z_scaled"]
    assert rms_rel_err(g["z_ref"], z_scaled) < ORACLE_TOL


def test_fixture_sizes():
    for name in fr.CASES:
        assert os.path.getsize(fr.case_path(name)) <= 1 << 20, name


# ------------------------------------------------------------------------------------------- ABI ----
def test_forward_entry_points_in_header_exports_and_signatures(hip_lib_path):
    header = open(os.path.join(REPO, "include", "cookietts_hip.h")).read()
    assert "#define CTTS_ABI_VERSION 7" in header
    declared = set(re.findall(r"\b(ctts_[a-z0-9_]+)\s*\(", header))
    handle = C.CDLL(hip_lib_path)
    assert handle.ctts_abi_version() == 7
    for sym in FORWARD_SYMBOLS:
        assert sym in declared and sym in _lib.SIGNATURES, sym
        assert hasattr(handle, sym), f"library does not export {sym}"
    # the whole-model entry: 14 arguments - config, two blobs, mel, audio, ids, z, log_s, sums, batch, frames, workspace, bytes, stream
    assert len(_lib.SIGNATURES["ctts_waveglow_forward_spk_f32"][1]) == 14
    assert len(_lib.SIGNATURES["ctts_waveglow_flow_forward_f32"][1]) == 14


def test_forward_size_queries_run_without_gpu(hip_lib_path):
    lib = _lib.lib()
    for key in ("toy", "toy_early", "toy_hop512_g16", "full"):
        cfg = synthetic.WAVEGLOW_CONFIGS[key]
        c = WaveGlow(**cfg).c_config()
        dims = synthetic.waveglow_flow_channels(cfg)
        nb = lib.ctts_waveglow_forward_packed_bytes(C.byref(c))
        assert nb >= 4 * sum(n_rem * n_rem for n_rem, _ in dims) and nb % 256 == 0
        infer_ws = lib.ctts_waveglow_workspace_bytes(C.byref(c), 2, 9)
        ws = lib.ctts_waveglow_forward_workspace_bytes(C.byref(c), 2, 9)
        L = 9 * cfg["hop_length"] // cfg["n_group"]
        slots = 2 * (cfg["n_flows"] * -(-L // 256) + -(-cfg["n_group"] * L // 4096))       # fp64 slots of the two-stage sums
        assert infer_ws + 8 * slots <= ws <= infer_ws + 8 * slots + 2 * 256
    c = WaveGlow(**synthetic.WAVEGLOW_CONFIGS["toy"]).c_config()
    c.n_group = 6                                                     # what make_plan refuses
    assert lib.ctts_waveglow_forward_packed_bytes(C.byref(c)) == 0 and b"n_group=6" in lib.ctts_last_error()
    assert lib.ctts_waveglow_forward_workspace_bytes(C.byref(c), 2, 9) == 0 and b"n_group=6" in lib.ctts_last_error()
    c.n_group = 8
    assert lib.ctts_waveglow_forward_workspace_bytes(C.byref(c), 2, 0) == 0 and b"frames=0" in lib.ctts_last_error()
    assert lib.ctts_waveglow_forward_workspace_bytes(C.byref(c), 0, 9) == 0 and b"batch=0" in lib.ctts_last_error()
    # a multispeaker config without ids is refused by the entry itself, before it touches a pointer's target
    m = WaveGlow(**synthetic.WAVEGLOW_CONFIGS["toy_spk_rezero"])
    c = m.c_config()
    one = C.c_void_p(256)                                              # non-NULL, never dereferenced: the check comes first
    rc = lib.ctts_waveglow_forward_spk_f32(C.byref(c), one, one, one, one, None, one, None, None, 1, 4, one, 1 << 40, None)
    assert rc == -1 and b"speaker ids" in lib.ctts_last_error()


# ------------------------------------------------------------------------------------ refusals ----
def _model(key="toy"):
    return WaveGlow(**synthetic.WAVEGLOW_CONFIGS[key]).eval()


def test_forward_refusals_by_name():
    m = _model()
    mel = torch.zeros(1, 80, 4)
    audio = torch.zeros(1, 4 * 256)
    with pytest.raises(ValueError, match="audio is None"):
        m.forward(mel)
    with pytest.raises(ValueError, match="audio is None"):
        m.nll(mel, None)
    with pytest.raises(ValueError, match=r"frames \* hop_length = 1024"):
        m(mel, audio[:, :1000])
    with pytest.raises(ValueError, match=r"frames \* hop_length = 1024"):
        m.nll(mel, torch.zeros(1, 1025))
    for dtype, word in ((torch.bfloat16, "'bf16'"), (torch.float16, "'f16'"), ("bf16x3", "'bf16x3'")):
        m.set_compute_dtype(dtype)
        with pytest.raises(NotImplementedError, match=word):
            m(mel, audio)
    m.set_compute_dtype(torch.float32)
    m.train()
    with pytest.raises(NotImplementedError, match="no backward pass"):
        m(mel, audio)
    with torch.no_grad():                      # a training-mode model without grad passes this refusal: the next one is the device's
        with pytest.raises(_lib.HipLibraryError, match="needs the model on a GPU"):
            m(mel, audio)
    m.eval()
    with pytest.raises(_lib.HipLibraryError, match="needs the model on a GPU"):
        m(mel, audio)
    cfg = dict(synthetic.WAVEGLOW_CONFIGS["toy"], spect_scaling=True)
    with pytest.raises(NotImplementedError, match="spect_scaling"):
        WaveGlow(**cfg).eval()(mel, audio)
    assert m._fwd is None and m._packed is None          # nothing was packed on the way to a refusal


def test_ax_core_forward_keeps_its_refusal():
    key = next(iter(synthetic.WAVEGLOW_AX_CONFIGS))
    m = WaveFlow(**synthetic.WAVEGLOW_AX_CONFIGS[key])
    with pytest.raises(NotImplementedError):
        m.forward(torch.zeros(1, 80, 4), torch.zeros(1, 1024))


# --------------------------------------------------------------------------------- WaveGlowLoss ----
@pytest.mark.parametrize("sigma", [1.0, 0.6])
def test_waveglow_loss_equals_the_float64_formula(sigma):
    rng = np.random.default_rng(5)
    B, G, L = 3, 8, 50
    z = rng.standard_normal((B, G, L))
    log_s = [rng.standard_normal((B, h, L)) * 0.2 for h in (4, 4, 3, 2)]
    log_det = [float(v) for v in rng.standard_normal(4) * 7.0]
    want = (np.sum(z * z) / (2 * sigma * sigma) - sum(np.sum(s) for s in log_s) - sum(log_det)) / z.size
    out = (torch.from_numpy(z), [torch.from_numpy(s) for s in log_s], [torch.tensor(v, dtype=torch.float64) for v in log_det])
    got = WaveGlowLoss(sigma)(out)
    assert got.dim() == 0 and abs(float(got) - want) <= 1e-12 * abs(want)
    assert float(out[2][0]) == log_det[0]                  # (the reference's class sums INTO its input, glow.py:59; this one does not)
    got32 = WaveGlowLoss(sigma)((out[0].float(), [s.float() for s in out[1]], [v.float() for v in out[2]]))
    assert got32.dtype == torch.float32 and abs(float(got32) - want) <= 1e-5 * abs(want)
