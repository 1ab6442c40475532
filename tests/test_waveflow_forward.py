"""WaveFlow analysis pass, CPU side: the float64 restatement against the reference's recorded outputs (tests/golden/
waveflow_forward_<name>.npz, made by make_golden_waveflow_forward.py), the perturbation hooks, the host refusals in their order, and
``WaveFlowLoss``.  The device checks are in test_waveflow_forward_gpu.py."""
import os

import numpy as np
import pytest
import torch

import ax_cond_f64_restatement as acr
import waveflow_core_f64_restatement as wcr
import waveflow_forward_restatement as fr
from conftest import REPO, rms_rel_err
from cookietts_amd import WaveFlow, WaveFlowLoss, _lib, synthetic

WAVE_TOL = 1e-3
ORACLE_TOL = 5e-6            # test_waveflow's bound for a float64 oracle against the reference's fp32 output
FACTOR, EPS32 = acr.FACTOR, acr.EPS32

_R64 = {}


def _r64(name):
    """the float64 restatement of a fixture case, computed once and left unchanged"""
    if name not in _R64:
        cfg, sd, melp, audio, ids, sigma, z = fr.case_inputs(name)
        _R64[name] = fr.forward(sd, cfg, melp, audio, ids, np.float64)
    return _R64[name]


@pytest.mark.parametrize("name", fr.RECOVERS_Z)
def test_restatement_recovers_the_golden_noise(name):
    """forward(mel + 1 frame, inverse_full) is the z ``infer`` was given: the early-output order of forward is the order inverse consumes."""
    z = fr.case_inputs(name)[6]
    d = rms_rel_err(_r64(name)["z"], z)
    print(f"{name}: float64 restatement vs the infer fixture's z {d:.2e}")
    assert d < WAVE_TOL


@pytest.mark.parametrize("name", fr.CASES)
def test_restatement_matches_reference_golden(name):
    """The float64 restatement against the reference's own forward tuple and loss, and the fixture's float64 arrays decode to it."""
    g = np.load(fr.case_path(name))
    r = _r64(name)
    sigma = float(g["sigma"])
    B, T = g["z_ref"].shape
    assert rms_rel_err(r["z"], g["z_ref"]) < ORACLE_TOL
    assert rms_rel_err(r["log_s_sum"], g["log_s_sum_ref"]) < ORACLE_TOL
    scale = np.abs(r["sums"]).sum(axis=1) + np.abs(r["logdet_w"]).sum()
    assert np.all(np.abs(r["logdet"] - g["logdet_ref"]) <= ORACLE_TOL * scale)
    assert abs(r["logdet_w"].sum() - float(g["logdet_w_sum_ref"])) <= ORACLE_TOL * np.abs(r["logdet_w"]).sum()
    loss, per_item = fr.loss(r["z"], r["logdet"], sigma)
    assert abs(loss - float(g["loss_ref"])) <= ORACLE_TOL * max(1.0, abs(loss)) and per_item.shape == (B,)
    # the stored float64 side is this restatement
    z64 = fr.unpack_delta(g["z_f64_delta16"], g["z_f64_scale"], g["z_ref"])
    assert np.abs(z64 - r["z"]).max() <= float(g["z_f64_scale"])
    ls64 = fr.unpack_delta(g["log_s_f64_delta16"], g["log_s_f64_scale"], g["log_s_f32"])
    assert np.abs(ls64 - r["log_s"]).max() <= float(g["log_s_f64_scale"])
    assert np.allclose(g["sums_f64"], r["sums"], rtol=1e-12, atol=1e-12) and np.allclose(g["logdet_f64"], r["logdet"], rtol=1e-12)
    assert g["z_e32"].shape == (fr.case_inputs(name)[0]["n_group"],) and g["log_s_e32"].shape == (r["log_s"].shape[1],)
    if name == "author_toy":            # pre-emphasis 0.9: the reference's PreEmphasis reflects at t = 0, so forward is not inverse^-1
        assert rms_rel_err(r["z"], fr.case_inputs(name)[6]) > 0.05


# hook -> the fixture case that is meant to catch it
CAUGHT_BY = {'row_shift': "toy", 'affine_dir': "toy_odd", 'mix_transpose': "toy_conv_mixlast", 'early_order': "toy_conv_early",
             'tap_row': "toy_dilations_h", 'halo': "full_short", 'preemph_edge': "author_toy"}


def test_every_hook_has_a_case():
    assert set(CAUGHT_BY) == set(fr.PERTURBATIONS)
    assert fr.case_inputs(CAUGHT_BY['preemph_edge'])[0]["preempthasis"]
    assert len(set(fr.active_rows(fr.case_inputs(CAUGHT_BY['early_order'])[0]))) >= 3     # two early chunks: their order can be wrong
    assert wcr.params(fr.case_inputs(CAUGHT_BY['mix_transpose'])[0])["conv_mix"]


@pytest.mark.parametrize("hook", fr.PERTURBATIONS)
def test_every_perturbation_matters(hook):
    """On the reference-pinned float64 result alone: each mistake moves z by far more than the GPU bound on its case."""
    name = CAUGHT_BY[hook]
    cfg, sd, melp, audio, ids, sigma, _ = fr.case_inputs(name)
    g = np.load(fr.case_path(name))
    G = cfg["n_group"]
    y64 = wcr.rows_of(_r64(name)["z"], G)
    bound = FACTOR * np.maximum(g["z_e32"], 4 * EPS32 * np.abs(y64).max(axis=(0, 2)))
    bad = fr.forward(sd, cfg, melp, audio, ids, np.float64, perturb=(hook,))
    d = np.abs(wcr.rows_of(bad["z"], G) - y64).max(axis=(0, 2))
    ratio = d / bound
    print(f"{hook} on {name}: largest distance / bound per row {np.array2string(ratio, precision=1)}")
    assert ratio.max() > 10, (hook, name, ratio)


# --------------------------------------------------------------------------------------------------------- refusals ----
def test_refusals_come_by_name_in_order_and_pack_nothing(monkeypatch):
    packed = []
    monkeypatch.setattr(WaveFlow, "_ensure_packed", lambda self, device: packed.append(1))
    mel, wave = torch.zeros(1, 80, 4), torch.zeros(1, 1024)
    m = WaveFlow(**synthetic.WAVEFLOW_CONFIGS["toy"])
    # 1. no backward pass: first of all, whatever else is wrong
    assert m.training
    for args in ((mel, wave), (mel, None), (mel, torch.zeros(1, 1023))):
        with pytest.raises(NotImplementedError, match="no backward pass"):
            m.forward(*args)
        with pytest.raises(NotImplementedError, match="no backward pass"):
            m.nll(*args)
    ax1d = WaveFlow(**synthetic.WAVEGLOW_AX_CONFIGS[next(iter(synthetic.WAVEGLOW_AX_CONFIGS))])
    with pytest.raises(NotImplementedError, match="no backward pass"):
        ax1d.forward(mel, None)
    # 2. the 1-D core keeps its refusal, by name, before the audio is looked at
    with pytest.raises(NotImplementedError, match="waveflow=False"):
        ax1d.eval().forward(mel, None)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="waveflow=False"):
        ax1d.train().forward(mel, wave)
    # 3. the audio
    m.eval()
    with pytest.raises(ValueError, match="audio is None"):
        m.forward(mel, None)
    with pytest.raises(ValueError, match="multiple of"):
        m.forward(mel, torch.zeros(1, 1023))
    with pytest.raises(ValueError, match="multiple of"):
        m.nll(mel, torch.zeros(1, 2, 1024))
    # 4. perceived-volume companding
    vol = WaveFlow(**dict(synthetic.WAVEFLOW_CONFIGS["toy"], preceived_vol_scaling=True)).eval()
    with pytest.raises(ValueError, match="audio is None"):
        vol.forward(mel, None)
    with pytest.raises(NotImplementedError, match="preceived_vol_scaling"):
        vol.forward(mel, wave)
    assert not packed
    # 5. a CPU model: the existing refusal, for [B, T] and [B, 1, T] alike
    monkeypatch.undo()
    for a in (wave, wave[:, None, :]):
        with pytest.raises(_lib.HipLibraryError, match="needs the model on a GPU"):
            m.forward(mel, a)
    assert m._fwd is None and m._packed is None


def test_knob_and_entry_points_are_declared(hip_lib_path):
    assert _lib.TUNING_BITS_EXT["CTTS_WF_FWD_ROWWISE"] == 31 and "CTTS_WF_FWD_ROWWISE" not in _lib.TUNING_BITS     # bits 0-30 are taken
    hdr = open(os.path.join(REPO, "include", "cookietts_hip.h")).read()
    assert "31 CTTS_WF_FWD_ROWWISE" in hdr and "CTTS_WF_FWD_ROWWISE" in open(os.path.join(REPO, "cookietts_amd", "csrc", "tuning.h")).read()
    os.environ.pop("CTTS_WF_FWD_ROWWISE", None)
    _lib.tuning_reload()
    assert not _lib.tuning_active("CTTS_WF_FWD_ROWWISE")
    lib = _lib.lib()
    assert lib.ctts_abi_version() == 7
    cfg = WaveFlow(**synthetic.WAVEFLOW_CONFIGS["toy"]).c_config()
    import ctypes as C
    assert lib.ctts_waveflow_forward_packed_bytes(C.byref(cfg)) == 0                      # PermuteHeight: nothing to hold
    conv = WaveFlow(**synthetic.WAVEFLOW_CONFIGS[str(np.load(fr.case_path("toy_conv_early").replace("_forward", ""))["config_key"])])
    assert lib.ctts_waveflow_forward_packed_bytes(C.byref(conv.c_config())) > 0
    inv = lib.ctts_waveflow_workspace_bytes(C.byref(cfg), 2, 1536)
    fwd = lib.ctts_waveflow_forward_workspace_bytes(C.byref(cfg), 2, 1536)
    assert fwd > inv > 0 and lib.ctts_waveflow_forward_workspace_bytes(C.byref(cfg), 2, 1537) == 0


# ------------------------------------------------------------------------------------------------------ WaveFlowLoss ----
@pytest.mark.parametrize("sigma", [1.0, 0.6])
def test_waveflow_loss_equals_the_float64_formula(sigma):
    rng = np.random.default_rng(5)
    B, T = 3, 400
    z = rng.standard_normal((B, T))
    logdet = rng.standard_normal(B) * 50
    want, _ = fr.loss(z, logdet, sigma)
    got = WaveFlowLoss(sigma)((torch.from_numpy(z).float(), torch.from_numpy(logdet).float(), torch.tensor(0.0), torch.zeros(B, 50)))
    assert got.dim() == 0 and abs(float(got) - want) <= 8 * EPS32 * max(1.0, abs(want))
