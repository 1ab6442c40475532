"""1-D ax WaveGlow (waveflow=False) with separable in-layers (glow_ax.py:337-348: weight-normed depthwise
Conv1d(C, C, ks, groups=C, dilation=d) then pointwise Conv1d(C, 2C, 1)): the ctts_wgax_sep_* entry points and the depthwise
operator in front of the unchanged conv-GEMM.

References: the reference's own ``infer`` / ``inverse`` outputs (tests/golden/waveglow_ax_sep_*.npz, make_golden_ax_sep.py) at
the project's waveform bound; a float64 evaluation for the depthwise operator alone; and, as a cross-check, the same weights
folded into dense in-layers (``synthetic.fold_separable``: W[o][c][t] = Wp[o][c] wd[c][t], exact in real arithmetic) run
through the dense path that existed before."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rms_rel_err
from cookietts_amd import synthetic
from oracle import waveglow_ax_oracle as ao

WAVE_TOL = 1e-3           # BASELINE.json: waveform RMS relative error (as in test_waveglow_ax.py)
ORACLE_TOL = 5e-6         # test_waveglow_ax.py's bound of the fp32 oracle against the reference's outputs
FP32_FLOOR = 2e-7         # the reference's own separable-against-folded difference is 1.3e-7 RMS relative
KEYS = ["sep_toy", "sep_k7_dil_c96", "sep_k13_merge_c160", "sep_deep", "sep_k1", "sep_notebook_toy"]
DENSE_MAX_KS = 11         # taps of a dense in-layer on the HIP path (GEMM segments)


def _load(key):
    g = np.load(os.path.join(GOLDEN, f"waveglow_ax_{key}.npz"))
    cfg = synthetic.WAVEGLOW_AX_SEP_CONFIGS[str(g["config_key"])]
    return g, cfg, synthetic.waveglow_ax_state_dict(cfg, seed=int(g["seed"]))


def _ids(g):
    return g["speaker_ids"] if "speaker_ids" in g.files else None


def _ks(cfg):
    return cfg["WN_config"]["kernel_size_w"]


# ------------------------------------------------------------------------------------------------ CPU ----
def test_module_tree_matches_reference_format():
    """The goldens were produced by loading these recipes into the reference with strict=True, so equality with the recipe
    IS equality with the reference's own state_dict keys and shapes."""
    from cookietts_amd.waveglow_ax import WaveGlow
    for key, cfg in synthetic.WAVEGLOW_AX_SEP_CONFIGS.items():
        sd = synthetic.waveglow_ax_state_dict(cfg, seed=1)
        m = WaveGlow(**cfg)
        own = m.state_dict()
        assert sorted(own) == sorted(sd), key
        assert all(tuple(own[k].shape) == sd[k].shape for k in sd), key
        has_pair = any(".in_layers.0.0." in k for k in sd)
        assert has_pair == (key != "sep_k1")                 # kernel size 1: the reference builds the dense layer
        if has_pair:
            Cc, ks = cfg["WN_config"]["n_channels"], _ks(cfg)
            assert sd["WN.0.WN.in_layers.0.0.weight_v"].shape == (Cc, 1, ks)
            assert sd["WN.0.WN.in_layers.0.1.weight_v"].shape == (2 * Cc, Cc, 1)
        m.load_state_dict(synthetic.to_torch(sd))
        m.remove_weightnorm()
        assert not any(k.endswith("weight_g") for k in m.state_dict())
    assert WaveGlow(**synthetic.WAVEGLOW_AX_SEP_CONFIGS["sep_k13_merge_c160"]).c_config_1d().kernel_size == 13
    with pytest.raises(NotImplementedError, match="wider than 11"):                  # the dense form keeps its limit
        WaveGlow(**synthetic.fold_separable({}, synthetic.WAVEGLOW_AX_SEP_CONFIGS["sep_k13_merge_c160"])[1])
    with pytest.raises(NotImplementedError, match="wider than 31"):
        WaveGlow(**synthetic.waveglow_ax_config(kernel_size_w=33, WN=dict(seperable_conv=True)))


@pytest.mark.parametrize("key", KEYS)
def test_folded_oracle_matches_reference_golden(key):
    """The unchanged dense oracle on ``fold_separable``'s weights reproduces the reference's separable outputs: pins the
    goldens and the fold helper."""
    g, cfg, sd = _load(key)
    dsd, dcfg = synthetic.fold_separable(sd, cfg)
    assert not any(".in_layers.0.0." in k for k in dsd) and not dcfg["WN_config"]["seperable_conv"]
    assert cfg["WN_config"]["seperable_conv"]                                      # the caller's config is not touched
    melp = np.pad(g["mel"], ((0, 0), (0, 0), (0, 1)))
    err = rms_rel_err(ao.waveglow_ax_inverse(dsd, dcfg, g["z"], melp, _ids(g)), g["inverse_full"])
    print(f"{key}: folded dense oracle vs reference = {err:.3e}")
    assert err < ORACLE_TOL
    audio = ao.waveglow_ax_infer(dsd, dcfg, g["mel"], g["z"], speaker_ids=_ids(g))
    assert audio.shape == g["audio"].shape and rms_rel_err(audio, g["audio"]) < ORACLE_TOL


# sha256 over (key, dtype, shape, bytes) of every entry, seed 1234, computed from the recipe as it was before the separable
# keys were added: the committed goldens of these configs depend on the recipe drawing exactly what it drew
RECIPE_SHA256 = {
    "toy_conv": "162678ce3dd1a43faee00ef66baee694e363c301ea796770643ce86cf2116653",
    "toy_c96": "468df7c1b0ad2e6e2448b5f4d0aa1b5af86d486eccacee01b65820462794b3d0",
    "notebook_toy": "c7ae38eff8bbfde1944de8d7615e5cef49de16bf9c236d0a4cfcb484ebc5b4d5",
}


@pytest.mark.parametrize("key", sorted(RECIPE_SHA256))
def test_recipe_of_existing_configs_is_unchanged(key):
    sd = synthetic.waveglow_ax_state_dict(synthetic.WAVEGLOW_AX_CONFIGS[key], seed=1234)
    d = hashlib.sha256()
    for k, v in sd.items():
        d.update(k.encode()); d.update(str(v.dtype).encode()); d.update(str(v.shape).encode()); d.update(v.tobytes())
    assert d.hexdigest() == RECIPE_SHA256[key]


def test_c_abi_size_queries_and_argument_validation(hip_lib_path):
    from cookietts_amd import _lib
    lib = _lib.lib()
    for name in ("ctts_wgax_sep_packed_bytes", "ctts_wgax_sep_pack_flow", "ctts_wgax_sep_workspace_bytes",
                 "ctts_wgax_sep_inverse_f32", "ctts_depthwise_conv1d_f32"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    cfg = _lib.WgaxConfig(n_flows=48, n_group=24, n_early_every=16, n_early_size=2, n_layers=8, n_channels=256,
                          kernel_size=7, mixing=_lib.MIX_PERMUTE, mix_first=0, ignore_nan=1)
    dense, sep = lib.ctts_wgax_packed_bytes(C.byref(cfg)), lib.ctts_wgax_sep_packed_bytes(C.byref(cfg))
    # per layer 7 * 2C * C + res/skip against 2C * C + C * ks + res/skip
    assert 0 < sep < 0.4 * dense
    # one more C-row tensor: B * C * ld floats, ld = round_up(L, 256) + 2 * pad with pad = (ks/2) * 128 = 384
    B, L = 2, 11675
    ld = -(-L // 256) * 256 + 2 * 384
    ws_d, ws_s = lib.ctts_wgax_workspace_bytes(C.byref(cfg), B, 24 * L), lib.ctts_wgax_sep_workspace_bytes(C.byref(cfg), B, 24 * L)
    assert ws_d > 0 and ws_s - ws_d == B * 256 * ld * 4
    assert lib.ctts_wgax_sep_workspace_bytes(C.byref(cfg), 1, 24 * L + 1) == 0
    assert b"multiple of n_group" in lib.ctts_last_error()
    for bad in (4, 33, 1):
        c2 = _lib.WgaxConfig.from_buffer_copy(cfg)
        c2.kernel_size = bad
        assert lib.ctts_wgax_sep_packed_bytes(C.byref(c2)) == 0, bad
        assert b"kernel_size" in lib.ctts_last_error()
        assert lib.ctts_wgax_sep_workspace_bytes(C.byref(c2), 1, 24 * L) == 0, bad
    c31 = _lib.WgaxConfig.from_buffer_copy(cfg)
    c31.kernel_size = 31
    assert lib.ctts_wgax_sep_packed_bytes(C.byref(c31)) > 0 and lib.ctts_wgax_packed_bytes(C.byref(c31)) == 0
    # the operator refuses before it launches (no GPU needed): made-up, aligned, never dereferenced addresses
    x, y, w, b = (C.c_void_p(4096 * i) for i in (1, 2, 3, 4))
    E_ARG = -1
    assert lib.ctts_depthwise_conv1d_f32(x, w, b, x, 1, 32, 100, 512, 128, 3, 1, None) == E_ARG
    assert b"x == y" in lib.ctts_last_error()
    for args in ((None, w, b, y), (x, None, b, y), (x, w, None, y), (x, w, b, None)):
        assert lib.ctts_depthwise_conv1d_f32(*args, 1, 32, 100, 512, 128, 3, 1, None) == E_ARG
    assert lib.ctts_depthwise_conv1d_f32(x, w, b, y, 1, 32, 100, 512, 128, 4, 1, None) == E_ARG        # even
    assert lib.ctts_depthwise_conv1d_f32(x, w, b, y, 1, 32, 100, 512, 128, 33, 1, None) == E_ARG
    assert lib.ctts_depthwise_conv1d_f32(x, w, b, y, 1, 32, 100, 512, 128, 3, 129, None) == E_ARG      # (ks/2) * dil > pad
    assert b"> pad" in lib.ctts_last_error()
    assert lib.ctts_depthwise_conv1d_f32(x, w, b, y, 1, 32, 300, 512, 128, 3, 128, None) == E_ARG      # row too short


def test_half_storage_is_refused_and_half_falls_back_to_bf16x3(hip_lib_path):
    from cookietts_amd.vocoder import WaveGlowVocoder
    from cookietts_amd.waveglow_ax import WaveGlow
    m = WaveGlow(**synthetic.WAVEGLOW_AX_SEP_CONFIGS["sep_toy"])
    with pytest.raises(NotImplementedError, match="seperable_conv"):
        m.set_compute_dtype(torch.float16)
    assert m._compute_dtype == torch.float32
    v = WaveGlowVocoder(WaveGlow(**synthetic.WAVEGLOW_AX_SEP_CONFIGS["sep_toy"])).half()
    assert v.waveglow._compute_dtype == torch.float32 and v.waveglow._f32_gemm_mode == "bf16x3"
    d = WaveGlow(**synthetic.WAVEGLOW_AX_CONFIGS["toy_conv"]).set_compute_dtype(torch.float16)   # the dense model still does
    assert d._compute_dtype == torch.float16
    k1 = WaveGlow(**synthetic.WAVEGLOW_AX_SEP_CONFIGS["sep_k1"]).set_compute_dtype(torch.float16)  # dense layers: existing path
    assert k1._compute_dtype == torch.float16


# ------------------------------------------------------------------------------------------------ GPU ----
DW_B, DW_C, DW_L, DW_PAD, DW_LD = 2, 40, 325, 224, 1024
DW_DILS = (1, 3, 4, 7, 128, 200)
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def dw_input():
    rng = np.random.default_rng(31)
    # halo and tail columns carry values too: the operator reads them as they are
    return rng.standard_normal((DW_B, DW_C, DW_LD)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("ks", [3, 7, 13, 31])
def test_depthwise_operator_against_float64(hip_lib_path, dw_input, ks):
    """|y - y64| <= ks * 2^-23 * (|b| + sum |w| |x|): one rounding (2^-24 relative) per fma step of the specified chain, with
    a factor 2 for the growth of the partial sums' bound; nothing outside [pad, pad + L) is written."""
    from cookietts_amd import _lib
    lib = _lib.lib()
    rng = np.random.default_rng(ks)
    w = rng.standard_normal((DW_C, ks)).astype(np.float32)
    b = rng.standard_normal(DW_C).astype(np.float32)
    x = torch.from_numpy(dw_input).cuda()
    tw, tb = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
    stream = _lib.stream(x.device)
    dils = [d for d in DW_DILS if (ks // 2) * d <= DW_PAD]
    assert dils[:4] == [1, 3, 4, 7] and ((128 in dils) == (ks == 3))
    cols = DW_PAD + np.arange(DW_L)
    for dil in dils:
        y = torch.full((DW_B, DW_C, DW_LD), SENTINEL, dtype=torch.float32, device=x.device)
        _lib.check(lib.ctts_depthwise_conv1d_f32(_lib.ptr(x), _lib.ptr(tw), _lib.ptr(tb), _lib.ptr(y), DW_B, DW_C, DW_L, DW_LD,
                                                 DW_PAD, ks, dil, stream), "ctts_depthwise_conv1d_f32")
        got = y.cpu().numpy()
        outside = np.ones(DW_LD, bool)
        outside[cols] = False
        assert np.all(got[:, :, outside] == np.float32(SENTINEL)), (ks, dil)
        y64 = np.broadcast_to(b.astype(np.float64)[None, :, None], (DW_B, DW_C, DW_L)).copy()
        mag = np.abs(y64)
        for t in range(ks):
            xt = dw_input[:, :, cols + (t - ks // 2) * dil].astype(np.float64)
            wt = w[:, t].astype(np.float64)[None, :, None]
            y64 += wt * xt
            mag += np.abs(wt) * np.abs(xt)
        diff = np.abs(got[:, :, cols].astype(np.float64) - y64)
        ratio = float((diff / (ks * 2.0 ** -23 * mag)).max())
        print(f"depthwise ks={ks} dil={dil}: max |y - y64| / bound = {ratio:.3f}")
        assert ratio <= 1.0, (ks, dil)


def _model(cfg, sd):
    from cookietts_amd.waveglow_ax import WaveGlow
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(sd))
    return m.cuda().eval()


def _run(m, g):
    melp = torch.from_numpy(np.pad(g["mel"], ((0, 0), (0, 0), (0, 1)))).cuda()
    ids = None if _ids(g) is None else torch.from_numpy(_ids(g)).cuda()
    audio, _ = m.inverse(torch.from_numpy(g["z"]).cuda(), melp, speaker_ids=ids)
    return audio.numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS)
def test_hip_matches_reference_golden_and_folded_dense_path(hip_lib_path, key):
    """``inverse`` and ``infer`` against the reference's outputs; then the same weights folded into dense in-layers through the
    dense path: err_sep <= 4 * max(err_fold, 2e-7) - 2e-7 is the fp32 floor (the reference's own separable-against-folded
    difference is 1.3e-7), the factor 4 allows for the different summation orders of a K = C and a K = ks * C chain.
    The dense HIP path takes at most 11 taps, so for the 13-tap config (whose point is exactly that) the folded arm is the
    fp32 dense oracle on the folded weights instead."""
    g, cfg, sd = _load(key)
    m = _model(cfg, sd)
    assert m._sep1d == (key != "sep_k1")
    err_sep = rms_rel_err(_run(m, g), g["inverse_full"])
    ids = None if _ids(g) is None else torch.from_numpy(_ids(g)).cuda()
    audio = m.infer_from_noise(torch.from_numpy(g["mel"]).cuda(), torch.from_numpy(g["z"]).cuda(), speaker_ids=ids)
    err_infer = rms_rel_err(audio.numpy(), g["audio"])
    dsd, dcfg = synthetic.fold_separable(sd, cfg)
    if _ks(cfg) <= DENSE_MAX_KS:
        folded = _run(_model(dcfg, dsd), g)
    else:
        folded = ao.waveglow_ax_inverse(dsd, dcfg, g["z"], np.pad(g["mel"], ((0, 0), (0, 0), (0, 1))), _ids(g))
    err_fold = rms_rel_err(folded, g["inverse_full"])
    print(f"waveglow_ax {key}: separable vs reference inverse {err_sep:.3e}, infer {err_infer:.3e}; folded dense {err_fold:.3e}")
    assert audio.shape == g["audio"].shape and err_sep < WAVE_TOL and err_infer < WAVE_TOL
    assert err_sep <= 4 * max(err_fold, FP32_FLOOR)


@pytest.mark.gpu
def test_hip_batch_independence_and_repeatability(hip_lib_path):
    """Row b of a B = 3 call is bit-equal to the same utterance alone; a repeated call is bit-equal (workspace reuse: the
    depthwise tensor's halo and tail columns stay zero)."""
    g, cfg, sd = _load("sep_toy")
    m = _model(cfg, sd)
    B, Fr = 3, 13
    mel = synthetic.synthetic_mel(B, Fr, cfg["n_mel_channels"], seed=7)
    z = np.random.default_rng(8).standard_normal((B, Fr * cfg["hop_length"])).astype(np.float32) * np.float32(0.8)
    tz, tm = torch.from_numpy(z).cuda(), torch.from_numpy(np.pad(mel, ((0, 0), (0, 0), (0, 1)))).cuda()
    got, _ = m.inverse(tz, tm, return_CPU=False)
    assert torch.isfinite(got).all()
    for b in range(B):
        one, _ = m.inverse(tz[b:b + 1], tm[b:b + 1], return_CPU=False)
        assert torch.equal(one[0], got[b]), b
    again, _ = m.inverse(tz, tm, return_CPU=False)
    assert torch.equal(again, got)
    # a shorter utterance after a longer one through the same model (another workspace)
    short, _ = m.inverse(tz[:1, :5 * cfg["hop_length"]].contiguous(), tm[:1, :, :5].contiguous(), return_CPU=False)
    assert torch.isfinite(short).all() and short.shape == (1, 5 * cfg["hop_length"])


@pytest.mark.gpu
def test_hip_gemm_modes(hip_lib_path):
    """f32_gemm_mode acts on the two GEMMs of a separable layer as it does on a dense one; the depthwise stage stays fp32."""
    g, cfg, sd = _load("sep_toy")
    m = _model(cfg, sd)
    base = _run(m, g)
    for mode in ("bf16x3", "bf16x6"):
        m.set_f32_gemm_mode(mode)
        out = _run(m, g)
        err = rms_rel_err(out, g["inverse_full"])
        print(f"sep_toy {mode}: vs reference {err:.3e}")
        assert np.isfinite(out).all() and err < WAVE_TOL
    assert not np.array_equal(out, base)
    m.set_f32_gemm_mode(None)
    assert np.array_equal(_run(m, g), base)


@pytest.mark.gpu
def test_5_infer_vocoder_slot_loads_a_separable_checkpoint(hip_lib_path, tmp_path):
    """A reference-format checkpoint (train.py:128-145) of the separable notebook toy through ``load_waveglow``."""
    from cookietts_amd import load_waveglow
    from cookietts_amd.waveglow_ax import WaveGlow as WaveGlowAx
    g, cfg, sd = _load("sep_notebook_toy")
    ext = [1000 + 7 * int(i) for i in g["speaker_ids"]]
    path = str(tmp_path / "ax_sep_ckpt.pt")
    torch.save({"model": synthetic.to_torch(sd), "waveglow_config": cfg, "iteration": 7, "learning_rate": 1e-4,
                "speaker_lookup": {e: int(i) for e, i in zip(ext, g["speaker_ids"])}}, path)
    vocoder, vcfg = load_waveglow(path)
    assert isinstance(vocoder.waveglow, WaveGlowAx) and vocoder.waveglow._sep1d and vcfg["WN_config"]["seperable_conv"]
    ids = vocoder.speaker_ids_for(ext)
    mel = torch.from_numpy(g["mel"]).cuda()
    noise = torch.from_numpy(g["z"]).cuda()
    audio = vocoder(mel, speaker_ids=ids, noise=noise)
    assert audio.is_cuda and tuple(audio.shape) == (mel.shape[0], 1, (mel.shape[2] - 1) * cfg["hop_length"])
    err = rms_rel_err(audio.squeeze(1).cpu().numpy(), g["audio"])
    print(f"sep_notebook_toy through load_waveglow + vocoder(mel): rms rel err vs reference infer = {err:.3e}")
    assert err < WAVE_TOL
    vocoder.half()                                                              # separable: split bf16, not half storage
    assert vocoder.waveglow._f32_gemm_mode == "bf16x3" and next(vocoder.parameters()).dtype == torch.float32
    audio_h = vocoder(mel, speaker_ids=ids, noise=noise)
    assert rms_rel_err(audio_h.squeeze(1).cpu().numpy(), g["audio"]) < WAVE_TOL
