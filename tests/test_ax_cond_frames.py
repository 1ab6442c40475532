"""The conditioning path of the ``waveglow_ax.WaveGlow`` family (``WaveGlow._cond_frames``: 30-odd launches of small kernels and
conv-GEMMs per call) element by element against the float64 restatement of tests/ax_cond_f64_restatement.py.

CPU (unmarked): the restatement is pinned before it judges anything - its fp32 run against ``oracle.waveflow_oracle`` stage by
stage on every config below (ORACLE_TOL, the bound test_waveflow.py uses between oracle and reference), its interpolation
positions bit for bit against torch's fp32 kernels (one-hot probes: the output IS the weight), its float64 sums against torch
float64 on the CPU (1e-12), and its purposely broken forms against its own bound (the tests bite).

GPU: every flow's rows ``[:, :, PAD:PAD+T]`` of ``_cond_frames`` against float64.  Bound of a comparison:
``max(FACTOR * e32, 4 * 2^-23 * max|y64|)`` with e32 the L-inf distance of the restatement's fp32 run from its float64 run on
the same inputs - never a figure of the code under test.  ``alpha`` / ``upsample_net.res_weight`` are set to 0.8 so that the conv
stacks reach the output unattenuated.  A failure names the flow, item, row and column.  Every comparison prints and appends
(case, HIP L-inf, e32, ratio, bound) to profiles/r21_01_ax_cond_frames_parity.jsonl.

``transposed_conv_residual_linear=False`` cannot be constructed: F.interpolate rejects ``align_corners`` with 'nearest'
(glow_ax.py:231 raises ValueError) and the constructor refuses it for that reason (pinned below).  The 'nearest' residual that
``_cond_frames`` is written for is reached by building the linear model and clearing the flag on its parameter holder; the
restatement computes 'nearest' by scale factor.

Measured on the MI355X (the 63 comparisons of the jsonl): the HIP L-inf is 0.57 ... 2.07 x e32 (largest: ax untts_toy with
the rezero row tail at Fr = 2, 2.07; ax toy_wn_tconv at Fr = 129, 2.05 - both behind transposed convs, where a phase convolution
sums its taps in another order than the scatter of the restatement; nothing above 1.3 where no transposed conv runs).  By
the text-side test's rule - 4 x the largest measured ratio, rounded up to a power of two - FACTOR is 16 here; the floor
4 * 2^-23 * max|y64| is below FACTOR * e32 in every case, and the largest error is 0.13 of its bound.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ax_cond_f64_restatement as acr
from conftest import REPO, rms_rel_err
from cookietts_amd import synthetic
from oracle import waveflow_oracle as wf

FACTOR = 16                      # started at acr.FACTOR = 8; 4 x the largest measured ratio (2.07), rounded up to a power of two - see
assert FACTOR <= 32              # the module docstring.  Beyond 32 an error is a finding, not a tolerance
ORACLE_TOL = 5e-6                # test_waveflow.ORACLE_TOL
PARITY_LOG = os.path.join(REPO, "profiles", "r21_01_ax_cond_frames_parity.jsonl")
IDS = np.array([0, 511, 42], np.int64)
B = 3
FRAMES = (2, 9, 129)             # 129: the frame-rate convs cross the 128-column tile; x 6 = 774 columns behind the transposed convs

# (family, config, variant)
CASES = [("waveflow", k, None) for k in ("author_toy", "untts_toy", "toy_groupconv", "toy_wn_tconv", "toy_wn_tconv_crop",
                                         "toy_upsample_first")]
CASES += [("ax", k, None) for k in ("notebook_toy", "untts_toy", "toy_groupconv", "toy_groupconv_dense", "toy_sigmoid_vol",
                                    "toy_wn_tconv", "toy_wn_tconv_crop")]
CASES += [("waveflow", "toy_upsample_first", "nearest"), ("ax", "untts_toy", "nearest"),             # resample_rows mode 2 by factor
          ("waveflow", "toy_upsample_first", "rezero_tail"), ("ax", "untts_toy", "rezero_tail"),     # rezero over the row tail
          # the MODEL's net cropped (factor 6 == hop / n_group) in front of the 2-D core.  3 + 3
          # columns by efficient_model_ax._upsample_mels (ax:177-181), where the 2-D WN's own rule (3 + 4) finds no crop: the
          # host code took the rule from the core and refused these shapes until this test
          ("waveflow", "toy_upsample_first", "model_crop")]
CASE_IDS = ["-".join(str(p) for p in c if p) for c in CASES]


def _cfg(case):
    family, key, variant = case
    cfg = (synthetic.WAVEFLOW_CONFIGS if family == "waveflow" else synthetic.WAVEGLOW_AX_CONFIGS)[key]
    if variant == "nearest":
        cfg = dict(cfg, transposed_conv_residual_linear=False)
    elif variant == "model_crop":
        cfg = dict(cfg, hop_length=48, win_length=192)
        assert _tconv_factor(cfg) == (6, 6)
    elif variant == "rezero_tail":
        # more output channels than the net reads: rows above min(in, out) get the rezero weight and no residual
        c_in = synthetic.waveflow_cond_channels(cfg)[1]
        cfg = dict(cfg, transposed_conv_res_rezero=True, transposed_conv_output_dim=c_in + 16)
        assert cfg["transposed_conv_output_dim"] > c_in
    return cfg


@functools.lru_cache(maxsize=None)
def _state(case):
    """(cfg, state dict) with the rezero weights near 1: at the synthetic 0.3 / 0.4 (0.01 ... 0.03 at init) the conv stacks would
    reach the output attenuated, and so would a mistake in them."""
    cfg = _cfg(case)
    make = synthetic.waveflow_state_dict if case[0] == "waveflow" else synthetic.waveglow_ax_state_dict
    sd = make(cfg, seed=31)
    for key in ("alpha", "upsample_net.res_weight"):
        if key in sd:
            sd[key] = np.array([0.8], np.float32)
    if case[2] == "rezero_tail":
        assert "upsample_net.res_weight" in sd
    return cfg, sd


def _n_in(cfg):
    return cfg["n_mel_channels"] * (2 if cfg.get("use_logvar_channels") else 1)


def _tconv_factor(cfg):
    """(factor of the transposed convs or 0, hop // n_group)."""
    wn = cfg["WN_config"]
    scales = cfg.get("transposed_conv_scales") if cfg.get("upsample_first") is True else wn.get("transposed_conv_scales")
    return (int(np.prod(scales)) if scales else 0), cfg["hop_length"] // cfg["n_group"]


def _lengths(cfg, Fr):
    """The latent lengths a case runs at: crop configs with no column to crop and with 2 + 2, interpolating ones one frame short,
    the rest (frame-rate output: L is not read) once."""
    factor, per_frame = _tconv_factor(cfg)
    if factor and factor == per_frame:
        return [Fr * per_frame, (Fr - 1) * per_frame]
    return [(Fr - 1) * per_frame]


@functools.lru_cache(maxsize=None)
def _reference(case, Fr, L):
    """Inputs, float64 / float32 restatements and the bound of one case, computed once and never written to again."""
    cfg, sd = _state(case)
    mel = synthetic.synthetic_mel(B, Fr, _n_in(cfg), seed=100 + Fr)
    y64, T = acr.cond_frames(sd, cfg, mel, IDS, L, np.float64)
    y32, T32 = acr.cond_frames(sd, cfg, mel, IDS, L, np.float32)
    assert T == T32 and y64[0].dtype == np.float64 and y32[0].dtype == np.float32
    factor, per_frame = _tconv_factor(cfg)
    assert T == (L if factor else Fr)
    C2L = 2 * cfg["WN_config"]["n_channels"] * cfg["WN_config"]["n_layers"]
    y64, y32 = np.stack(y64), np.stack(y32)                                     # [n_flows, B, 2C*n_layers, T]
    assert y64.shape == (cfg["n_flows"], B, C2L, T)
    e32, bound = acr.bound(y32, y64, FACTOR)
    for a in (mel, y64, y32):
        a.setflags(write=False)
    return dict(cfg=cfg, sd=sd, mel=mel, y64=y64, y32=y32, T=T, e32=e32, bound=bound)


def _perturbations(case, L, Fr):
    """name -> (cfg, speaker ids, perturb set): those of the five mistakes (module docstring of the restatement) that CAN happen
    on this case."""
    cfg, _ = _state(case)
    wn = cfg["WN_config"]
    factor, per_frame = _tconv_factor(cfg)
    out = {}
    if cfg["speaker_embed"] or wn.get("speaker_embed_dim", 0):
        out["speaker"] = (cfg, np.array([IDS[0], IDS[0], IDS[2]]), ())
    if factor and factor == per_frame and L != Fr * per_frame:
        out["crop_shift"] = (cfg, IDS, ("crop_shift",))
    if factor:
        out["last_frame"] = (cfg, IDS, ("last_frame",))
    if cfg.get("cond_padding_mode") == 'replicate' and cfg["cond_layers"] and cfg["cond_kernel_size"] > 1:
        out["zeros_padding"] = (dict(cfg, cond_padding_mode='zeros'), IDS, ())
    if "group_conv_output_dim" in cfg and cfg.get("group_conv_groupped", True):
        out["group_slice"] = (cfg, IDS, ("group_slice",))
    return out


def _moves(case, Fr, L):
    """name -> L-inf move of the float64 restatement under each applicable mistake."""
    ref = _reference(case, Fr, L)
    res = {}
    for name, (cfg, ids, perturb) in _perturbations(case, L, Fr).items():
        y, T = acr.cond_frames(ref["sd"], cfg, ref["mel"], ids, L, np.float64, perturb)
        assert T == ref["T"]
        res[name] = float(np.abs(np.stack(y) - ref["y64"]).max())
    return res


# ------------------------------------------------------------------------------------------ CPU: the restatement itself ----
def _oracle_stages(cfg, sd, mel, ids, L):
    """The same stages out of oracle.waveflow_oracle's functions (fp32) -> dict of stage name -> array."""
    sd = {k: np.asarray(v, np.float32) for k, v in sd.items()}
    wn = cfg["WN_config"]
    out = {"model_cond": wf.model_cond(sd, cfg, mel, ids)}
    cond = out["model_cond"]
    if cfg.get("upsample_first") is True:
        scales = cfg["transposed_conv_scales"]
        out["upsample_net"] = wf.transposed_upsample_net(sd, "upsample_net", cond, scales, cfg["transposed_conv_kernel_size"], True,
                                                         cfg.get("transposed_conv_residual", False),
                                                         cfg.get("transposed_conv_residual_linear", False))
        cond = out["to_latent"] = wf.to_latent_length(out["upsample_net"], L, int(np.prod(scales)) != cfg["hop_length"] // cfg["n_group"],
                                                      False)
    per_flow = wf.flow_conds(sd, cfg, cond)
    act = wf.activation(wn.get("cond_activation_func", 'none'), wn.get("negative_slope"))
    for k in range(cfg["n_flows"]):
        p = f"WN.{k}.WN"
        out[f"flow_cond.{k}"] = spect = per_flow[k]
        if wn.get("speaker_embed_dim", 0):
            emb = sd[p + ".speaker_embed.weight"][ids]
            spect = np.concatenate([spect, np.repeat(emb[:, :, None], spect.shape[2], axis=2)], axis=1)
        for l in range(wn["cond_layers"]):
            spect = wf.conv1d_same(spect, wf._w(sd, f"{p}.cond_layers.{l}"), sd[f"{p}.cond_layers.{l}.bias"],
                                   wn.get("cond_padding_mode", 'zeros'))
            if act is not None and (wn.get("cond_out_activation_func", True) or l != wn["cond_layers"] - 1):
                spect = act(spect).astype(np.float32)
        out[f"wn_stack.{k}"] = spect
        if cfg.get("upsample_first") is not True and f"{p}.upsample_net.t_convs.0.weight" in sd:
            spect = wf.wn_upsample(sd, p, wn, spect, L, cfg["hop_length"] // cfg["n_group"], bool(cfg.get("waveflow", True)))
        out[f"frames.{k}"] = spect
    return out


def _own_stages(cfg, sd, mel, ids, L, dtype):
    wn = cfg["WN_config"]
    out = {"model_cond": acr.model_cond(sd, cfg, mel, ids, dtype)}
    if cfg.get("upsample_first") is True:
        scales = cfg["transposed_conv_scales"]
        out["upsample_net"] = acr.transposed_upsample_net(sd, "upsample_net", out["model_cond"], scales,
                                                          cfg["transposed_conv_kernel_size"], True,
                                                          cfg.get("transposed_conv_residual", False),
                                                          cfg.get("transposed_conv_residual_linear", False), dtype)
    cond = out["to_latent"] = acr.shared_cond(sd, cfg, mel, ids, L, dtype)
    per_flow = acr.flow_conds(sd, cfg, cond, dtype)
    no_up = dict(cfg, upsample_first=True)                                    # the stack alone: the WN does not upsample
    for k in range(cfg["n_flows"]):
        out[f"flow_cond.{k}"] = per_flow[k]
        out[f"wn_stack.{k}"] = acr.wn_stage(sd, no_up, k, per_flow[k], ids, L, bool(cfg.get("waveflow", True)), dtype)[0]
    frames, _ = acr.cond_frames(sd, cfg, mel, ids, L, dtype)
    for k in range(cfg["n_flows"]):
        out[f"frames.{k}"] = frames[k]
    return out


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_float32_restatement_matches_the_oracle_stage_by_stage(case):
    cfg, sd = _state(case)
    for Fr in (2, 9):
        for L in _lengths(cfg, Fr):
            mel = synthetic.synthetic_mel(B, Fr, _n_in(cfg), seed=100 + Fr)
            want = _oracle_stages(cfg, sd, mel, IDS, L)
            got = _own_stages(cfg, sd, mel, IDS, L, np.float32)
            for name, w in want.items():
                g = got[name]
                assert g.dtype == np.float32 and g.shape == w.shape, (name, g.dtype, g.shape, w.shape)
                err = rms_rel_err(g, w)
                assert err < ORACLE_TOL, (name, Fr, L, err)
            # float64 really is float64, and close to the fp32 run
            got64 = _own_stages(cfg, sd, mel, IDS, L, np.float64)
            for name, w in want.items():
                assert got64[name].dtype == np.float64 and rms_rel_err(got64[name], w) < ORACLE_TOL, name


def test_the_nearest_residual_is_refused_at_construction_like_the_reference():
    """glow_ax.py:231: F.interpolate(..., mode='nearest', align_corners=False) raises ValueError, so the model cannot run."""
    from cookietts_amd.waveglow_ax import WaveGlow
    with pytest.raises(ValueError, match="align_corners"):
        F.interpolate(torch.zeros(1, 1, 4), scale_factor=2, mode='nearest', align_corners=False)
    with pytest.raises(NotImplementedError, match="nearest"):
        WaveGlow(**_cfg(("waveflow", "toy_upsample_first", "nearest")))


T_INS = (1, 2, 7, 129)
FACTORS = (2, 3, 6, 30)


def _one_hot_weights(pos, n_in):
    """What an fp32 linear interpolation of the n_in one-hot rows gives with these positions: row j, column n holds
    l0[n] * (i0[n] == j) + l1[n] * (i1[n] == j) - products by 0 / 1 are exact, one fp32 addition."""
    i0, i1, l0, l1 = pos
    j = np.arange(n_in)[:, None]
    return (l0[None, :] * (i0[None, :] == j).astype(np.float32) + l1[None, :] * (i1[None, :] == j).astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("n_in", T_INS)
def test_interpolation_positions_and_values_match_torch_cpu(n_in, factor):
    rng = np.random.default_rng(1000 * n_in + factor)
    x = rng.standard_normal((2, 3, n_in))
    x32 = x.astype(np.float32)
    eye = torch.eye(n_in, dtype=torch.float32)[None]
    n_out = n_in * factor
    forms = {
        "align_corners": (acr.positions_align_corners(n_in, n_out), dict(size=n_out, mode='linear', align_corners=True),
                          lambda v, dt: acr.lerp_align_corners(v, n_out, dt)),
        "linear_scale": (acr.positions_linear_scale(n_in, factor), dict(scale_factor=factor, mode='linear', align_corners=False),
                         lambda v, dt: acr.interp_scale(v, factor, True, dt)),
    }
    for name, (pos, kw, fn) in forms.items():
        i0, i1, l0, l1 = pos
        assert all(a.dtype == np.float32 for a in (l0, l1)) and len(i0) == n_out
        assert i0.min() >= 0 and i1.max() <= n_in - 1 and ((i1 == i0) | (i1 == i0 + 1)).all()
        # positions: torch's fp32 kernel on one-hot rows hands out its own weights - identical bits
        probe = F.interpolate(eye, **kw)[0].numpy()
        assert probe.shape == (n_in, n_out)
        assert np.array_equal(probe.view(np.uint32), _one_hot_weights(pos, n_in).view(np.uint32)), name
        # fp32 run against torch fp32: the same weights, a sum of two products (fused or not)
        got32 = fn(x32, np.float32)
        t32 = F.interpolate(torch.from_numpy(x32), **kw).numpy()
        tol32 = 2.0 ** -23 * (l0 * np.abs(x32[..., i0]) + l1 * np.abs(x32[..., i1]))
        assert got32.dtype == np.float32 and (np.abs(got32.astype(np.float64) - t32) <= tol32).all(), name
        # float64 values.  First only that the restatement really combines THESE weights in double: the same expression written in
        # torch float64 (nearly a copy of the code under check - it guards the dtype handling, nothing more)
        got64 = fn(x32, np.float64)
        xt = torch.from_numpy(x32).double()
        t64 = (torch.from_numpy(l0).double() * xt[..., torch.from_numpy(i0)] + torch.from_numpy(l1).double() * xt[..., torch.from_numpy(i1)]).numpy()
        assert got64.dtype == np.float64
        assert np.abs(got64 - t64).max() <= 1e-12 * max(np.abs(t64).max(), 1e-300), name
        # ... and torch's own float64 kernel, which takes its positions in DOUBLE: they differ from the fp32 ones by a few fp32
        # roundings of `real` (<= 4 * 2^-24 * n_in), and the interpolant is piecewise linear with slope <= max|x[i+1] - x[i]|;
        # l0 = 1 - l1 is rounded once more in fp32 (<= 2^-24 absolute, times |x[i0]|)
        own64 = F.interpolate(xt, **kw).numpy()
        slope = float(np.abs(np.diff(x32.astype(np.float64), axis=-1)).max()) if n_in > 1 else 0.0
        assert np.abs(got64 - own64).max() <= 4 * 2.0 ** -24 * n_in * slope + 2.0 ** -24 * np.abs(x32).max() + 1e-12, name
    # 'nearest' by scale factor: indices from fp32 arithmetic, values are copies - equal bits at both precisions
    idx = acr.positions_nearest_scale(n_in, factor)
    assert len(idx) == n_out and idx.min() >= 0 and idx.max() <= n_in - 1
    probe = F.interpolate(eye, scale_factor=factor, mode='nearest')[0].numpy()
    assert np.array_equal(probe.argmax(axis=0), idx) and (probe.sum(axis=0) == 1).all()
    assert np.array_equal(acr.interp_scale(x32, factor, False, np.float32),
                          F.interpolate(torch.from_numpy(x32), scale_factor=factor, mode='nearest').numpy())
    assert np.array_equal(acr.interp_scale(x, factor, False, np.float64),
                          F.interpolate(torch.from_numpy(x), scale_factor=factor, mode='nearest').numpy())


@pytest.mark.parametrize("k,s", [(4, 2), (9, 3), (4, 4)])
def test_conv_transpose1d_matches_torch_float64(k, s):
    rng = np.random.default_rng(10 * k + s)
    for T in (1, 2, 7):
        x, w, b = rng.standard_normal((3, 5, T)), rng.standard_normal((5, 7, k)), rng.standard_normal(7)
        want = F.conv_transpose1d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), stride=s, padding=(k - s) // 2).numpy()
        got = acr.conv_transpose1d(x, w, b, s, (k - s) // 2, np.float64)
        assert got.dtype == np.float64 and got.shape == want.shape == (3, 7, s * T)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert acr.conv_transpose1d(x, w, b, s, (k - s) // 2, np.float32).dtype == np.float32


@pytest.mark.parametrize("k", [1, 3, 9])
def test_conv1d_zero_and_replicate_padding_match_torch_float64(k):
    rng = np.random.default_rng(k)
    for T in (1, 2, 11):
        x, w, b = rng.standard_normal((3, 5, T)), rng.standard_normal((7, 5, k)), rng.standard_normal(7)
        xt, wt, bt = (torch.from_numpy(a) for a in (x, w, b))
        zeros = F.conv1d(xt, wt, bt, padding=k // 2).numpy()
        edge = F.conv1d(F.pad(xt, (k // 2, k // 2), mode='replicate'), wt, bt).numpy()
        for mode, want in (("zeros", zeros), ("replicate", edge)):
            got = acr.conv1d_same(x, w, b, mode, np.float64)
            assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (mode, T)
        if k > 1:
            assert np.abs(zeros - edge).max() > 1e-3                             # the two modes are told apart


def test_weight_norm_fold_matches_torch_float64():
    rng = np.random.default_rng(5)
    v, g = rng.standard_normal((6, 4, 3)), rng.standard_normal((6, 1, 1))
    want = torch._weight_norm(torch.from_numpy(v), torch.from_numpy(g), 0).numpy()
    got = acr.fold_weightnorm(g, v, np.float64)
    assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_crop_rules_follow_the_reference_slices():
    x = np.arange(2 * 3 * 12, dtype=np.float64).reshape(2, 3, 12)
    assert np.array_equal(acr.to_latent_length(x, 8, False, False, np.float64), x[:, :, 2:-2])    # ax:179-181
    assert np.array_equal(acr.to_latent_length(x, 8, False, True, np.float64), x[:, :, 2:-2])     # gax:551-553, pad 2
    assert np.array_equal(acr.to_latent_length(x, 10, False, False, np.float64), x[:, :, 1:-1])
    assert np.array_equal(acr.to_latent_length(x, 9, False, True, np.float64), x[:, :, 1:-2])     # pad 1: remainder 1
    assert np.array_equal(acr.to_latent_length(x, 12, False, True, np.float64), x)
    assert np.array_equal(acr.to_latent_length(x, 8, False, False, np.float64, ("crop_shift",)), x[:, :, 3:-1])
    with pytest.raises(AssertionError):
        acr.to_latent_length(x, 10, False, True, np.float64)                                      # pad 1 + 2 columns: 9, not 10
    assert np.array_equal(acr.to_latent_length(x, 5, True, False, np.float64), acr.lerp_align_corners(x, 5, np.float64))
    with pytest.raises(AssertionError):
        acr.to_latent_length(x, 9, False, False, np.float64)                 # 1-D, odd difference: [1:-1] leaves 10 columns
    with pytest.raises(AssertionError):
        wf.to_latent_length(x.astype(np.float32), 9, False, False)


def test_host_crop_follows_the_reference_and_refuses_what_it_cannot_crop(hip_lib_path):
    """``WaveGlow._to_latent_length`` decides the crop before it touches the device: the 1-D rule (the model's own net on both
    cores, the 1-D WN) is floor(d / 2) on both sides (ax:179-181 as Python reads it), so an odd difference is refused like
    the reference's mismatched addition; the 2-D WN's rule (gax:551-553) wants pad + pad + pad % 2 columns."""
    from cookietts_amd.waveglow_ax import WaveGlow
    m = WaveGlow(**synthetic.WAVEGLOW_AX_CONFIGS["toy_wn_tconv_crop"])

    def crop(hT, T, two_d):
        m._to_latent_length(None, 0, 1, hT, hT + 16, T, T + 16, None, False, None, two_d=two_d)       # B = 0: decides, launches nothing
    for hT, T, two_d in ((12, 12, False), (12, 8, False), (12, 10, False), (18, 12, False), (12, 12, True), (12, 8, True), (12, 9, True)):
        crop(hT, T, two_d)
    for hT, T, two_d in ((12, 9, False), (17, 12, False), (12, 11, False), (12, 10, True), (18, 12, True), (12, 13, False)):
        with pytest.raises(RuntimeError, match="cannot be cropped"):
            crop(hT, T, two_d)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_each_mistake_moves_the_reference_far_beyond_the_bound(case):
    """Non-vacuity, on the restatement alone: a wrong speaker row, a crop shifted by one column, a dropped last frame, the wrong
    padding mode and a neighbour's group slice each move the float64 result by >= 1000 x the bound of the case.  Such a broken
    restatement is what a HIP path with the same mistake would be compared with: the GPU comparison fails by the same margin
    and its message names the flow, row and column (checked here on the message)."""
    cfg, _ = _state(case)
    seen = set()
    for Fr in FRAMES[:2]:
        for L in _lengths(cfg, Fr):
            ref = _reference(case, Fr, L)
            for name, move in _moves(case, Fr, L).items():
                seen.add(name)
                assert move >= 1000 * ref["bound"], (name, Fr, L, move, ref["bound"])
    need = set()
    if cfg["speaker_embed"] or cfg["WN_config"].get("speaker_embed_dim", 0):
        need.add("speaker")
    factor, per_frame = _tconv_factor(cfg)
    if factor:
        need.add("last_frame")
        if factor == per_frame:
            need.add("crop_shift")
    assert need <= seen, (need, seen)
    # the message of a failing comparison: broken restatement against the intact one
    Fr, L = 9, _lengths(cfg, 9)[-1]
    ref = _reference(case, Fr, L)
    for name, (pcfg, ids, perturb) in _perturbations(case, L, Fr).items():
        y, _ = acr.cond_frames(ref["sd"], pcfg, ref["mel"], ids, L, np.float64, perturb)
        k = int(np.argmax([np.abs(y[i] - ref["y64"][i]).max() for i in range(cfg["n_flows"])]))
        text = acr.worst(y[k], ref["y64"][k], flow=k)
        assert f"flow {k}, item " in text and "row " in text and "column " in text and "from the end" in text
        if name == "speaker":
            assert "item 1" in text
        if name == "group_slice":
            assert k == 1


def test_every_mistake_is_covered_by_some_case():
    seen = set()
    for case in CASES:
        cfg, _ = _state(case)
        for L in _lengths(cfg, 9):
            seen |= set(_perturbations(case, L, 9))
    assert seen == {"speaker", "crop_shift", "last_frame", "zeros_padding", "group_slice"}


# ------------------------------------------------------------------------------------------------------------ GPU ----
_MODELS = {}


def _model(case):
    if case not in _MODELS:
        from cookietts_amd.waveglow_ax import WaveGlow
        cfg, sd = _state(case)
        build = dict(cfg, transposed_conv_residual_linear=True) if case[2] == "nearest" else cfg
        m = WaveGlow(**build)
        m.load_state_dict(synthetic.to_torch(sd))
        if case[2] == "nearest":
            m.upsample_net.residual_linear = False       # see the module docstring: the constructor refuses it like the reference
        m = m.cuda().eval()
        assert not m._folded
        _MODELS[case] = m
    return _MODELS[case]


@pytest.fixture(scope="module", autouse=True)
def _drop_models():
    yield
    _MODELS.clear()


def _log(rec):
    print(json.dumps(rec))
    try:
        with open(PARITY_LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def _run(m, mel, L):
    """One ``_cond_frames`` call -> (frames on the host [n_flows, B, 2C*n_layers, ld], ld, T)."""
    from cookietts_amd import _lib
    dev = torch.device("cuda", 0)
    _, ops = m._ensure_packed(dev)
    with torch.cuda.device(dev):
        frames, ld, T = m._cond_frames(ops, torch.from_numpy(np.array(mel)).to(dev), torch.from_numpy(IDS).to(dev),
                                       _lib.stream(dev), out_steps=L)
        torch.cuda.synchronize()
    return frames.cpu().numpy(), ld, T


@pytest.mark.gpu
@pytest.mark.parametrize("Fr", FRAMES)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_cond_frames_match_float64(hip_lib_path, case, Fr):
    from cookietts_amd._lib import PAD
    cfg, _ = _state(case)
    m = _model(case)
    for L in _lengths(cfg, Fr):
        ref = _reference(case, Fr, L)
        if Fr < FRAMES[-1]:
            for name, move in _moves(case, Fr, L).items():
                assert move >= 1000 * ref["bound"], (name, move, ref["bound"])
        got, ld, T = _run(m, ref["mel"], L)
        assert T == ref["T"] and got.shape == ref["y64"].shape[:3] + (ld,) and ld >= PAD + T + PAD
        rows = got[..., PAD:PAD + T]
        err = np.abs(rows.astype(np.float64) - ref["y64"])
        linf = float(np.where(np.isnan(err), np.inf, err).max())
        rec = dict(test="cond_frames", family=case[0], config=case[1], variant=case[2], frames=Fr, L=L, T=T, linf=linf,
                   e32=ref["e32"], ratio=linf / ref["e32"] if ref["e32"] else None, bound=ref["bound"], factor=FACTOR)
        _log(rec)
        assert np.isfinite(got).all(), rec
        k = int(np.argmax([np.abs(rows[i].astype(np.float64) - ref["y64"][i]).max() for i in range(cfg["n_flows"])]))
        assert linf <= ref["bound"], (rec, acr.worst(rows[k], ref["y64"][k], flow=k))
        assert not got[..., :PAD].any() and not got[..., PAD + T:].any(), "halo columns of frames are not zero"
        # another length on the same model, then the first again: same bits
        Fr2 = Fr + 3
        _run(m, synthetic.synthetic_mel(B, Fr2, _n_in(cfg), seed=7), _lengths(cfg, Fr2)[-1])
        again, ld2, T2 = _run(m, ref["mel"], L)
        assert (ld2, T2) == (ld, T) and np.array_equal(again.view(np.uint32), got.view(np.uint32))
