"""WaveFlow analysis pass on the device (``WaveFlow.forward`` / ``nll``: ctts_waveflow_forward_f32 / _cond_f32) against the reference's
recorded outputs and the float64 restatement, in both launch forms: the all-rows form (one launch per WN layer over every row; the
default of C = 64 GTU dense models) and the row-wise form (``CTTS_WF_FWD_ROWWISE=1``; the only form of every other model).

Bounds: a value y of a latent row may sit ``FACTOR * max(e32, 4 * 2^-23 * max|y64|)`` from the float64 restatement, with e32 the fp32
restatement's own distance on that row (stored in the fixture, or computed live for the ragged shapes) and FACTOR =
``ax_cond_f64_restatement.FACTOR`` - the rule of ``waveflow_core_f64_restatement.row_bounds``.  z against the infer fixture's z: the
project's waveform bound, 1e-3 RMS relative.
"""
import json
import os

import numpy as np
import pytest
import torch

import ax_cond_f64_restatement as acr
import waveflow_core_f64_restatement as wcr
import waveflow_forward_restatement as fr
from conftest import REPO, rms_rel_err
from cookietts_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

WAVE_TOL = 1e-3
FACTOR = acr.FACTOR
EPS32 = acr.EPS32
PARITY_LOG = os.path.join(REPO, "profiles", "r24_01_waveflow_forward_parity.jsonl")
ALL_ROWS_BIT = 256                      # ctts_last_gemm_loop(): the all-rows layer launch
FORMS = ("all_rows", "rowwise")


def _log(rec):
    print(json.dumps(rec))
    try:
        with open(PARITY_LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


_MODELS = {}


def _model(key, seed, **override):
    from cookietts_amd.waveglow_ax import WaveGlow
    k = (key, seed, tuple(sorted(override.items())))
    if k not in _MODELS:
        cfg = dict(synthetic.WAVEFLOW_CONFIGS[key], **override)
        sd = synthetic.waveflow_state_dict(cfg, seed=seed)
        m = WaveGlow(**cfg)
        m.load_state_dict(synthetic.to_torch(sd))
        _MODELS[k] = (m.cuda().eval(), cfg, sd)
    return _MODELS[k]


def _case_model(name):
    g = np.load(os.path.join(fr.GOLDEN, f"waveflow_{name}.npz"))
    return _model(str(g["config_key"]), int(g["seed"]))


def _form(tuning, form):
    if form == "rowwise":
        tuning.set("CTTS_WF_FWD_ROWWISE", "1")
    else:
        tuning.clear("CTTS_WF_FWD_ROWWISE")


def _bound(e32, y64_rows):
    """per row (axis 1 of [B, R, L]): FACTOR * max(e32, 4 eps max|y64|)"""
    return FACTOR * np.maximum(np.asarray(e32, np.float64), 4 * EPS32 * np.abs(y64_rows).max(axis=(0, 2)))


def _row_err(got, y64_rows):
    err = np.abs(np.asarray(got, np.float64) - y64_rows)
    return np.where(np.isnan(err), np.inf, err).max(axis=(0, 2))


def _check_rows(what, tag, got_rows, y64_rows, e32):
    err, bound = _row_err(got_rows, y64_rows), _bound(e32, y64_rows)
    ratio = err / (bound / FACTOR)
    r = int(np.argmax(ratio))
    _log(dict(tag, what=what, worst_row=r, hip_linf=float(err[r]), ratio=float(ratio[r])))
    assert np.all(err <= bound), f"{tag} {what}: rows over the bound {np.nonzero(err > bound)[0].tolist()}, ratios {np.array2string(ratio, precision=2)}"


def _has_all_rows(cfg):
    """WfPlan::all_rows(): the fused layer (C = 64, GTU) with dense in-layers."""
    wn = cfg["WN_config"]
    return wn["n_channels"] == 64 and str(wn.get("gated_unit", "GTU")).upper() == "GTU" and not wn.get("seperable_conv")


def _case_cfg(name):
    return synthetic.WAVEFLOW_CONFIGS[str(np.load(os.path.join(fr.GOLDEN, f"waveflow_{name}.npz"))["config_key"])]


def _runs():
    """every fixture in every form its model has"""
    return [(n, f) for n in fr.CASES for f in (FORMS if _has_all_rows(_case_cfg(n)) else FORMS[1:])]


# ---------------------------------------------------------------------------------------------------------- a. goldens ----
@pytest.mark.parametrize("name,form", _runs(), ids=[f"{n}-{f}" for n, f in _runs()])
def test_forward_matches_reference_golden(hip_lib_path, tuning, name, form):
    cfg, sd, melp, audio, ids, sigma, z_infer = fr.case_inputs(name)
    g = np.load(fr.case_path(name))
    m, _, _ = _case_model(name)
    _form(tuning, form)
    G = cfg["n_group"]
    B, T = audio.shape
    L = T // G
    z, logdet, ldw_sum, log_s_sum, log_s = m.forward(_dev(melp), _dev(audio), speaker_ids=_dev(ids), return_log_s=True)
    code = _lib.lib().ctts_last_gemm_loop()
    assert z.is_cuda and z.dtype == torch.float32 and z.shape == (B, T) and logdet.shape == (B,) and ldw_sum.dim() == 0
    assert log_s_sum.shape == (B, L) and [v.shape[1] for v in log_s] == [n - 1 for n in fr.active_rows(cfg)]
    z = z.cpu().numpy()
    tag = dict(case=name, form=form, loop=code)
    d_ref = rms_rel_err(z, g["z_ref"])
    _log(dict(tag, what="z_rms_rel_vs_reference", value=d_ref))
    assert d_ref < WAVE_TOL
    if name in fr.RECOVERS_Z:
        assert rms_rel_err(z, z_infer) < WAVE_TOL                          # the latent infer was given
    z64 = fr.unpack_delta(g["z_f64_delta16"], g["z_f64_scale"], g["z_ref"])
    _check_rows("z", tag, wcr.rows_of(z, G), wcr.rows_of(z64, G), g["z_e32"])
    ls64 = fr.unpack_delta(g["log_s_f64_delta16"], g["log_s_f64_scale"], g["log_s_f32"])
    _check_rows("log_s", tag, torch.cat(log_s, 1).cpu().numpy(), ls64, g["log_s_e32"])
    lss64 = fr.unpack_delta(g["log_s_sum_f64_delta16"], g["log_s_sum_f64_scale"], g["log_s_sum_ref"])
    _check_rows("log_s_sum", tag, log_s_sum.cpu().numpy()[:, None], lss64[:, None], [float(g["log_s_sum_e32"])])
    # logdet, loss: the rule of test_waveglow_forward_gpu._loss_bound
    ld_bound = max(FACTOR * float(g["logdet_e32"]), 4.0 * EPS32 * float(np.abs(g["logdet_f64"]).max()))
    ld_err = float(np.abs(logdet.cpu().numpy().astype(np.float64) - g["logdet_f64"]).max())
    out = m.nll(_dev(melp), _dev(audio), speaker_ids=_dev(ids), sigma=sigma)
    loss_bound = max(FACTOR * float(g["loss_e32"]), 4.0 * EPS32 * abs(float(g["loss_f64"])))
    loss_err = abs(float(out["loss"]) - float(g["loss_f64"]))
    _log(dict(tag, what="logdet_loss", logdet_err=ld_err, logdet_bound=ld_bound, loss_err=loss_err, loss_bound=loss_bound))
    assert ld_err <= ld_bound and loss_err <= loss_bound
    assert out["loss"].dim() == 0 and out["per_item"].shape == (B,) and out["per_item"].dtype == torch.float64
    n2 = float(sum(n * n for n in fr.active_rows(cfg)))
    assert abs(float(ldw_sum) - float(g["logdet_w_sum_ref"])) <= B * L * n2 * EPS32
    assert bool(code & ALL_ROWS_BIT) == (form == "all_rows")               # h. the form the case is about really ran


# ------------------------------------------------------------------------------------------- b. ragged shapes, live ----
RAGGED = [("toy", 1, 1), ("toy", 3, 5), ("toy", 2, 9), ("toy", 1, 17), ("toy_dilations_h", 2, 33)]
_LIVE = {}


def _live(key, B, F):
    """One float64 and one float32 restatement per shape, shared by the forms."""
    if (key, B, F) not in _LIVE:
        m, cfg, sd = _model(key, 41)
        rng = np.random.default_rng(1000 * B + F)
        melp = np.pad(synthetic.synthetic_mel(B, F, cfg["n_mel_channels"], seed=F), ((0, 0), (0, 0), (0, 1))).astype(np.float32)
        audio = (0.3 * rng.standard_normal((B, F * cfg["hop_length"]))).astype(np.float32)
        _LIVE[(key, B, F)] = (melp, audio, fr.forward(sd, cfg, melp, audio, None, np.float64),
                              fr.forward(sd, cfg, melp, audio, None, np.float32))
    return _LIVE[(key, B, F)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key,B,F", RAGGED, ids=[f"{k}-B{b}-F{f}" for k, b, f in RAGGED])
def test_ragged_shapes_match_live_float64(hip_lib_path, tuning, key, B, F, form):
    m, cfg, sd = _model(key, 41)
    melp, audio, r64, r32 = _live(key, B, F)
    G = cfg["n_group"]
    _form(tuning, form)

    def run():
        z, logdet, _, lss, ls = m.forward(_dev(melp), _dev(audio), return_log_s=True)
        return z.cpu().numpy(), torch.cat(ls, 1).cpu().numpy(), lss.cpu().numpy(), logdet.cpu().numpy()
    z, ls, lss, logdet = run()
    code = _lib.lib().ctts_last_gemm_loop()
    assert bool(code & ALL_ROWS_BIT) == (form == "all_rows")
    tag = dict(case=f"{key}-B{B}-F{F}", form=form, loop=code)
    _check_rows("z", tag, wcr.rows_of(z, G), wcr.rows_of(r64["z"], G), fr.row_linf(wcr.rows_of(r32["z"], G), wcr.rows_of(r64["z"], G)))
    _check_rows("log_s", tag, ls, r64["log_s"], fr.row_linf(r32["log_s"], r64["log_s"]))
    _check_rows("log_s_sum", tag, lss[:, None], r64["log_s_sum"][:, None],
                [np.abs(r32["log_s_sum"].astype(np.float64) - r64["log_s_sum"]).max()])
    e_ld = np.abs(r32["logdet"].astype(np.float64) - r64["logdet"]).max()
    assert np.abs(logdet - r64["logdet"]).max() <= max(FACTOR * e_ld, 4 * EPS32 * np.abs(r64["logdet"]).max())
    # the same workspace again after a call at another geometry: same bits (a stale halo or row would show)
    other = (0.3 * np.random.default_rng(3).standard_normal((B + 1, 2 * cfg["hop_length"]))).astype(np.float32)
    m.forward(_dev(np.pad(synthetic.synthetic_mel(B + 1, 2, cfg["n_mel_channels"], seed=2), ((0, 0), (0, 0), (0, 1))).astype(np.float32)), _dev(other))
    z2, ls2, lss2, _ = run()
    assert np.array_equal(z2.view(np.uint32), z.view(np.uint32)) and np.array_equal(ls2.view(np.uint32), ls.view(np.uint32))
    assert np.array_equal(lss2.view(np.uint32), lss.view(np.uint32))


# ------------------------------------------------------------------------- c. determinism, batch independence; d. sums ----
@pytest.mark.parametrize("form", FORMS)
def test_bits_repeat_and_items_do_not_see_their_batch(hip_lib_path, tuning, form):
    m, cfg, sd = _model("toy_conv_early", 7)
    B, F = 4, 3
    melp = np.pad(synthetic.synthetic_mel(B, F, seed=5), ((0, 0), (0, 0), (0, 1))).astype(np.float32)
    audio = (0.3 * np.random.default_rng(9).standard_normal((B, F * cfg["hop_length"]))).astype(np.float32)
    _form(tuning, form)

    def run(sl):
        z, logdet, _, lss, ls = m.forward(_dev(melp[sl]), _dev(audio[sl]), return_log_s=True)
        out = m.nll(_dev(melp[sl]), _dev(audio[sl]), sigma=0.8)
        return (z.cpu().numpy().view(np.uint32), torch.cat(ls, 1).cpu().numpy().view(np.uint32), lss.cpu().numpy().view(np.uint32),
                logdet.cpu().numpy().view(np.uint32), out["per_item"].cpu().numpy().view(np.uint64)), (z, ls, out)
    first, (z, ls, out) = run(slice(0, B))
    again, _ = run(slice(0, B))
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    for b in range(B):
        one, _ = run(slice(b, b + 1))
        assert all(np.array_equal(a[b:b + 1], o) for a, o in zip(first, one)), b
    # d. per_item against the float64 sum of the returned fp32 values; loss == mean(per_item) to fp32 rounding
    zz = z.cpu().numpy().astype(np.float64)
    lsum = sum(v.cpu().numpy().astype(np.float64).sum(axis=(1, 2)) for v in ls)
    labs = sum(np.abs(v.cpu().numpy().astype(np.float64)).sum(axis=(1, 2)) for v in ls)
    L = zz.shape[1] // cfg["n_group"]
    ldw = float(m._log_det_W(m._fwd[2], L).double().sum())               # fp32 on the host, as the reference takes it
    T = zz.shape[1]
    want = ((zz ** 2).sum(axis=1) / (2 * 0.8 * 0.8) - lsum - ldw) / T
    mag = ((zz ** 2).sum(axis=1) / (2 * 0.8 * 0.8) + labs + abs(ldw)) / T
    per_item = out["per_item"].cpu().numpy()
    assert np.all(np.abs(per_item - want) <= 1e-10 * mag), (per_item, want)
    assert abs(float(out["loss"]) - per_item.mean()) <= 2 * EPS32 * abs(per_item.mean())


# ------------------------------------------------------------------------------------------------------ e. round trip ----
ROUND_TRIPS = [(k, {}, f) for k in ("toy", "toy_conv_early", "toy_permute_mixfirst_early") for f in FORMS] + \
              [("author_toy", {"preempthasis": None}, "rowwise")]          # separable: the row-wise form is its only one


@pytest.mark.parametrize("key,over,form", ROUND_TRIPS, ids=[f"{k}{'-nopre' if o else ''}-{f}" for k, o, f in ROUND_TRIPS])
def test_round_trip_through_infer_from_noise(hip_lib_path, tuning, key, over, form):
    m, cfg, sd = _model(key, 13, **over)
    B, F = 2, 4
    n_in = cfg["n_mel_channels"] * (2 if cfg.get("use_logvar_channels") else 1)
    mel = synthetic.synthetic_mel(B, F, n_in, seed=17).astype(np.float32)
    melp = np.pad(mel, ((0, 0), (0, 0), (0, 1)))
    x = (0.3 * np.random.default_rng(23).standard_normal((B, F * cfg["hop_length"]))).astype(np.float32)
    ids = _dev(np.array([3, 17], np.int64)) if m.multispeaker else None
    _form(tuning, form)
    z = m.forward(_dev(melp), _dev(x), speaker_ids=ids)[0]
    back = m.infer_from_noise(_dev(mel), z, speaker_ids=ids).cpu().numpy()
    want = x[:, :(F - 1) * cfg["hop_length"]]
    assert back.shape == want.shape and rms_rel_err(back, want) < WAVE_TOL
    if m.multispeaker:
        wrong = m.infer_from_noise(_dev(mel), z, speaker_ids=_dev(np.array([5, 250], np.int64))).cpu().numpy()
        assert np.isfinite(wrong).all() and rms_rel_err(wrong, want) > WAVE_TOL


# --------------------------------------------------------------------------- f. split-bf16 mode; g. infer undisturbed ----
def test_bf16x3_mode_recovers_the_golden_noise(hip_lib_path):
    cfg, sd, melp, audio, ids, sigma, z_infer = fr.case_inputs("toy")
    from cookietts_amd.waveglow_ax import WaveGlow
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(sd))
    m = m.cuda().eval().set_f32_gemm_mode("bf16x3")
    z = m.forward(_dev(melp), _dev(audio))[0]
    assert not (_lib.lib().ctts_last_gemm_loop() & ALL_ROWS_BIT)           # a split mode takes the row-wise form
    assert rms_rel_err(z.cpu().numpy(), z_infer) < WAVE_TOL


def test_infer_is_undisturbed_and_repack_drops_the_forward_blob(hip_lib_path):
    cfg, sd, melp, audio, ids, sigma, z_infer = fr.case_inputs("toy_conv_early")
    from cookietts_amd.waveglow_ax import WaveGlow
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(sd))
    m = m.cuda().eval()
    mel = melp[:, :, :-1]
    before = m.infer_from_noise(_dev(mel), _dev(z_infer)).cpu().numpy()
    assert m._fwd is None                                                  # a model that only infers packs nothing new
    m.forward(_dev(melp), _dev(audio))
    assert m._fwd is not None and m._fwd[1] is not None
    after = m.infer_from_noise(_dev(mel), _dev(z_infer)).cpu().numpy()
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    m.repack()
    assert m._fwd is None
