"""The forward (analysis) direction of the fp32 WaveGlow on the device: ``WaveGlow.forward`` / ``nll`` over
ctts_waveglow_forward_spk_f32, against the reference's own forward outputs and a float64 restatement
(tests/waveglow_forward_restatement.py, fixtures of tests/golden/make_golden_waveglow_forward.py).

Bounds.  z against the noise the reference's infer drew: the project's waveform bound, RMS relative < WAVE_TOL = 1e-3.  z and log_s
element by element (L-inf) against float64: FACTOR x the L-inf distance of the restatement's own fp32 numpy run from its float64 run
on the same inputs - stored in the fixtures, computed live for the ragged shapes, never a figure of the code under test.  FACTOR is
waveglow_f64_restatement.FACTOR = 8, measured for ONE flow; the whole model is held to the same factor here (ceiling:
test_hifigan.py's 100).  The loss: FACTOR x the fp32 restatement's loss distance with a floor of 4 fp32 ulps of the loss.
log det W_k is ill-conditioned in itself (a sum of n logs of pivots that each carry ~n eps of the elimination): B L n^2 eps32.

Every synthetic model has det W_k < 0 (see the restatement's docstring), where the reference's log_det_W and loss are NaN: NaN is
asserted there, and the finite side is held by the "toy_early_posdet" case.

Every case prints its ratios (HIP distance / fp32-restatement distance) and appends them to
profiles/r22_01_waveglow_forward_parity.jsonl.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import waveglow_f64_restatement as wr
import waveglow_forward_restatement as fr
from conftest import GOLDEN, REPO, rms_rel_err
from cookietts_amd import WaveGlow, WaveGlowLoss, _lib, synthetic

pytestmark = pytest.mark.gpu

FACTOR = wr.FACTOR
assert FACTOR <= 100.0
WAVE_TOL = 1e-3
EPS32 = float(np.finfo(np.float32).eps)
PARITY_LOG = os.path.join(REPO, "profiles", "r22_01_waveglow_forward_parity.jsonl")
H = wr.COND_HIDDEN

_MODELS = {}
_LIVE = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_models():
    yield
    _MODELS.clear()
    _LIVE.clear()


def _model(name, hip_lib_path):
    """The packed model of a case of waveglow_forward_restatement.CASES (its config and weights), on the device."""
    if name not in _MODELS:
        cfg, sd, _, _, _, _ = fr.case_inputs(name)
        m = WaveGlow(**cfg)
        m.load_state_dict(synthetic.to_torch(sd))
        _MODELS[name] = (m.cuda().eval(), cfg, sd)
    return _MODELS[name]


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype=dtype)


def _forward(m, mel, wave, ids=None):
    """WaveGlow.forward -> numpy (z, log_s concatenated, log_det_W [n_flows])."""
    z, log_s, ld = m(_dev(mel), _dev(wave), speaker_id=_dev(ids))
    assert all(not t.requires_grad for t in [z] + log_s + ld)
    return z.cpu().numpy(), torch.cat(log_s, 1).cpu().numpy(), np.array([float(v) for v in ld], np.float64)


def _log(rec):
    print(json.dumps(rec))
    try:
        with open(PARITY_LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def _check_linf(rec, z, log_s, z64, log_s64, z_linf32, log_s_linf32):
    ez, es = wr.linf(z, z64), wr.linf(log_s, log_s64)
    rec = dict(rec, z_linf=ez, log_s_linf=es, z_ref_linf32=float(z_linf32), log_s_ref_linf32=float(log_s_linf32),
               z_ratio=ez / float(z_linf32), log_s_ratio=es / float(log_s_linf32), factor=FACTOR)
    _log(rec)
    assert np.isfinite(z).all() and np.isfinite(log_s).all()
    assert ez <= FACTOR * z_linf32, rec
    assert es <= FACTOR * log_s_linf32, rec


def _loss_bound(g):
    return max(FACTOR * float(g["loss_dist32"]), 4.0 * EPS32 * abs(float(g["loss_f64"])))


def _check_log_det_and_loss(m, cfg, g, mel, wave, ids, log_det):
    """log_det_W and nll()["loss"] against the fixture: NaN exactly where the reference is NaN, else within the bounds above."""
    B, G, L = g["z_ref"].shape
    ref = g["log_det_W_ref"].astype(np.float64)
    assert np.array_equal(np.isnan(log_det), np.isnan(ref))
    fin = ~np.isnan(ref)
    n2 = np.array([n_rem * n_rem for n_rem, _ in synthetic.waveglow_flow_channels(cfg)], np.float64)
    assert np.all(np.abs(log_det[fin] - ref[fin]) <= B * L * n2[fin] * EPS32), (log_det, ref)
    out = m.nll(_dev(mel), _dev(wave), speaker_id=_dev(ids), sigma=float(g["sigma"]))
    loss = float(out["loss"])
    assert out["loss"].dim() == 0 and out["per_item"].shape == (B,) and out["per_item"].dtype == torch.float64
    assert np.isnan(loss) == np.isnan(float(g["loss_ref"]))
    if fin.all():
        rec = {"case": "loss", "loss": loss, "loss_f64": float(g["loss_f64"]), "loss_ref": float(g["loss_ref"]), "bound": _loss_bound(g)}
        _log(rec)
        assert abs(loss - float(g["loss_f64"])) <= _loss_bound(g), rec
        assert abs(loss - float(g["loss_ref"])) <= _loss_bound(g), rec
    return out


# ------------------------------------------------------------------------------- a. the reference's goldens ----
@pytest.mark.parametrize("name", fr.GOLDENS)
def test_forward_recovers_the_noise_of_the_reference_golden(hip_lib_path, name):
    m, cfg, _ = _model(name, hip_lib_path)
    _, _, mel, wave, ids, _ = fr.case_inputs(name)
    gi = np.load(os.path.join(GOLDEN, f"waveglow_{name}.npz"))
    g = fr.load_case(name)
    z, log_s, log_det = _forward(m, mel, wave, ids)
    err = rms_rel_err(z, gi["z_scaled"])
    print(f"{name}: rms rel err of z against the golden z_scaled {err:.3e}")
    assert z.shape == gi["z_scaled"].shape and err < WAVE_TOL
    assert rms_rel_err(log_s, g["log_s_ref"]) < WAVE_TOL
    _check_linf({"case": name, "test": "golden"}, z, log_s, g["z_f64"], g["log_s_f64"], g["z_linf32"], g["log_s_linf32"])
    _check_log_det_and_loss(m, cfg, g, mel, wave, ids, log_det)


def test_log_det_and_loss_match_the_reference_where_they_are_finite(hip_lib_path):
    """det W_k > 0 in every flow: the reference's log_det_W and loss are numbers, and WaveGlowLoss on the tuple gives the same."""
    name = fr.POSDET
    m, cfg, _ = _model(name, hip_lib_path)
    _, _, mel, wave, ids, sigma = fr.case_inputs(name)
    g = fr.load_case(name)
    assert np.isfinite(g["log_det_W_ref"]).all() and np.isfinite(float(g["loss_ref"]))
    z, log_s, log_det = _forward(m, mel, wave, ids)
    _check_linf({"case": name, "test": "golden"}, z, log_s, g["z_f64"], g["log_s_f64"], g["z_linf32"], g["log_s_linf32"])
    out = _check_log_det_and_loss(m, cfg, g, mel, wave, ids, log_det)
    tup = m(_dev(mel), _dev(wave))
    loss_t = float(WaveGlowLoss(sigma)(tup))                           # fp32 torch sums of ~5e3 terms: fp32 rounding of the loss
    assert abs(loss_t - float(out["loss"])) <= 16 * EPS32 * abs(loss_t)
    # views of one buffer, n_half 4 / 4 / 3 / 3 / 2
    assert [t.shape[1] for t in tup[1]] == [4, 4, 3, 3, 2]
    assert len({t.untyped_storage().data_ptr() for t in tup[1]}) == 1


# ------------------------------------------------------------------------------- b. ragged shapes, toy_early ----
def _wave(B, n, seed):
    return (np.random.default_rng(seed).standard_normal((B, n), dtype=np.float32) * np.float32(0.3)).astype(np.float32)


def _live(name, cfg, sd, B, F, seed, ids=None):
    key = (name, B, F, seed)
    if key not in _LIVE:
        mel = synthetic.synthetic_mel(B, F, cfg["n_mel_channels"], seed=seed)
        wave = _wave(B, F * cfg["hop_length"], seed)
        r64 = fr.forward(sd, cfg, mel, wave, ids, np.float64)
        r32 = fr.forward(sd, cfg, mel, wave, ids, np.float32)
        _LIVE[key] = (mel, wave, r64, wr.linf(r32["z"], r64["z"]), wr.linf(r32["log_s"], r64["log_s"]))
    return _LIVE[key]


class Entry:
    """ctts_waveglow_forward_spk_f32 itself, on workspaces the test owns."""

    def __init__(self, m):
        self.m, self.dev = m, torch.device("cuda", 0)
        self.blob, self.fwd, _ = m._ensure_forward_packed(self.dev)
        self.c, self.lib = m.c_config(), _lib.lib()
        self.S = sum(c.conv.weight.shape[0] // 2 for c in m.convinv)

    def workspace(self, B, F):
        n = _lib.nbytes(self.lib.ctts_waveglow_forward_workspace_bytes, C.byref(self.c), B, F, what="workspace query")
        return torch.zeros(n // 4, dtype=torch.float32, device=self.dev)

    def __call__(self, mel, wave, ids=None, ws=None):
        B, _, F = mel.shape
        L = self.m.steps_for(F)
        ws = self.workspace(B, F) if ws is None else ws
        z = torch.full((B, self.m.n_group, L), float("nan"), device=self.dev)
        log_s = torch.full((B, self.S, L), float("nan"), device=self.dev)
        sums = torch.full((B, self.m.n_flows + 1), float("nan"), dtype=torch.float64, device=self.dev)
        args = [_dev(mel), _dev(wave), _dev(ids)]
        _lib.check(self.lib.ctts_waveglow_forward_spk_f32(C.byref(self.c), _lib.ptr(self.blob), _lib.ptr(self.fwd), _lib.ptr(args[0]),
                                                          _lib.ptr(args[1]), _lib.ptr(args[2]), _lib.ptr(z), _lib.ptr(log_s),
                                                          _lib.ptr(sums), B, F, _lib.ptr(ws), ws.numel() * 4, _lib.stream(self.dev)),
                   "ctts_waveglow_forward_spk_f32")
        torch.cuda.synchronize()
        return z.cpu().numpy(), log_s.cpu().numpy(), sums.cpu().numpy(), ws


def _halo_is_zero(e, ws, B, F):
    """The padded [rows][ld] tensors at the head of the workspace (carve() in waveglow_api.hip: audio, then spect, speaker rows,
    h_tmp, h_all, x, act, out; every section starts on a multiple of 64 floats): nothing but zeros outside [pad, pad + L)."""
    geo = _lib.WaveGlowGeometry()
    _lib.check(e.lib.ctts_waveglow_geometry_for(C.byref(e.c), F, C.byref(geo)), "geometry")
    up = lambda n: (n + 63) // 64 * 64                                                   # noqa: E731
    m = e.m
    Cw, nf = m.WN_config["n_channels"], m.n_flows
    S = (m.WN_config["speaker_embed_dim"] + 31) // 32 * 32
    o = up(B * m.n_group * geo.steps)
    for rows in (m.n_mel_channels * m.n_group, nf * S, nf * H, nf * H, Cw, Cw, Cw):
        t = ws[o:o + B * rows * geo.ld].view(B * rows, geo.ld) if rows else None
        if t is not None and (float(t[:, :geo.pad].abs().max()) != 0.0 or float(t[:, geo.pad + geo.steps:].abs().max()) != 0.0):
            return False
        o = up(o + B * rows * geo.ld)
    return True


@pytest.mark.parametrize("B,F", [(1, 1), (3, 5), (2, 37), (1, 130)])
def test_ragged_shapes_match_float64(hip_lib_path, B, F):
    """toy_early (n_half 4 / 3 / 2): one frame; odd batch; L = 1184 (no multiple of 256: a cut tail workgroup); L = 4160 (more than
    one sum-of-squares chunk, 17 tail workgroups).  Then the same workspace again after a call at another geometry."""
    m, cfg, sd = _model("toy_early", hip_lib_path)
    mel, wave, r64, z32, ls32 = _live("toy_early", cfg, sd, B, F, 100 + F)
    e = Entry(m)
    z, log_s, sums, ws = e(mel, wave)
    _check_linf({"case": f"toy_early_b{B}_f{F}", "test": "ragged"}, z, log_s, r64["z"], r64["log_s"], z32, ls32)
    assert np.isfinite(sums).all() and _halo_is_zero(e, ws, B, F)
    e(synthetic.synthetic_mel(2, F + 2, cfg["n_mel_channels"], seed=7), _wave(2, (F + 2) * cfg["hop_length"], 7))
    z2, log_s2, sums2, _ = e(mel, wave, ws=ws)
    assert np.array_equal(z2.view(np.uint32), z.view(np.uint32)) and np.array_equal(log_s2.view(np.uint32), log_s.view(np.uint32))
    assert np.array_equal(sums2.view(np.uint64), sums.view(np.uint64))
    assert _halo_is_zero(e, ws, B, F)
    # the host class gives the entry's bits
    zc, lc, _ = _forward(m, mel, wave)
    assert np.array_equal(zc.view(np.uint32), z.view(np.uint32)) and np.array_equal(lc.view(np.uint32), log_s.view(np.uint32))


# ------------------------------------------------------------------------------- c. full_f9: every stack form ----
FORMS = {
    "default": [],                                                                        # direct in-layers at this length
    "winograd_paired": [("CTTS_F32_WINOGRAD_MIN", "0"), ("CTTS_F32_WINOGRAD_NO_FUSED", "1")],
    "winograd_fused": [("CTTS_F32_WINOGRAD_MIN", "0"), ("CTTS_F32_WINOGRAD_FUSED_MIN", "0")],
    "unfolded": [("CTTS_F32_NO_WN_FOLD", "1")],                                           # per-layer start + flow_tail forward
}


@pytest.mark.parametrize("form", list(FORMS))
def test_full_f9_matches_float64_in_every_form(hip_lib_path, tuning, form):
    m, cfg, _ = _model("full_f9", hip_lib_path)
    _, _, mel, wave, _, _ = fr.case_inputs("full_f9")
    g = fr.load_case("full_f9")
    for knob, value in FORMS[form]:
        tuning.set(knob, value)
    z, log_s, _ = _forward(m, mel, wave)
    _check_linf({"case": "full_f9", "test": "form", "form": form}, z, log_s, g["z_f64"], g["log_s_f64"], g["z_linf32"],
                g["log_s_linf32"])
    assert rms_rel_err(z, g["z_ref"]) < WAVE_TOL


# ------------------------------------------------------------------------------- d. round trip ----
@pytest.mark.parametrize("name", ["toy_early", "toy_hop512_g16", "toy_spk_rezero"])
def test_round_trip_gives_the_waveform_back(hip_lib_path, name):
    """infer_from_noise(mel, forward(mel, x)[0]) against x = 0.3 N(0,1): RMS relative < 1e-3.  Multispeaker: the same ids both
    ways; other ids on the way back (voice conversion) give a finite waveform of the same shape."""
    m, cfg, _ = _model(name, hip_lib_path)
    B, F = 2, 6
    mel = _dev(synthetic.synthetic_mel(B, F, cfg["n_mel_channels"], seed=51))
    x = _dev(_wave(B, F * cfg["hop_length"], 52))
    ids = torch.tensor([5, 400]) if m.multispeaker else None
    z = m(mel, x, speaker_id=ids)[0]
    back = m.infer_from_noise(mel, z, speaker_id=ids)
    err = rms_rel_err(back.cpu().numpy(), x.cpu().numpy())
    _log({"case": name, "test": "round_trip", "rms_rel": err})
    assert back.shape == x.shape and err < WAVE_TOL
    if m.multispeaker:
        conv = m.infer_from_noise(mel, z, speaker_id=torch.tensor([400, 5]))
        assert conv.shape == x.shape and bool(torch.isfinite(conv).all())
        assert rms_rel_err(conv.cpu().numpy(), x.cpu().numpy()) > WAVE_TOL            # another voice is another waveform


# ------------------------------------------------------------------------------- e. batch independence, sums ----
def test_an_item_does_not_depend_on_its_batch_and_two_calls_agree(hip_lib_path):
    m, cfg, sd = _model("toy_early", hip_lib_path)
    B, F = 4, 11                                                       # L = 352: two tail workgroups, the second one cut
    mel = synthetic.synthetic_mel(B, F, cfg["n_mel_channels"], seed=61)
    wave = _wave(B, F * cfg["hop_length"], 62)
    e = Entry(m)
    z, log_s, sums, ws = e(mel, wave)
    z2, log_s2, sums2, _ = e(mel, wave, ws=ws)
    for a, b in ((z, z2), (log_s, log_s2)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(sums.view(np.uint64), sums2.view(np.uint64))
    for b in range(B):
        zb, lb, sb, _ = e(mel[b:b + 1], wave[b:b + 1])
        assert np.array_equal(zb[0].view(np.uint32), z[b].view(np.uint32)), b
        assert np.array_equal(lb[0].view(np.uint32), log_s[b].view(np.uint32)), b
        assert np.array_equal(sb[0].view(np.uint64), sums[b].view(np.uint64)), b


@pytest.mark.parametrize("F", [3, 130])
def test_sums_are_the_float64_sums_of_the_returned_values(hip_lib_path, F):
    """per_item against the float64 sum of the returned fp32 z / log_s: within 1e-10 of the sum of |terms| (double accumulation of
    <= 1e6 fp32 values); loss == mean(per_item) to fp32 rounding.  On the det > 0 model, where the loss is a number."""
    m, cfg, _ = _model(fr.POSDET, hip_lib_path)
    B, sigma = 3, 0.7
    mel = _dev(synthetic.synthetic_mel(B, F, cfg["n_mel_channels"], seed=71))
    x = _dev(_wave(B, F * cfg["hop_length"], 72))
    z, log_s, ld = m(mel, x)
    out = m.nll(mel, x, sigma=sigma)
    z64 = z.double().cpu().numpy()
    ls64 = torch.cat(log_s, 1).double().cpu().numpy()
    G, L = z64.shape[1], z64.shape[2]
    logdet = float(m._fwd[2].double().sum())                            # sum_k logdet W_k: the class's own fp32 values
    assert np.allclose([float(v) for v in ld], B * L * m._fwd[2].numpy(), rtol=2 * EPS32)
    want = ((z64 ** 2).sum(axis=(1, 2)) / (2 * sigma * sigma) - ls64.sum(axis=(1, 2)) - L * logdet) / (G * L)
    scale = ((z64 ** 2).sum(axis=(1, 2)) / (2 * sigma * sigma) + np.abs(ls64).sum(axis=(1, 2)) + L * abs(logdet)) / (G * L)
    got = out["per_item"].cpu().numpy()
    assert np.all(np.abs(got - want) <= 1e-10 * scale), (got, want)
    assert abs(float(out["loss"]) - got.mean()) <= EPS32 * abs(got.mean())


# ------------------------------------------------------------------------------- f. modes, and infer undisturbed ----
def test_split_bf16_gemm_mode_recovers_the_noise(hip_lib_path):
    name = "toy"
    cfg, sd, mel, wave, _, _ = fr.case_inputs(name)
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(sd))
    m = m.cuda().eval().set_f32_gemm_mode("bf16x3")
    z, _, _ = _forward(m, mel, wave)
    err = rms_rel_err(z, np.load(os.path.join(GOLDEN, f"waveglow_{name}.npz"))["z_scaled"])
    _log({"case": name, "test": "bf16x3", "rms_rel": err})
    assert err < WAVE_TOL


def test_infer_before_and_after_a_forward_is_bit_equal(hip_lib_path):
    """A model that only infers packs nothing new; the forward blob, packed on the first forward call, disturbs nothing."""
    cfg, sd, mel, wave, _, _ = fr.case_inputs("toy_early")
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(sd))
    m = m.cuda().eval()
    g = np.load(os.path.join(GOLDEN, "waveglow_toy_early.npz"))
    before = m.infer_from_noise(_dev(mel), _dev(g["z_scaled"])).cpu().numpy()
    assert m._fwd is None
    m(_dev(mel), _dev(wave))
    assert m._fwd is not None
    after = m.infer_from_noise(_dev(mel), _dev(g["z_scaled"])).cpu().numpy()
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    m.repack()
    assert m._fwd is None


# ------------------------------------------------------------------------------- g. the one-flow stage entry ----
def test_stage_entry_runs_what_the_whole_model_entry_runs(hip_lib_path):
    """ctts_upsample_squeeze_f32 -> ctts_wn_cond_f32 -> ctts_waveglow_flow_forward_f32 flow by flow (flow 0 from the waveform) gives
    the bits of ctts_waveglow_forward_spk_f32: z, every flow's log_s and its sum per item."""
    m, cfg, _ = _model("toy_early", hip_lib_path)
    B, F = 2, 11
    mel = synthetic.synthetic_mel(B, F, cfg["n_mel_channels"], seed=81)
    wave = _wave(B, F * cfg["hop_length"], 82)
    e = Entry(m)
    z_ref, log_s_ref, sums_ref, _ = e(mel, wave)
    lib, c, dev = e.lib, e.c, e.dev
    geo = _lib.WaveGlowGeometry()
    _lib.check(lib.ctts_waveglow_geometry_for(C.byref(c), F, C.byref(geo)), "geometry")
    L, st = geo.steps, _lib.stream(dev)
    spect = torch.zeros(B, m.n_mel_channels * m.n_group, geo.ld, device=dev)
    h_tmp = torch.zeros(B, m.n_flows * H, geo.ld, device=dev)
    h_all = torch.zeros_like(h_tmp)
    mel_d, wave_d = _dev(mel), _dev(wave)
    _lib.check(lib.ctts_upsample_squeeze_f32(C.byref(c), _lib.ptr(e.blob), _lib.ptr(mel_d), _lib.ptr(spect), B, F, st), "upsample_squeeze")
    _lib.check(lib.ctts_wn_cond_f32(C.byref(c), _lib.ptr(e.blob), _lib.ptr(spect), None, _lib.ptr(h_tmp), _lib.ptr(h_all), B, F, st), "wn_cond")
    ws = e.workspace(B, F)
    z = torch.full((B, m.n_group, L), float("nan"), device=dev)
    off = 0
    for k, conv in enumerate(m.convinv):
        nh = conv.conv.weight.shape[0] // 2
        log_s = torch.full((B, nh, L), float("nan"), device=dev)
        s = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
        _lib.check(lib.ctts_waveglow_flow_forward_f32(C.byref(c), _lib.ptr(e.blob), _lib.ptr(e.fwd), k, _lib.ptr(z),
                                                      _lib.ptr(wave_d) if k == 0 else None, _lib.ptr(h_all), _lib.ptr(log_s), _lib.ptr(s),
                                                      B, F, _lib.ptr(ws), ws.numel() * 4, st), f"flow_forward({k})")
        torch.cuda.synchronize()
        assert np.array_equal(log_s.cpu().numpy().view(np.uint32), log_s_ref[:, off:off + nh].view(np.uint32)), k
        assert np.array_equal(s.cpu().numpy().view(np.uint64), sums_ref[:, k].view(np.uint64)), k
        off += nh
    assert np.array_equal(z.cpu().numpy().view(np.uint32), z_ref.view(np.uint32))
    # only flow 0 may read the waveform
    rc = lib.ctts_waveglow_flow_forward_f32(C.byref(c), _lib.ptr(e.blob), _lib.ptr(e.fwd), 1, _lib.ptr(z), _lib.ptr(wave_d), _lib.ptr(h_all),
                                            None, None, B, F, _lib.ptr(ws), ws.numel() * 4, st)
    assert rc == -1 and b"flow 0" in lib.ctts_last_error()
