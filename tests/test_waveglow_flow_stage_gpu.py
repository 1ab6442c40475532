"""ONE flow of the fp32 WaveGlow path, exactly as the whole-infer entry runs it, against a float64 restatement of that flow.

ctts_waveglow_flow_f32 shares its body with the loop of ctts_waveglow_infer_spk_f32, so every form the knobs select - start / end
folds, deferred skip sum, Winograd F(2,3) in-layers, the per-layer stack plus flow tail - is compared element by element (L-inf)
with tests/waveglow_f64_restatement.py at the project's real channel counts and at the lengths where the pair mapping has its
edges.  Errors do not compound over flows, so the bound sits close to fp32 rounding, and a failure names a column.

Bound: FACTOR x ref_fp32_vs_fp64, the L-inf distance of the restatement's own fp32 numpy run from its float64 run on the same
inputs (stored in the fixtures of tests/golden/make_golden_wn_flow.py; computed live for the toy sizes).  FACTOR and how it was set:
waveglow_f64_restatement.FACTOR.  Every case prints its ratio (HIP L-inf / reference L-inf) and appends it to
profiles/r13_01_wn_flow_stage_parity.jsonl.

The reference rows are rebuilt from the fixture's float64 (b, log_s) with the very fp32 W_inverse the Python class handed the packer
(cast to float64): how the inverse was computed does not enter the comparison.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import waveglow_f64_restatement as wr
from conftest import REPO
from cookietts_amd import WaveGlow, _lib, synthetic
from oracle import waveglow_oracle as wo

pytestmark = pytest.mark.gpu

FACTOR = wr.FACTOR
assert FACTOR <= 100.0                       # test_hifigan.py's LINF_FACTOR: a case that needs more is a finding, not a bound to raise
PARITY_LOG = os.path.join(REPO, "profiles", "r13_01_wn_flow_stage_parity.jsonl")
H = wr.COND_HIDDEN

# the forms of one flow (knob, value); the in-layer form is pinned in each so that the length alone never picks it
FORMS = {
    "winograd": [("CTTS_F32_WINOGRAD_MIN", "0")],                                       # the server's form for long utterances
    "direct": [("CTTS_F32_NO_WINOGRAD", "1")],                                          # folds + deferred skip, 3-tap in-layers
    "unfolded_winograd": [("CTTS_F32_NO_WN_FOLD", "1"), ("CTTS_F32_WINOGRAD_MIN", "0")],  # layer 0 reads x at d = 1: the
                                                                                        # transform kernel's non-vector path
    "per_layer": [("CTTS_F32_NO_DEFER_SKIP", "1")],                                     # res/skip per layer + flow tail
    # the Winograd form on the register-staged conv-GEMM: transform, T2, T3, even, odd as launches of their own, even where the
    # one-launch layer is asked for
    "winograd_no_glds": [("CTTS_F32_NO_GLDS", "1"), ("CTTS_F32_WINOGRAD_MIN", "0"), ("CTTS_F32_WINOGRAD_FUSED_MIN", "0")],
}


class Stage:
    """A packed model and the C calls of its stage entry points."""

    def __init__(self, name, seed):
        self.name, self.cfg = name, synthetic.WAVEGLOW_CONFIGS[name]
        self.sd = wr.state_dict(name, seed)
        m = WaveGlow(**self.cfg)
        m.load_state_dict(synthetic.to_torch(self.sd))
        self.m = m.cuda().eval()
        self.dev = torch.device("cuda", 0)
        self.blob, _ = self.m._ensure_packed(self.dev)
        self.c = self.m.c_config()
        self.lib = _lib.lib()
        wn = self.cfg["WN_config"]
        self.C, self.n_layers, self.G, self.n_flows = wn["n_channels"], wn["n_layers"], self.cfg["n_group"], self.cfg["n_flows"]

    def w_inv(self, k):
        return self.m.convinv[k].W_inverse[..., 0].cpu().numpy()

    def geometry(self, F):
        geo = _lib.WaveGlowGeometry()
        _lib.check(self.lib.ctts_waveglow_geometry_for(C.byref(self.c), F, C.byref(geo)), "geometry")
        return geo

    def workspace(self, B, F):
        n = _lib.nbytes(self.lib.ctts_waveglow_workspace_bytes, C.byref(self.c), B, F, what="workspace query")
        return torch.zeros(n // 4, dtype=torch.float32, device=self.dev)

    def padded(self, rows, geo, at=0, total=None):
        """numpy [B][R][L] -> device [B][total][ld] in the padded layout, rows at row offset `at`, zeros elsewhere."""
        B, R, L = rows.shape
        t = torch.zeros(B, total or R, geo.ld, device=self.dev)
        t[:, at:at + R, geo.pad:geo.pad + L] = torch.from_numpy(np.ascontiguousarray(rows)).to(self.dev)
        return t

    def flow(self, k, audio, h, F, ws=None, wave=False):
        """ctts_waveglow_flow_f32 on copies of the inputs -> (audio after the call, wave or None, the workspace)."""
        B = audio.shape[0]
        geo = self.geometry(F)
        assert geo.steps == audio.shape[2] == h.shape[2]
        ws = self.workspace(B, F) if ws is None else ws
        a = torch.from_numpy(audio).to(self.dev).contiguous()
        h_all = self.padded(h, geo, at=k * H, total=self.n_flows * H)
        w = torch.zeros(B, geo.steps * self.G, device=self.dev) if wave else None
        _lib.check(self.lib.ctts_waveglow_flow_f32(C.byref(self.c), _lib.ptr(self.blob), k, _lib.ptr(a), _lib.ptr(h_all), _lib.ptr(w),
                                                   B, F, _lib.ptr(ws), ws.numel() * 4, _lib.stream(self.dev)), "ctts_waveglow_flow_f32")
        torch.cuda.synchronize()
        return a.cpu().numpy(), None if w is None else w.cpu().numpy(), ws


@pytest.fixture(scope="module")
def full(hip_lib_path):
    return Stage("full", 9)


_TOYS = {}


@pytest.fixture
def toy(hip_lib_path):
    def get(name):
        if name not in _TOYS:
            _TOYS[name] = Stage(name, 17)
        return _TOYS[name]
    yield get


@pytest.fixture(scope="module", autouse=True)
def _drop_toys():
    yield
    _TOYS.clear()


def _set_form(tuning, form, no_small=False):
    for knob, value in FORMS[form]:
        tuning.set(knob, value)
    if no_small:
        tuning.set("CTTS_F32_NO_SMALL")


def _worst(got, ref, n_layers):
    """Where the largest deviation sits: (item, row, column), the column's distance to each end, column mod 2d for each d."""
    err = np.abs(got.astype(np.float64) - ref)
    b, r, c = np.unravel_index(int(np.argmax(err)), err.shape)
    L = err.shape[2]
    mods = ", ".join(f"d={1 << i}: {c % (2 << i)}" for i in range(n_layers))
    return (f"worst |err| {err[b, r, c]:.3e} at (item {b}, row {r}, column {c}); {c} from the start, {L - 1 - c} from the end; "
            f"column mod 2d: {mods}")


def _log(rec):
    print(json.dumps(rec))
    try:
        with open(PARITY_LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def _check_flow(st, k, audio, h, F, ref_rows, ref_linf, rec):
    """The assertions every flow case shares; ref_rows float64 [B][n_rem][L], ref_linf the fp32 restatement's distance from it."""
    n_rem, _, ch_off = wr.flow_dims(st.cfg, k)
    got, _, ws = st.flow(k, audio, h, F)
    rows = got[:, ch_off:ch_off + n_rem]
    err = wr.linf(rows, ref_rows)
    rec = dict(rec, config=st.name, flow=k, batch=int(audio.shape[0]), frames=F, steps=int(audio.shape[2]), linf=err,
               ref_fp32_vs_fp64_linf=float(ref_linf), linf_over_ref=err / float(ref_linf), bound_linf=FACTOR * float(ref_linf))
    _log(rec)
    assert np.isfinite(got).all()
    assert err < FACTOR * ref_linf, (rec, _worst(rows, ref_rows, st.n_layers))
    other = np.ones(st.G, bool)
    other[ch_off:ch_off + n_rem] = False
    assert np.array_equal(got[:, other].view(np.uint32), audio[:, other].view(np.uint32))      # rows of other flows: untouched
    # the same workspace again, after a call at another length (on a workspace of its own: one geometry per workspace)
    F2 = F + 2
    a2, h2 = wr.case_inputs(st.cfg, audio.shape[0], F2, 5, 1.0)
    st.flow(k, a2, h2, F2)
    again, _, _ = st.flow(k, audio, h, F, ws=ws)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))
    if k == 0:                                                  # the last flow of infer: the mixed rows go out un-squeezed
        assert n_rem == st.G
        _, wave, _ = st.flow(k, audio, h, F, wave=True)
        assert np.array_equal(wave.view(np.uint32), wr.unsqueeze(got).view(np.uint32))
    return err / float(ref_linf)


# ---------------------------------------------------------------------------- a. the main matrix: "full", fixtures ----
@pytest.mark.parametrize("no_small", [False, True], ids=["shape_auto", "no_small"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", list(wr.FLOW_CASES))
def test_full_flow_matches_float64(full, tuning, case, form, no_small):
    key, wseed, k, B, F, seed = wr.FLOW_CASES[case]
    z = np.load(wr.flow_case_path(case))
    assert (str(z["config"]), int(z["weight_seed"]), int(z["flow"]), int(z["batch"]), int(z["frames"]), int(z["seed"])) == \
        (key, wseed, k, B, F, seed)
    n_rem, _, ch_off = wr.flow_dims(full.cfg, k)
    audio, h = wr.case_inputs(full.cfg, B, F, seed, float(z["h_scale"]))
    rows_in = audio[:, ch_off:ch_off + n_rem].astype(np.float64)
    ref_rows = wr.mix(full.w_inv(k).astype(np.float64), wr.couple(rows_in, z["e"]))
    assert wr.linf(ref_rows, z["rows"]) < 1e-4                 # (the fixture's own rows: the generator's host inverse)
    _set_form(tuning, form, no_small)
    _check_flow(full, k, audio, h, F, ref_rows, z["ref_fp32_vs_fp64"][1], {"case": case, "form": form, "no_small": no_small})


# ---------------------------------------------------------------------------- b. toy configs, references live ---------
_LIVE = {}


def _live_reference(st, k, B, F, seed):
    key = (st.name, k, B, F, seed)
    if key not in _LIVE:
        _LIVE[key] = wr.reference_case(st.cfg, st.sd, k, B, F, seed, w_inv=st.w_inv(k))
    return _LIVE[key]


@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("form", ["default", "winograd", "per_layer", "winograd_no_glds"])
@pytest.mark.parametrize("name", ["toy_spk_rezero", "toy_hop512_g16", "toy_hop384_g12"])
def test_toy_flows_match_float64(toy, tuning, name, form, F):
    """toy_spk_rezero: ReZero's alpha in the res/skip rows; toy_hop512_g16: n_half up to 8 against FOLD_ROWS; toy_hop384_g12: the
    third n_group.  Every flow of the model; "default" = no knob (short utterances keep the direct in-layers)."""
    st = toy(name)
    B, seed = 2, 23
    if form != "default":
        _set_form(tuning, form)
    for k in range(st.n_flows):
        ref = _live_reference(st, k, B, F, seed)
        audio, h = wr.case_inputs(st.cfg, B, F, seed, ref["h_scale"])
        _check_flow(st, k, audio, h, F, ref["rows"], ref["ref_fp32_vs_fp64"][1], {"case": f"{name}_k{k}_f{F}", "form": form,
                                                                                 "no_small": False})


# ---------------------------------------------------------------------------- d. the three older stage entries --------
def _halo_is_zero(t, geo):
    return float(t[:, :, :geo.pad].abs().max()) == 0.0 and float(t[:, :, geo.pad + geo.steps:].abs().max()) == 0.0


@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("name", ["toy", "toy_spk_rezero"])
def test_stage_entries_match_float64(toy, name, F):
    """ctts_wn_cond_f32, ctts_wn_stack_f32 (the per-layer form, direct in-layers) and ctts_flow_tail_f32, each from the inputs the
    stage before it left on the device, each against float64 of that stage alone."""
    st = toy(name)
    lib, c, dev = st.lib, st.c, st.dev
    B, seed = 2, 31
    geo = st.geometry(F)
    L, Cw, nl = geo.steps, st.C, st.n_layers
    sdim = st.cfg["WN_config"]["speaker_embed_dim"]
    ids = np.array([3, 500]) if sdim else None
    mel = synthetic.synthetic_mel(B, F, st.cfg["n_mel_channels"], seed=seed)
    spect = wo.upsample_squeeze(mel, st.sd["upsample.weight"], st.sd["upsample.bias"], st.cfg["hop_length"], st.G)
    w64 = [wr.flow_weights(st.sd, k, nl) for k in range(st.n_flows)]
    w32 = [wr.flow_weights(st.sd, k, nl, np.float32) for k in range(st.n_flows)]

    # cond layers 0 and 1 of every flow in one call
    spect_d = st.padded(spect, geo)
    spk_d = None
    if sdim:
        S = (sdim + 31) // 32 * 32
        spk_d = torch.zeros(B, st.n_flows * S, geo.ld, device=dev)
        for k in range(st.n_flows):
            spk_d[:, k * S:k * S + sdim, geo.pad:geo.pad + L] = torch.from_numpy(wr.speaker_rows(w32[k], ids, L)).to(dev)
    h_tmp = torch.zeros(B, st.n_flows * H, geo.ld, device=dev)
    h_all = torch.zeros_like(h_tmp)
    _lib.check(lib.ctts_wn_cond_f32(C.byref(c), _lib.ptr(st.blob), _lib.ptr(spect_d), _lib.ptr(spk_d), _lib.ptr(h_tmp), _lib.ptr(h_all),
                                    B, F, _lib.stream(dev)), "ctts_wn_cond_f32")
    torch.cuda.synchronize()
    assert _halo_is_zero(h_all, geo)
    h_gpu = h_all[:, :, geo.pad:geo.pad + L].cpu().numpy()
    for k in range(st.n_flows):
        ref = wr.cond_hidden(w64[k], spect, ids)
        ref_linf = wr.linf(wr.cond_hidden(w32[k], spect, ids), ref)
        got = h_gpu[:, k * H:(k + 1) * H]
        err = wr.linf(got, ref)
        _log({"case": f"{name}_k{k}_f{F}", "stage": "wn_cond", "linf": err, "ref_fp32_vs_fp64_linf": ref_linf, "linf_over_ref": err / ref_linf})
        assert np.isfinite(got).all() and err < FACTOR * ref_linf, (k, _worst(got, ref, nl))

    audio = (synthetic.synthetic_noise(B, st.G, L, seed=seed) * np.float32(0.7)).astype(np.float32)
    for k in range(st.n_flows):
        n_rem, n_half, ch_off = wr.flow_dims(st.cfg, k)
        hk = h_gpu[:, k * H:(k + 1) * H]
        a0 = audio[:, ch_off:ch_off + n_half]
        # the WN stack up to (not including) `end`: the skip sum
        a_d = torch.from_numpy(audio).to(dev)
        x, act, out = (torch.zeros(B, Cw, geo.ld, device=dev) for _ in range(3))
        _lib.check(lib.ctts_wn_stack_f32(C.byref(c), _lib.ptr(st.blob), k, _lib.ptr(a_d), _lib.ptr(h_all), _lib.ptr(x), _lib.ptr(act),
                                         _lib.ptr(out), B, F, _lib.stream(dev)), "ctts_wn_stack_f32")
        torch.cuda.synchronize()
        assert _halo_is_zero(out, geo) and _halo_is_zero(x, geo) and _halo_is_zero(act, geo)
        out_gpu = out[:, :, geo.pad:geo.pad + L].cpu().numpy()

        def skip_sum(w):
            dt = w["start_w"].dtype
            return wr.wn_stack(w, a0.astype(dt), lambda i: wr.cond_rows(w, hk.astype(dt), i, Cw), Cw, nl)["out"]
        ref = skip_sum(w64[k])
        ref_linf = wr.linf(skip_sum(w32[k]), ref)
        err = wr.linf(out_gpu, ref)
        _log({"case": f"{name}_k{k}_f{F}", "stage": "wn_stack", "linf": err, "ref_fp32_vs_fp64_linf": ref_linf, "linf_over_ref": err / ref_linf})
        assert np.isfinite(out_gpu).all() and err < FACTOR * ref_linf, (k, _worst(out_gpu, ref, nl))

        # end + coupling + inverse 1x1 on THAT skip sum
        _lib.check(lib.ctts_flow_tail_f32(C.byref(c), _lib.ptr(st.blob), k, _lib.ptr(out), _lib.ptr(a_d), None, B, F, _lib.stream(dev)),
                   "ctts_flow_tail_f32")
        torch.cuda.synchronize()
        got = a_d.cpu().numpy()
        w_inv = st.w_inv(k)

        def tail(w):
            dt = w["start_w"].dtype
            e = np.matmul(w["end_w"], out_gpu.astype(dt)) + w["end_b"][None, :, None]
            return wr.mix(w_inv, wr.couple(audio[:, ch_off:ch_off + n_rem].astype(dt), e))
        ref = tail(w64[k])
        ref_linf = wr.linf(tail(w32[k]), ref)
        rows = got[:, ch_off:ch_off + n_rem]
        err = wr.linf(rows, ref)
        _log({"case": f"{name}_k{k}_f{F}", "stage": "flow_tail", "linf": err, "ref_fp32_vs_fp64_linf": ref_linf, "linf_over_ref": err / ref_linf})
        assert np.isfinite(got).all() and err < FACTOR * ref_linf, (k, _worst(rows, ref, nl))
        other = np.ones(st.G, bool)
        other[ch_off:ch_off + n_rem] = False
        assert np.array_equal(got[:, other].view(np.uint32), audio[:, other].view(np.uint32))
