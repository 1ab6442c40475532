"""The composed conditioning of the fp32 WaveGlow: h_all straight from the mel frames in one GEMM (ctts_wn_cond_composed_f32)
against a float64 restatement of the reference chain - ConvTranspose1d, trim, squeeze, cond layers 0 and 1 (glow.py:318-324,
198-199) - on the weights the packer receives.

Bound: the chain of launches (ctts_upsample_squeeze_f32 -> ctts_wn_cond_f32) runs inside the test on the same inputs; the composed
form's L-inf error against float64 must be <= 2 x the chain's.  The factor 2 covers another summation order: one sum over J n_mel
products of a matrix rounded once from double, against n_mel G + 256 products through two fp32 roundings.  Every case prints both
errors and appends them to profiles/r31_01_cond_composed_parity.jsonl.

The fallbacks run `infer` in child processes, because the library reads CTTS_F32_COND_CHAIN once: the grouped-upsampler and the
multispeaker toys must come out bit-equal with and without the knob (they never leave the chain), and `toy` under the knob must be
bit-equal to `toy` packed without the composed matrix, where the new launch cannot be reached.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import waveglow_f64_restatement as wr
from conftest import REPO
from cookietts_amd import WaveGlow, _lib, synthetic

pytestmark = pytest.mark.gpu

PARITY_LOG = os.path.join(REPO, "profiles", "r31_01_cond_composed_parity.jsonl")
H = wr.COND_HIDDEN
# frames from which `infer` takes the composed form on the toys (n_mel 80, 32 phases: waveglow_api.hip cond_composed)
F_COMPOSED = 48


def upsample_squeeze_f64(mel, w_up, b_up, hop, G):
    """glow.py:318-324 in float64: y[b, co, hop (f + j) + u] += mel[b, ci, f] w_up[ci, co, hop j + u], + bias, the first F hop samples
    kept, then spect[b, co G + s, l] = y[b, co, G l + s]."""
    mel = np.asarray(mel, np.float64)
    B, M, F = mel.shape
    w = np.asarray(w_up, np.float64)
    win = w.shape[2]
    J = win // hop
    assert J * hop == win and w.shape[:2] == (M, M)
    w = w.reshape(M, M, J, hop)
    y = np.zeros((B, M, F + J - 1, hop))
    for j in range(J):
        y[:, :, j:j + F] += np.einsum("bif,iou->bofu", mel, w[:, :, j])
    y = y[:, :, :F].reshape(B, M, F * hop) + np.asarray(b_up, np.float64)[None, :, None]
    return y.reshape(B, M, F * hop // G, G).transpose(0, 1, 3, 2).reshape(B, M * G, F * hop // G)


class Model:
    def __init__(self, name, seed=17):
        self.name, self.cfg = name, synthetic.WAVEGLOW_CONFIGS[name]
        self.sd = wr.state_dict(name, seed)
        m = WaveGlow(**self.cfg)
        m.load_state_dict(synthetic.to_torch(self.sd))
        self.m = m.cuda().eval()
        self.dev = torch.device("cuda", 0)
        self.blob, _ = self.m._ensure_packed(self.dev)
        self.c = self.m.c_config()
        self.lib = _lib.lib()
        self.n_flows, self.G, self.n_layers = self.cfg["n_flows"], self.cfg["n_group"], self.cfg["WN_config"]["n_layers"]

    def geometry(self, F):
        geo = _lib.WaveGlowGeometry()
        _lib.check(self.lib.ctts_waveglow_geometry_for(C.byref(self.c), F, C.byref(geo)), "geometry")
        return geo


_MODELS = {}


@pytest.fixture
def model(hip_lib_path):
    def get(name):
        if name not in _MODELS:
            _MODELS[name] = Model(name)
        return _MODELS[name]
    yield get


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


# toy: 3 frames < J = 4 taps (the zero halo), 9 (no multiple of 4), 131 (a second column tile of frames, its taps reach back into
# the first); toy_hop512_g16: J = 2, 16-row latent; toy_hop384_g12: J = 3, n_group 12
# no_glds: the register-staged loop of the same launch (CTTS_F32_NO_GLDS), on the two-tile case
@pytest.mark.parametrize("name,F,no_glds", [("toy", 3, False), ("toy", 9, False), ("toy", 131, False), ("toy", 131, True),
                                            ("toy_hop512_g16", 5, False), ("toy_hop384_g12", 5, False)])
def test_composed_cond_matches_float64(model, tuning, name, F, no_glds):
    st = model(name)
    if no_glds:
        tuning.set("CTTS_F32_NO_GLDS")
    lib, c, dev = st.lib, st.c, st.dev
    B = 2
    geo = st.geometry(F)
    L, stream = geo.steps, _lib.stream(dev)
    n_mel, hop = st.cfg["n_mel_channels"], st.cfg["hop_length"]
    mel = synthetic.synthetic_mel(B, F, n_mel, seed=41 + F)
    spect64 = upsample_squeeze_f64(mel, st.sd["upsample.weight"], st.sd["upsample.bias"], hop, st.G)
    assert spect64.shape == (B, n_mel * st.G, L)
    ref = [wr.cond_hidden(wr.flow_weights(st.sd, k, st.n_layers), spect64) for k in range(st.n_flows)]

    mel_d = torch.from_numpy(mel).to(dev).contiguous()
    # today's chain through its stage entries
    spect = torch.zeros(B, n_mel * st.G, geo.ld, device=dev)
    h_tmp = torch.zeros(B, st.n_flows * H, geo.ld, device=dev)
    h_chain = torch.zeros_like(h_tmp)
    _lib.check(lib.ctts_upsample_squeeze_f32(C.byref(c), _lib.ptr(st.blob), _lib.ptr(mel_d), _lib.ptr(spect), B, F, stream), "upsample_squeeze")
    _lib.check(lib.ctts_wn_cond_f32(C.byref(c), _lib.ptr(st.blob), _lib.ptr(spect), None, _lib.ptr(h_tmp), _lib.ptr(h_chain), B, F, stream),
               "wn_cond")
    # the composed form: every valid column must be written (NaN before), no halo column touched (zero before)
    nbytes = lib.ctts_wn_cond_composed_scratch_bytes(C.byref(c), B, F)
    assert nbytes > 0, lib.ctts_last_error()
    scratch = torch.full((nbytes // 4,), float("nan"), device=dev)
    h_new = torch.zeros_like(h_tmp)
    h_new[:, :, geo.pad:geo.pad + L] = float("nan")
    _lib.check(lib.ctts_wn_cond_composed_f32(C.byref(c), _lib.ptr(st.blob), _lib.ptr(mel_d), _lib.ptr(scratch), _lib.ptr(h_new), B, F, stream),
               "wn_cond_composed")
    torch.cuda.synchronize()
    assert float(h_new[:, :, :geo.pad].abs().max()) == 0.0 and float(h_new[:, :, geo.pad + L:].abs().max()) == 0.0
    got_new = h_new[:, :, geo.pad:geo.pad + L].cpu().numpy()
    got_chain = h_chain[:, :, geo.pad:geo.pad + L].cpu().numpy()
    assert np.isfinite(got_new).all() and np.isfinite(got_chain).all()
    for k in range(st.n_flows):
        e_new = wr.linf(got_new[:, k * H:(k + 1) * H], ref[k])
        e_chain = wr.linf(got_chain[:, k * H:(k + 1) * H], ref[k])
        _log({"case": f"{name}_f{F}" + ("_no_glds" if no_glds else ""), "flow": k, "batch": B, "frames": F, "steps": L, "composed_linf": e_new, "chain_linf": e_chain,
              "composed_over_chain": e_new / e_chain, "ref_abs_max": float(np.abs(ref[k]).max())})
        assert e_chain > 0.0 and e_new <= 2.0 * e_chain, (name, F, k, e_new, e_chain)


def test_no_composed_form_is_refused_by_name(model):
    """A multispeaker config holds no composed matrix: the size query answers 0 and the stage entry refuses."""
    st = model("toy_spk_rezero")
    assert st.lib.ctts_wn_cond_composed_scratch_bytes(C.byref(st.c), 2, 9) == 0
    buf = torch.zeros(16, device=st.dev)
    rc = st.lib.ctts_wn_cond_composed_f32(C.byref(st.c), _lib.ptr(st.blob), _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), 2, 9, None)
    assert rc == -1 and b"composed" in st.lib.ctts_last_error()


# ---------------------------------------------------------------------------------------- the fallbacks, through `infer` ----
_CHILD = r"""
import ctypes as C, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import waveglow_f64_restatement as wr
from cookietts_amd import WaveGlow, _lib, synthetic
out, F, B = {}, int(sys.argv[3]), 2
for name, composed in (("toy_simple", True), ("toy_spk_rezero", True), ("toy", True), ("toy", False)):
    cfg = synthetic.WAVEGLOW_CONFIGS[name]
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(wr.state_dict(name, 17)))
    m = m.cuda().eval()
    m._composed_cond = composed
    mel = torch.from_numpy(synthetic.synthetic_mel(B, F, cfg["n_mel_channels"], seed=5)).cuda()
    z = torch.from_numpy(synthetic.synthetic_noise(B, cfg["n_group"], F * cfg["hop_length"] // cfg["n_group"], seed=6) * np.float32(0.7)).cuda()
    ids = torch.tensor([3, 500]) if cfg["WN_config"]["speaker_embed_dim"] else None
    key = name + ("" if composed else "_nocc")
    out[key] = m.infer_from_noise(mel, z, speaker_id=ids).cpu().numpy()
    c = m.c_config()
    out[key + "_ws"] = np.int64(_lib.lib().ctts_waveglow_workspace_bytes_opt(C.byref(c), B, F, m._options()))
    out[key + "_opt"] = np.int64(m._options())
np.savez(sys.argv[2], **out)
"""


@pytest.fixture(scope="module")
def arms(hip_lib_path, tmp_path_factory):
    """`infer` of the four models at F_COMPOSED frames in two fresh processes: without the knob and with CTTS_F32_COND_CHAIN=1."""
    d = tmp_path_factory.mktemp("cond_arms")
    res = {}
    for arm, knob in (("default", None), ("chain", "1")):
        env = {k: v for k, v in os.environ.items() if k != "CTTS_F32_COND_CHAIN"}
        if knob:
            env["CTTS_F32_COND_CHAIN"] = knob
        path = str(d / f"{arm}.npz")
        subprocess.run([sys.executable, "-c", _CHILD, REPO, path, str(F_COMPOSED)], check=True, env=env, timeout=600)
        res[arm] = dict(np.load(path))
    return res


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_grouped_and_multispeaker_models_keep_the_chain(arms):
    for name in ("toy_simple", "toy_spk_rezero"):
        d, k = arms["default"][name], arms["chain"][name]
        assert np.isfinite(d).all() and _bits_equal(d, k), name
        assert arms["default"][name + "_ws"] == arms["chain"][name + "_ws"], name          # spect and h_tmp still reserved
        assert arms["default"][name + "_opt"] == 0, name                                    # the class never asks for it


def test_knob_arm_is_the_library_without_the_composed_form(arms):
    d, k = arms["default"], arms["chain"]
    # under the knob: the bits of a model packed without the composed matrix (no knob), whose infer cannot reach the new launch
    assert _bits_equal(k["toy"], d["toy_nocc"]) and _bits_equal(k["toy"], k["toy_nocc"])
    assert k["toy_ws"] == d["toy_nocc_ws"] and d["toy_opt"] == 1 and d["toy_nocc_opt"] == 0
    # without it the composed form ran: the workspace holds no spect / h_tmp, and the waveform moves by rounding only
    assert d["toy_ws"] < k["toy_ws"]
    assert np.isfinite(d["toy"]).all()
    rms = float(np.sqrt(np.mean((d["toy"].astype(np.float64) - k["toy"]) ** 2)) / np.sqrt(np.mean(k["toy"].astype(np.float64) ** 2)))
    _log({"case": f"toy_infer_f{F_COMPOSED}", "composed_vs_chain_rms_rel": rms})
    assert rms <= 1e-3                                    # the fp32 waveform tolerance of tests/test_waveglow_gpu.py
