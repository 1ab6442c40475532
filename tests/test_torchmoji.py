"""torchMoji feature encoder (the T2S server's style input) on the HIP path against the reference's own outputs and a float64
restatement: ``cookietts_amd.TorchMoji`` over ``ctts_torchmoji_*``, and the operators ``ctts_lstm_biseq_hardsig_f32`` and
``ctts_attention_pool_f32`` on their own.

References: tests/golden/torchmoji_*.npz are outputs of the reference's ``TorchMoji(nb_classes=None, nb_tokens=500,
feature_output=True)`` with ``cookietts_amd.synthetic.torchmoji_state_dict`` weights (tests/golden/make_golden_torchmoji.py);
tests/torchmoji_restatement.py restates the model in numpy, generic in dtype.

Bound (the rule of tests/test_tacotron_text_side.py, FACTOR = 8, without its floor): per case, e32 = the L-inf distance of the
float32 restatement from the float64 one (the reference arithmetic's own rounding, never the code under test); the reference
golden and the HIP output must both be within ``FACTOR * e32`` of the float64 restatement.  Nothing else is fixed in advance.
Every comparison prints e32, its error and the bound.

Measured on the MI355X (profiles/r21_05_torchmoji_parity.txt; tables in the docstrings of the GPU tests): the HIP error is
0.66 ... 1.57 x e32 at model and LSTM-operator level and below e32 on the pooling operator, so FACTOR stays 8.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from cookietts_amd import synthetic
import torchmoji_restatement as tmr

FACTOR = 8                       # tests/test_tacotron_text_side.py:35
SENTINEL = -7.0                  # what out / hn hold before a call: no LSTM output (|h| < 1) can equal it
GOLDENS = ("ragged6", "ragged3", "one_token", "t130")
WANT_LENGTHS = {"ragged6": (20, 7, 1, 13, 20, 2), "ragged3": (20, 7, 1), "one_token": (1,), "t130": (130, 129)}
KEYS = {"embed.weight": (500, 256), "attention_layer.attention_vector": (2304,)}
for _l, _i in ((0, 256), (1, 1024)):
    for _s in ("", "_reverse"):
        KEYS.update({f"lstm_{_l}.weight_ih_l0{_s}": (2048, _i), f"lstm_{_l}.weight_hh_l0{_s}": (2048, 512),
                     f"lstm_{_l}.bias_ih_l0{_s}": (2048,), f"lstm_{_l}.bias_hh_l0{_s}": (2048,)})


def _err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@functools.lru_cache(maxsize=None)
def _sd(nb_tokens, seed, E=256, H=512):
    return synthetic.torchmoji_state_dict(nb_tokens, seed, embedding_dim=E, hidden_size=H)


@functools.lru_cache(maxsize=None)
def _case(name):
    """A golden case with its float64 / float32 restatements and bounds, computed once."""
    g = np.load(os.path.join(GOLDEN, f"torchmoji_{name}.npz"))
    tokens, seed, V = g["tokens"], int(g["seed"]), int(g["nb_tokens"])
    sd = _sd(V, seed)
    r64, r32 = tmr.features(sd, tokens, np.float64), tmr.features(sd, tokens, np.float32)
    assert r64["features"].dtype == np.float64 and r32["features"].dtype == np.float32
    e32, e32_att = _err(r32["features"], r64["features"]), _err(r32["attention"], r64["attention"])
    return dict(name=name, tokens=tokens, seed=seed, V=V, sd=sd, r64=r64, e32=e32, bound=FACTOR * e32, e32_att=e32_att,
                bound_att=FACTOR * e32_att, golden=g["features"], golden_att=g["attention"] if "attention" in g.files else None)


# ------------------------------------------------------------------------------------------------------------------ CPU ----
@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_matches_reference_golden(name):
    c = _case(name)
    assert tuple(c["r64"]["lengths"]) == WANT_LENGTHS[name] and c["golden"].shape == (len(WANT_LENGTHS[name]), 2304)
    err = _err(c["golden"], c["r64"]["features"])
    print(f"{name}: e32 {c['e32']:.3g} reference golden {err:.3g} bound {c['bound']:.3g} max |feature| {np.abs(c['golden']).max():.2f}")
    assert 0 < c["e32"] < 5e-6                                                  # fp32 rounding, not a tolerance
    assert err <= c["bound"], (err, c["bound"])
    assert (c["golden_att"] is not None) == (len(set(WANT_LENGTHS[name])) == len(WANT_LENGTHS[name]))
    if c["golden_att"] is not None:
        err_att = _err(c["golden_att"], c["r64"]["attention"])
        print(f"{name}: attention e32 {c['e32_att']:.3g} reference golden {err_att:.3g} bound {c['bound_att']:.3g}")
        assert err_att <= c["bound_att"], (err_att, c["bound_att"])
    if name == "ragged6":
        assert c["tokens"][3, 5] == 0 and (c["tokens"][3, :5] != 0).all() and c["tokens"][3, 12] != 0      # the interior zero


def test_deliberately_wrong_restatements_miss_the_goldens():
    """Proof that the parity tests can fail: each slip, made in the restatement, misses the reference's own output by more
    than 100 x the bound the HIP result is held to - on a case whose inputs make the slip visible."""
    for name, mutations in (("ragged6", tmr.MUTATIONS), ("ragged3", ("sigmoid", "order")), ("t130", ("sigmoid", "order"))):
        c = _case(name)
        for m in mutations:
            if m == "len_count":                                                # needs a zero inside a sentence
                assert (tmr.lengths_of(c["tokens"], mutation=m) != tmr.lengths_of(c["tokens"])).any()
            err = _err(tmr.features(c["sd"], c["tokens"], np.float64, mutation=m)["features"], c["golden"])
            print(f"{name} {m}: misses the golden by {err:.3g} = {err / c['bound']:.0f} x bound")
            assert err > 100 * c["bound"], (name, m, err, c["bound"])


@pytest.mark.parametrize("name", GOLDENS)
def test_synthetic_weights_reach_both_clamps(name):
    c = _case(name)
    pre = tmr.lstm0_preactivations(c["sd"], c["tokens"])
    lo, hi = float((pre < -2.5).mean()), float((pre > 2.5).mean())
    print(f"{name}: lstm_0 i/f/o pre-activations below -2.5: {lo:.1%}, above +2.5: {hi:.1%}")
    assert lo >= 0.01 and hi >= 0.01
    assert all(float(np.abs(c["sd"][k]).max()) > 0.5 for k in c["sd"] if "bias" in k)       # a dropped b_hh would show


def test_symbols_and_size_queries(hip_lib_path):
    from cookietts_amd import _lib
    lib = _lib.lib()
    assert lib.ctts_abi_version() == 7
    for n in ("ctts_lstm_biseq_hardsig_f32", "ctts_attention_pool_f32", "ctts_torchmoji_packed_bytes", "ctts_torchmoji_pack_f32",
              "ctts_torchmoji_workspace_bytes", "ctts_torchmoji_lengths", "ctts_torchmoji_features_f32"):
        assert n in _lib.SIGNATURES and getattr(lib, n) is not None
    for V, E, H in ((50000, 256, 512), (500, 256, 512), (50, 32, 64), (50, 16, 64)):
        cfg = _lib.TorchMojiConfig(V, E, H)
        assert lib.ctts_torchmoji_packed_bytes(C.byref(cfg)) >= 4 * (V * E + 4 * H + E)
        for B, T in ((1, 1), (4, 130), (6, 20), (33, 12), (256, 5)):
            assert lib.ctts_torchmoji_workspace_bytes(C.byref(cfg), B, T) >= 4 * B * T * (4 * H + E)
    bad = _lib.TorchMojiConfig(500, 256, 96)
    assert lib.ctts_torchmoji_packed_bytes(C.byref(bad)) == 0 and "hidden_size" in _lib.last_error()
    assert lib.ctts_torchmoji_workspace_bytes(C.byref(bad), 2, 5) == 0 and "hidden_size" in _lib.last_error()
    bad = _lib.TorchMojiConfig(500, 24, 64)
    assert lib.ctts_torchmoji_packed_bytes(C.byref(bad)) == 0 and "embedding_dim" in _lib.last_error()
    ok = _lib.TorchMojiConfig(500, 256, 512)
    for B in (0, 257):
        assert lib.ctts_torchmoji_workspace_bytes(C.byref(ok), B, 20) == 0 and "batch" in _lib.last_error()
    assert lib.ctts_torchmoji_workspace_bytes(C.byref(ok), 2, 0) == 0 and "T=" in _lib.last_error()


def test_host_class_keys_loading_and_refusals(tmp_path, monkeypatch):
    from cookietts_amd import TorchMoji, torchmoji_feature_encoding
    from cookietts_amd import torchmoji as tm_mod
    m = TorchMoji(nb_tokens=500)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == KEYS and not m.training
    assert tuple(synthetic.torchmoji_state_dict(500, 1)) == tuple(m.state_dict())            # same keys, same order
    # refused by name
    with pytest.raises(NotImplementedError):
        m.train()
    with pytest.raises(NotImplementedError):
        TorchMoji(nb_tokens=500, feature_output=False)
    with pytest.raises(NotImplementedError):
        TorchMoji(nb_tokens=500, nb_classes=64)
    assert m.eval() is m
    # host path: both errors before anything touches the library
    monkeypatch.setattr(tm_mod._lib, "lib", lambda: pytest.fail("the library was reached before the host checks"))
    tok = np.array([[3, 0, 4, 0], [0, 0, 0, 0], [1, 2, 3, 4]], np.uint16)
    with pytest.raises(ValueError, match="row 1"):
        m(tok)
    with pytest.raises(IndexError):
        m(np.array([[3, 500]], np.int32))
    with pytest.raises(IndexError):
        m(torch.tensor([[3, -1]]))
    with pytest.raises(ValueError):
        m(np.zeros((2, 3), np.float32))
    got, lens = m._host_tokens(np.array([[3, 0, 4, 0, 0], [1, 0, 0, 0, 0]], np.uint16))
    assert got.dtype == np.int64 and got.shape == (2, 3) and tuple(lens) == (3, 1)
    monkeypatch.undo()
    # torchmoji_feature_encoding: output_layer.* skipped, anything else missing or stray refused
    monkeypatch.setattr(tm_mod, "NB_TOKENS", 500)
    sd = synthetic.to_torch(synthetic.torchmoji_state_dict(500, 7))
    path = str(tmp_path / "pytorch_model.bin")
    torch.save({**sd, "output_layer.0.weight": torch.zeros(64, 2304), "output_layer.0.bias": torch.zeros(64)}, path)
    loaded = torchmoji_feature_encoding(path, return_attention=True)
    assert loaded.return_attention and not loaded.training
    assert all(torch.equal(v, sd[k]) for k, v in loaded.state_dict().items())
    torch.save({**sd, "stray.weight": torch.zeros(3)}, path)
    with pytest.raises(RuntimeError, match="stray"):
        torchmoji_feature_encoding(path)
    torch.save({k: v for k, v in sd.items() if k != "lstm_1.bias_hh_l0_reverse"}, path)
    with pytest.raises(RuntimeError, match="bias_hh_l0_reverse"):
        torchmoji_feature_encoding(path)


# ------------------------------------------------------------------------------------------------------------------ GPU ----
@functools.lru_cache(maxsize=None)
def _gpu_model(seed, return_attention=True):
    from cookietts_amd import TorchMoji
    m = TorchMoji(nb_tokens=500, return_attention=return_attention)
    m.load_state_dict(synthetic.to_torch(_sd(500, seed)))
    return m.cuda().eval()


def _check_model(what, feats, att, r64, bound, bound_att, e32):
    lens = r64["lengths"]
    err = _err(feats, r64["features"])
    err_att = _err(att[:, :r64["attention"].shape[1]], r64["attention"])
    print(f"{what}: e32 {e32:.3g}  HIP features {err:.3g} (bound {bound:.3g}, HIP / e32 = {err / e32:.2f})  "
          f"attention {err_att:.3g} (bound {bound_att:.3g})")
    assert np.isfinite(feats).all() and np.isfinite(att).all()
    assert err <= bound, (err, bound)
    assert err_att <= bound_att, (err_att, bound_att)
    for b, n in enumerate(lens):
        assert (att[b, n:] == 0).all() and abs(float(att[b].sum()) - 1.0) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDENS)
def test_hip_matches_float64_on_the_golden_cases(hip_lib_path, name):
    """Host tokens in, device features and input-order attention out, against the float64 restatement (which the reference's
    golden is pinned to on the CPU).  one_token / ragged3: the VALU step kernels; ragged6: the batched MFMA form (16 padded
    rows) and the interior zero; t130: the server's maxlen, two 128-column tiles of the input projections.

    Measured on the MI355X (factor in use 8; the largest HIP error is 1.57 x e32):
        case        e32       HIP features  bound     attention e32 x 8  HIP attention  HIP vs reference golden
        ragged6     1.03e-06  1.05e-06      8.26e-06  4.27e-06           4.75e-07       1.34e-06
        ragged3     1.74e-06  1.31e-06      1.39e-05  7.36e-06           8.86e-07       1.86e-06
        one_token   2.38e-07  3.74e-07      1.90e-06  0                  0              3.95e-07
        t130        7.85e-07  7.69e-07      6.28e-06  3.59e-06           4.17e-07       8.64e-07
    """
    c = _case(name)
    m = _gpu_model(c["seed"])
    feats, att = m(c["tokens"])
    assert feats.is_cuda and feats.dtype == torch.float32 and feats.shape == c["golden"].shape
    assert att.shape == (c["tokens"].shape[0], int(c["r64"]["lengths"].max()))
    _check_model(name, feats.cpu().numpy(), att.cpu().numpy(), c["r64"], c["bound"], c["bound_att"], c["e32"])
    print(f"{name}: HIP against the reference golden {_err(feats.cpu().numpy(), c['golden']):.3g}")


@functools.lru_cache(maxsize=None)
def _b33():
    rng = np.random.default_rng(33)
    B, T = 33, 12
    lens = np.arange(B) % 12 + 1
    tok = np.zeros((B, T), np.int64)
    for b, n in enumerate(lens):
        tok[b, :n] = rng.integers(1, 500, size=n)
    sd = _sd(500, 233)
    r64, r32 = tmr.features(sd, tok, np.float64), tmr.features(sd, tok, np.float32)
    assert tuple(r64["lengths"]) == tuple(lens)
    return tok, r64, _err(r32["features"], r64["features"]), _err(r32["attention"], r64["attention"])


@pytest.mark.gpu
def test_hip_matches_float64_at_33_rows(hip_lib_path):
    """B = 33, lengths 1 ... 12 cycling: the batched form's 64-row shape, its second and third item tiles ragged or empty.

    Measured on the MI355X: e32 1.28e-06, HIP features 1.23e-06 (bound 1.02e-05), attention 6.09e-07 (bound 4.65e-06)."""
    tok, r64, e32, e32_att = _b33()
    feats, att = _gpu_model(233)(tok)
    _check_model("B33", feats.cpu().numpy(), att.cpu().numpy(), r64, FACTOR * e32, FACTOR * e32_att, e32)


# (I, H, B, T): the widths of the existing sweep; VALU form (3, 2 rows; 130 steps), batched form 16-row and 64-row shapes
HS_CASES = [(32, 64, 3, 5), (32, 64, 5, 12), (32, 64, 33, 12), (16, 64, 2, 130)]


@functools.lru_cache(maxsize=None)
def _hs_case(case):
    I, H, B, T = case
    rng = np.random.default_rng(7000 + 100 * B + T)
    x = rng.standard_normal((B, T, I)).astype(np.float32)
    # pre-activations wide enough to sit on both clamps of the hard sigmoid (|0.2 v| > 0.5) at several per cent of the gates
    dirs = [tuple((np.float32(s) * rng.standard_normal(shape)).astype(np.float32)
                  for s, shape in ((2.5 / np.sqrt(I), (4 * H, I)), (2.5 / np.sqrt(H), (4 * H, H)), (0.3, (4 * H,)), (0.3, (4 * H,))))
            for _ in range(2)]
    lens = np.array([130, 129] if T == 130 else [T, 1] + [(3 * b) % T + 1 for b in range(2, B)], np.int64)
    assert lens.shape == (B,) and lens.max() == T and (T == 130 or lens.min() == 1)
    o64, h64 = tmr.bilstm(x, lens, dirs[0], dirs[1], np.float64)
    o32, h32 = tmr.bilstm(x, lens, dirs[0], dirs[1], np.float32)
    e32 = max(_err(o32, o64), _err(h32, h64))
    # the case tells the two gates apart by far more than the bound
    from lstm_seq_restatement import bilstm as logistic_bilstm
    assert _err(logistic_bilstm(x, lens, dirs[0], dirs[1], np.float64)[0], o64) > 1000 * FACTOR * e32
    return dict(x=x, dirs=dirs, lens=lens, o64=o64, h64=h64, e32=e32, bound=FACTOR * e32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", HS_CASES, ids=[f"I{c[0]}-H{c[1]}-B{c[2]}-T{c[3]}" for c in HS_CASES])
def test_hardsig_bilstm_operator_matches_float64(hip_lib_path, case):
    """``ctts_lstm_biseq_hardsig_f32`` alone against ``packed_lstm`` with the hard gate; out / hn pre-filled with a sentinel
    (nothing written beyond a length or in the extra columns), NaN-filled workspaces.

    Measured on the MI355X (factor in use 8):
        (I, H, B, T)        e32       HIP out   HIP hn    bound
        (32, 64, 3, 5)      2.53e-07  2.53e-07  2.53e-07  2.02e-06
        (32, 64, 5, 12)     4.80e-07  3.77e-07  3.13e-07  3.84e-06
        (32, 64, 33, 12)    1.16e-06  7.65e-07  7.65e-07  9.30e-06
        (16, 64, 2, 130)    5.17e-07  5.25e-07  2.60e-07  4.14e-06
    """
    from cookietts_amd import _lib
    from cookietts_amd.tacotron2 import PAD, _ld_for
    I, H, B, T = case
    r = _hs_case(case)
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    ld = _ld_for(T)
    with torch.cuda.device(dev):
        st = _lib.stream(dev)
        packs = []
        for d in r["dirs"]:
            ts = [torch.from_numpy(a).to(dev).contiguous() for a in d]
            w = _lib.LstmWeights(*[t.data_ptr() for t in ts])
            blob = torch.zeros(_lib.nbytes(lib.ctts_lstm_seq_packed_bytes, I, H, what="pack size") // 4, dtype=torch.float32, device=dev)
            _lib.check(lib.ctts_lstm_seq_pack_f32(C.byref(w), I, H, _lib.ptr(blob), st), "ctts_lstm_seq_pack_f32")
            torch.cuda.current_stream(dev).synchronize()
            packs.append(blob)
        x = torch.zeros(B, I, ld, dtype=torch.float32, device=dev)
        x[:, :, PAD:PAD + T] = torch.from_numpy(np.ascontiguousarray(r["x"].transpose(0, 2, 1))).to(dev)
        lens = torch.from_numpy(r["lens"].astype(np.int32)).to(dev)
        row = 2 * H + 5
        nbytes = _lib.nbytes(lib.ctts_lstm_seq_workspace_bytes, H, B, ld, what="workspace size")
        out = torch.full((B, T, row), SENTINEL, dtype=torch.float32, device=dev)
        hn = torch.full((B, 2 * H), SENTINEL, dtype=torch.float32, device=dev)
        ws = torch.full((2, nbytes // 4), float("nan"), dtype=torch.float32, device=dev)
        _lib.check(lib.ctts_lstm_biseq_hardsig_f32(_lib.ptr(packs[0]), _lib.ptr(packs[1]), _lib.ptr(x), _lib.ptr(lens), _lib.ptr(out),
                                                   T * row, row, 0, H, _lib.ptr(hn), 2 * H, 0, H, B, T, I, H, ld, PAD,
                                                   _lib.ptr(ws[0]), _lib.ptr(ws[1]), nbytes, st), "ctts_lstm_biseq_hardsig_f32")
        torch.cuda.synchronize()
    out, hn = out.cpu().numpy(), hn.cpu().numpy()
    mask = np.arange(T)[None, :] < r["lens"][:, None]
    assert (out[:, :, 2 * H:] == SENTINEL).all() and (out[:, :, :2 * H][~mask] == SENTINEL).all()
    err_out = float(np.abs(np.where(mask[:, :, None], out[:, :, :2 * H] - r["o64"], 0.0)).max())
    err_hn = _err(hn, r["h64"])
    print(f"{case}: e32 {r['e32']:.3g}  HIP out {err_out:.3g} hn {err_hn:.3g}  bound {r['bound']:.3g} "
          f"(HIP / e32 = {max(err_out, err_hn) / r['e32']:.2f})")
    assert np.isfinite(out).all() and np.isfinite(hn).all()
    assert err_out <= r["bound"] and err_hn <= r["bound"], (err_out, err_hn, r["bound"])


@pytest.mark.gpu
@pytest.mark.parametrize("D", (2304, 48))
@pytest.mark.parametrize("T", (1, 7, 130))
def test_attention_pool_operator(hip_lib_path, D, T):
    """``ctts_attention_pool_f32`` alone, B = 3: row 0 has one logit of +80 (exp(80) overflows fp32 unless a maximum is
    subtracted), row 1 has length 0 (zeros, no 0 / 0), row 2 is ordinary and shorter than T where T allows.  The float64
    reference subtracts the batch maximum as the reference does; the device subtracts each row's own.

    Measured on the MI355X (out: e32, HIP, bound; T = 1 is exact in both): D=2304 T=7 2.91e-06, 6.09e-07, 2.33e-05; D=48 T=7
    2.67e-06, 2.68e-07, 2.14e-05; D=2304 T=130 2.28e-06, 4.60e-07, 1.82e-05; D=48 T=130 2.19e-06, 9.38e-07, 1.75e-05; attention
    errors 2.4e-08 ... 8.1e-08 against bounds of 2.5e-06 ... 4.2e-06 (profiles/r21_05_torchmoji_parity.txt)."""
    from cookietts_amd import _lib
    rng = np.random.default_rng(100 * D + T)
    B = 3
    vec = (rng.standard_normal(D) / np.sqrt(D)).astype(np.float32)
    feat = rng.uniform(-1, 1, (B, T, D)).astype(np.float32) * np.float32(3.0)                # ordinary logits ~ N(0, 3)
    lens = np.array([T, 0, max(1, T - 2)], np.int64)
    t80 = T // 2
    feat[0, t80] = (80.0 * vec.astype(np.float64) / float(vec.astype(np.float64) @ vec.astype(np.float64))).astype(np.float32)
    assert abs(float(feat[0, t80].astype(np.float64) @ vec.astype(np.float64)) - 80.0) < 1e-3
    rows = lens > 0
    o64, a64 = tmr.attention_pool(feat[rows], vec, lens[rows], np.float64)
    o32, a32 = tmr.attention_pool(feat[rows], vec, lens[rows], np.float32)
    e32, e32_att = _err(o32, o64), _err(a32, a64)
    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev):
        out = torch.full((B, D), SENTINEL, dtype=torch.float32, device=dev)
        att = torch.full((B, T), SENTINEL, dtype=torch.float32, device=dev)
        args = [torch.from_numpy(a).to(dev) for a in (feat, vec, lens.astype(np.int32))]
        _lib.check(_lib.lib().ctts_attention_pool_f32(*[_lib.ptr(a) for a in args], _lib.ptr(out), _lib.ptr(att), B, T, D,
                                                      _lib.stream(dev)), "ctts_attention_pool_f32")
        out2 = torch.full((B, D), SENTINEL, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().ctts_attention_pool_f32(*[_lib.ptr(a) for a in args], _lib.ptr(out2), None, B, T, D,
                                                      _lib.stream(dev)), "ctts_attention_pool_f32")
        torch.cuda.synchronize()
    out, att = out.cpu().numpy(), att.cpu().numpy()
    err, err_att = _err(out[rows], o64), _err(att[rows], a64)
    print(f"D={D} T={T}: e32 {e32:.3g} HIP out {err:.3g} bound {FACTOR * e32:.3g}; attention e32 {e32_att:.3g} HIP {err_att:.3g} "
          f"bound {FACTOR * e32_att:.3g}")
    assert np.isfinite(out).all() and np.isfinite(att).all()
    assert (out[1] == 0).all() and (att[1] == 0).all()
    assert (att[2, lens[2]:] == 0).all()
    assert np.array_equal(out2.cpu().numpy(), out)
    assert err <= FACTOR * e32 and err_att <= FACTOR * e32_att, (err, FACTOR * e32, err_att, FACTOR * e32_att)


@pytest.mark.gpu
def test_token_forms_batches_and_repeats_give_identical_bits(hip_lib_path):
    """The ragged6 tokens as a zero-padded [6, 130] host array, as a [6, 20] host array and as a [6, 130] device tensor: the
    same bits (trimming on the host and idling on the device are the same arithmetic).  A row's features are the same in a
    B = 6 and a B = 9 call (both on the 16-row batched shape); a second call repeats the first; the workspace of another
    shape in between changes nothing.  An all-zero row of a device tensor gives a zero feature row."""
    c = _case("ragged6")
    m = _gpu_model(c["seed"])
    tok20 = c["tokens"]
    tok130 = np.zeros((6, 130), np.uint16)
    tok130[:, :20] = tok20
    f20, a20 = m(tok20)
    f20 = f20.clone()
    f130, a130 = m(tok130)
    assert a130.shape == (6, 20) and torch.equal(f130, f20) and torch.equal(a130, a20)
    fdev, adev = m(torch.from_numpy(tok130.astype(np.int64)).cuda())
    assert adev.shape == (6, 130) and torch.equal(fdev, f20) and torch.equal(adev[:, :20], a20) and (adev[:, 20:] == 0).all()
    rng = np.random.default_rng(9)
    tok9 = np.concatenate([tok20, rng.integers(1, 500, size=(3, 20)).astype(np.uint16)])
    tok9[7, 11:] = 0
    f9, _ = m(tok9)
    assert torch.equal(f9[:6], f20)
    f20b, a20b = m(tok20)                                                       # after other shapes used the workspace
    assert torch.equal(f20b, f20) and torch.equal(a20b, a20)
    fnp, anp = m(tok20, return_numpy=True)
    assert isinstance(fnp, np.ndarray) and np.array_equal(fnp, f20.cpu().numpy()) and np.array_equal(anp, a20.cpu().numpy())
    hole = tok130.astype(np.int64)
    hole[2] = 0
    fz, az = m(torch.from_numpy(hole).cuda())
    assert (fz[2] == 0).all() and (az[2] == 0).all() and torch.equal(fz[[0, 1, 3, 4, 5]], f20[[0, 1, 3, 4, 5]])


@pytest.mark.gpu
def test_tacotron_takes_the_device_features_as_they_are(hip_lib_path):
    """``Tacotron2.inference(..., torchmoji_hdn=TorchMoji(...)(tokens))`` on the tacotron_small config: the device tensor goes
    in unchanged; outputs equal those from the same vector passed as a host-made tensor."""
    from cookietts_amd.tacotron2 import Tacotron2
    hp = synthetic.tacotron_hparams(**synthetic.TACOTRON_SMALL_OVERRIDES)
    shapes = json.load(open(os.path.join(GOLDEN, "tacotron_small_state_shapes.json")))
    taco = Tacotron2(hp)
    taco.load_state_dict(synthetic.to_torch(synthetic.tacotron_state_dict(hp, seed=5, shapes=shapes)))
    taco = taco.cuda().eval()
    c = _case("ragged3")
    style = _gpu_model(c["seed"], False)(c["tokens"])
    assert style.is_cuda and style.shape == (3, hp.torchMoji_attDim)
    rng = np.random.default_rng(0)
    B, T = 3, 14
    text = torch.from_numpy(rng.integers(1, hp.n_symbols, size=(B, T))).cuda()
    lens = torch.tensor([14, 9, 11]).cuda()
    spk = torch.tensor([0, 1, 2]).cuda()
    masks = synthetic.prenet_dropout_masks(8, B, hp.prenet_dim)
    a = taco.inference(text, lens, spk, style, keep_masks=masks, fixed_steps=8)
    b = taco.inference(text, lens, spk, torch.from_numpy(style.cpu().numpy().copy()), keep_masks=masks, fixed_steps=8)
    for k in ("pred_mel_postnet", "pred_gate", "alignments"):
        assert torch.isfinite(a[k]).all() and torch.equal(a[k], b[k]), k
