"""Tacotron2Loss without a GPU: the numpy restatement (tests/taco_loss_restatement.py) against the reference's own outputs
(tests/golden/taco_loss_*.npz, make_golden_taco_loss.py), the power of those fixtures to tell a wrong implementation from a right
one, and the host-side surface of the device path (exports, workspace query, refusals).  The device side is
tests/test_taco_loss_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import taco_loss_restatement as tr

NEW_SYMBOLS = ("ctts_taco_loss_workspace_bytes", "ctts_taco_loss_f32", "ctts_taco_loss_finalize_f32",
               "ctts_alignment_metric_masked_f32")
# float64 restatement against the float64 reference: both evaluate the same formulas in IEEE double and differ by summation
# order over at most 80 * 65 * 5 = 26000 addends: 26000 * 2^-53 = 3e-12 of the sum of magnitudes; 1e-10 leaves room for the
# cancelling terms (sylps_kld, the score's punishments).  Keys the reference itself forms in float32 whatever it is handed
# (weighted_score: torch.tensor(scores); p_missing_enc; the float32 path length inside the diagonalities, and with it the
# score; the guided-attention weights of diag_att, which numpy's and torch's float32 exp round differently, and with it loss)
# get four float32 units instead.
TOL64 = 1e-10
F32_KEYS = ("weighted_score", "p_missing_enc", "diag_att", "loss", "diagonality", "att_diagonality", "att_score")


def _tol64(key, y):
    return (4 * tr.EPS32 if key in F32_KEYS else TOL64) * max(abs(y), 1.0)


def _check(what, key, got, want, tol):
    err = abs(float(got) - float(want))
    print(f"{what} {key}: {float(got):.9g} vs {float(want):.9g}, error {err:.2e}, bound {float(tol):.2e}")
    assert err <= tol or (np.isnan(got) and np.isnan(want)), (what, key, float(got), float(want), err, float(tol))


@pytest.mark.parametrize("case", tr.CASES)
def test_restatement_matches_reference_golden(case):
    """float32 against the reference's float32 run at the parity bound (two float32 evaluations of one formula, each within e32 of
    the float64 one up to summation order); float64 against its float64 run at TOL64."""
    g = tr.load_golden(case)
    for dtype, tag in ((np.float32, "32"), (np.float64, "64")):
        r = tr.taco_loss(g, dtype, g["hp"], g["loss_scalars"])
        assert (r["pred_len"] == g["pred_len"]).all()
        fl = tr.file_losses(r["per_item"], g["audiopath"])
        assert [p for p in g["audiopath"] if "att_score" in fl[p]] == g["audiopath"][-1:]          # :285
        for i, k in enumerate(tr.TERMS):
            y = g["ld" + tag][i]
            tol = tr.bound(g["ld_e32"][i], g["ld64"][i]) if tag == "32" else _tol64(k, y)
            _check(f"{case} f{tag}", k, r["loss_dict"][k], y, tol)
        for b, path in enumerate(g["audiopath"]):
            for j, k in enumerate(tr.FILE_KEYS):
                y = g["fl" + tag][b, j]
                tol = tr.bound(g["fl_e32"][b, j], g["fl64"][b, j]) if tag == "32" else _tol64(k, y)
                _check(f"{case} f{tag} item {b}", k, fl[path][k], y, tol)
        y = g["att_score" + tag]
        _check(f"{case} f{tag}", "att_score", fl[g["audiopath"][-1]]["att_score"], y,
               tr.bound(g["att_score_e32"], g["att_score64"]) if tag == "32" else _tol64("att_score", y))


def test_goldens_hold_the_promised_edges():
    g = tr.load_golden("edges")
    ml, tl, plen = g["mel_lengths"], g["text_lengths"], g["pred_len"]
    assert g["gt_mel"].shape[2] == 65 and g["alignments"].shape[2] == 65
    assert ml[1] == 1 and g["pres_prev_state"][2] == 1 and plen[3] > ml[3] and plen[0] < ml[0] and tl[4] <= 12
    r = tr.taco_loss(g, np.float64)
    assert tl[3] > 12 and ml[3] < 0.75 * ml.max() and r["metric_pred"][5][3] > 0.08
    g = tr.load_golden("weights")
    assert g["loss_scalars"] == {"spec_MSE_weight": 2.0, "gate_loss_weight": None, "diag_att_weight": 0.0}
    assert g["hp"]["gate_positive_weight"] == 4 and g["hp"]["DiagonalGuidedAttention_sigma"] == 0.4


@pytest.mark.parametrize("name", tr.PERTURBATIONS)
def test_each_perturbation_moves_a_golden_key_far_beyond_its_bound(name):
    """One mistake each, on the `edges` fixture: some key of loss_dict / file_losses leaves its bound by more than 10 x."""
    g = tr.load_golden("edges")
    r = tr.taco_loss(g, np.float64, g["hp"], g["loss_scalars"], perturb={name})
    ratios = {k: abs(float(r["loss_dict"][k]) - g["ld64"][i]) / tr.bound(g["ld_e32"][i], g["ld64"][i]) for i, k in enumerate(tr.TERMS)
              if g["ld64"][i] != 0}
    worst = max(ratios, key=ratios.get)
    print(f"{name}: {worst} moves by {ratios[worst]:.3g} bounds")
    assert ratios[worst] > 10, (name, ratios)


def test_att_score_quirk_and_nan_rule_by_hand():
    """:285 leaves att_score on the last path only; :287 replaces a NaN score by the mean of the others."""
    per_item = {k: np.arange(3, dtype=np.float64) for k in tr.FILE_KEYS + ("att_score",)}
    fl = tr.file_losses(per_item, ["a", "b", "c"])
    assert "att_score" not in fl["a"] and "att_score" not in fl["b"] and fl["c"]["att_score"] == 2.0
    inp = tr.random_inputs(1, 1, 1, 4, seed=3)                         # T = 1: predicted length 0, avg_prob = 0 * inf
    r = tr.taco_loss(inp, np.float64)
    assert r["pred_len"][0] == 0 and np.isnan(r["per_item"]["att_score"][0]) and np.isnan(r["loss_dict"]["weighted_score"])


# ---- host side of the device path -------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_typed(hip_lib_path):
    from conftest import REPO
    from cookietts_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(REPO, "include", "cookietts_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and (name + "(") in header, name
    assert lib.ctts_abi_version() == 7 and "#define CTTS_ABI_VERSION 7" in header
    from cookietts_amd import taco_loss
    assert f"#define CTTS_TACO_LOSS_COLUMNS {len(taco_loss.COLUMNS)}\n" in header
    assert f"#define CTTS_TACO_LOSS_TERMS {len(taco_loss.TERMS)}\n" in header and taco_loss.TERMS == tr.TERMS
    assert C.sizeof(_lib.TacoLossParams) == 11 * 8


def test_workspace_query_and_refusals_before_any_launch(hip_lib_path):
    from cookietts_amd import _lib
    lib = _lib.lib()
    small = lib.ctts_taco_loss_workspace_bytes(3, 80, 37, 23)
    gta = lib.ctts_taco_loss_workspace_bytes(192, 80, 800, 200)
    assert 0 < small < gta and small >= lib.ctts_alignment_workspace_bytes(3, 37, 23)
    assert lib.ctts_taco_loss_workspace_bytes(1, 1, 1, 1) > 0
    for bad in ((0, 80, 37, 23), (3, 0, 37, 23), (3, 80, 0, 23), (3, 80, 37, 0), (-1, 80, 37, 23)):
        assert lib.ctts_taco_loss_workspace_bytes(*bad) == 0 and "taco_loss" in _lib.last_error(), bad
    # made-up, aligned, never dereferenced addresses: every refusal comes before a launch
    p = _lib.TacoLossParams()
    a = [C.c_void_p(4096 * i) for i in range(1, 17)]
    assert lib.ctts_taco_loss_f32(C.byref(p), *a[:13], 3, 80, 37, 23, a[13], a[14], a[15], small - 16, None) == -3   # CTTS_E_WORKSPACE
    assert "workspace" in _lib.last_error() and str(small) in _lib.last_error()
    assert lib.ctts_taco_loss_f32(C.byref(p), *a[:13], 3, 80, 0, 23, a[13], a[14], a[15], small, None) == -1
    assert lib.ctts_taco_loss_f32(C.byref(p), None, *a[1:13], 3, 80, 37, 23, a[13], a[14], a[15], small, None) == -1
    assert "NULL" in _lib.last_error()
    assert lib.ctts_taco_loss_finalize_f32(C.byref(p), None, None, *a[:7], 3, 80, 37, 23, a[13], a[14], a[15], 16, None) == -3
    assert lib.ctts_alignment_metric_masked_f32(a[0], None, None, a[1], 3, 37, 23, 0.7, a[2], a[3], 16, None) == -3


def _host_batch(B=2, n_mel=4, T=6, enc=5):
    inp = tr.random_inputs(B, T, enc, n_mel, seed=0)
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    pred = {k: t[k] for k in ("pred_mel", "pred_mel_postnet", "pred_gate_logits", "pred_sylps_mu", "pred_sylps_logvar", "alignments")}
    pred["pred_sylps"] = t["pred_sylps"].unsqueeze(1)
    gt = {k: t[k] for k in ("gt_mel", "mel_lengths", "text_lengths", "gt_gate_logits", "gt_sylps", "pres_prev_state")}
    gt.update(audiopath=[f"{i}.wav" for i in range(B)], speaker_id_ext=list(range(B)))
    return pred, gt


def test_host_refusals_by_name_with_nothing_launched(hip_lib_path, monkeypatch):
    import cookietts_amd
    from cookietts_amd import Tacotron2Loss, _lib, synthetic
    assert "Tacotron2Loss" in cookietts_amd.__all__
    crit = Tacotron2Loss(synthetic.tacotron_hparams(diag_att_weight=0.25))
    assert crit.diag_att_weight == 0.25 and crit.pos_weight == 10.0 and crit.sigma == 0.5 and crit.sylps_kld_weight == 0.0020
    p = crit._params({"spec_MSE_weight": 3.0, "gate_loss_weight": None})
    assert list(p.weights) == [3.0, 0.0, 1.0, 1.0, 1.0, 0.0020, 0.0, 0.01, 0.25]                  # :152-161, dict order
    launched = []
    monkeypatch.setattr(_lib, "lib", lambda: launched.append(1))                                   # any library call would show
    pred, gt = _host_batch()
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        crit(pred, gt, {})
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        crit.per_item(pred, gt)
    g = dict(pred, pred_mel=pred["pred_mel"].clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="no backward pass"):
        crit.per_item(g, gt)
    with pytest.raises(NotImplementedError, match="no backward pass"):                             # the public entry, in the caller's
        crit(g, gt, {})                                                                            # grad mode
    with pytest.raises(NotImplementedError, match="no backward pass"):
        crit.forward(g, gt)
    with torch.no_grad(), pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):            # grad off: past that check
        crit(g, gt, {})
    for key, bad, owner in (("pred_mel_postnet", pred["pred_mel_postnet"][:, :, :-1], "pred"), ("alignments", pred["alignments"][:, :-1], "pred"),
                            ("pred_gate_logits", pred["pred_gate_logits"][:1], "pred"), ("gt_gate_logits", gt["gt_gate_logits"][:, 1:], "gt"),
                            ("gt_sylps", gt["gt_sylps"][:1], "gt"), ("mel_lengths", torch.tensor([6, 7]), "gt"),
                            ("text_lengths", torch.tensor([0, 5]), "gt"), ("mel_lengths", torch.tensor([6]), "gt"),
                            ("pres_prev_state", torch.zeros(3), "gt")):
        p2, g2 = dict(pred), dict(gt)
        (p2 if owner == "pred" else g2)[key] = bad
        with pytest.raises(ValueError, match=key):
            crit.per_item(p2, g2)
    with pytest.raises(ValueError, match="audiopath"):
        crit(pred, dict(gt, audiopath=["only one"]), {})
    assert not launched
