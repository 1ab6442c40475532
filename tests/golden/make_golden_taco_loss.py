#!/usr/bin/env python3
"""Goldens of Tacotron2Loss: the reference's own ``Tacotron2Loss.forward`` (_2_ttm/tacotron2_tm/loss_function.py:167-290) on
the CPU on seeded inputs, once in float32 and once on ``.double()`` copies of the same inputs.

Run in the build container only (it imports the reference):

    python tests/golden/make_golden_taco_loss.py

Data only: per case ``taco_loss_<case>.npz`` holds the inputs, the attributes and ``loss_scalars`` the loss was built and called
with, the float32 outputs (``ld32`` [13] in the order of the reference's dict, ``fl32`` [B, 7] the numeric fields of
``file_losses`` per item, ``att_score32`` the one the reference leaves on the last path, ``pred_len``), the float64 outputs
(``ld64``, ``fl64``, ``att_score64``) and ``e32 = |fp32 - fp64|`` per value.  The reference writes to its inputs
(``pred_mel_postnet``, ``alignments``): every run gets fresh copies.

The script ASSERTS that the fixtures stay away from the discontinuities of the loss: no second entry of an alignment row within
1e-4 of the row maximum, no encoder total (of either metric call) within 1e-3 of ``enc_min_thresh`` = 0.7, no gate sigmoid
within 1e-3 of 0.7 from frame 5 on; and that the ``edges`` case holds the items its name promises.
"""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402,F401  (puts the repository and the reference on sys.path)
import taco_loss_restatement as tr  # noqa: E402

NON_DEFAULT = dict(gate_positive_weight=4, spec_MSE_weight=0.5, spec_MFSE_weight=0.25, postnet_MSE_weight=1.5,
                   postnet_MFSE_weight=0.75, gate_loss_weight=2.0, sylps_kld_weight=0.01, sylps_MSE_weight=0.1,
                   sylps_MAE_weight=0.3, diag_att_weight=0.2, DiagonalGuidedAttention_sigma=0.4)
# name -> (random_inputs arguments, hparams, loss_scalars)
CASES = {
    "small": (dict(B=3, T=37, enc=23, n_mel=80), {}, {}),
    # item 0: the maximal lengths, predicted length (40) below the true one; 1: mel_length 1, predicted length above it;
    # 2: carries decoder state; 3: predicted length (50) above the true one (30), long text, short clip, a third of the text
    # never attended: the missing-encoder punishment applies; 4: text_length <= 12
    "edges": (dict(B=5, T=65, enc=65, n_mel=20, ml=[65, 1, 40, 30, 50], tl=[65, 20, 33, 40, 10], cross=[40, 7, 39, 50, 49],
                   cover=[0.95, 0.9, 0.9, 0.6, 0.9], pres=[0, 0, 1, 0, 0]), {}, {}),
    "weights": (dict(B=2, T=20, enc=12, n_mel=20), NON_DEFAULT,
                {"spec_MSE_weight": 2.0, "gate_loss_weight": None, "diag_att_weight": 0.0}),
}


def away_from_discontinuities(inp):
    """None if the inputs are safe, else the reason."""
    al = inp["alignments"].astype(np.float64)
    top = np.sort(al, axis=2)
    if al.shape[2] > 1 and (top[:, :, -1] - top[:, :, -2]).min() < 1e-4:
        return "two entries of an alignment row within 1e-4 of its maximum"
    sig = 1 / (1 + np.exp(-inp["pred_gate_logits"].astype(np.float64)))
    if np.abs(sig[:, 5:] - 0.7).min(initial=1.0) < 1e-3:
        return "a gate sigmoid within 1e-3 of 0.7"
    pg = sig.copy()
    pg[:, :5] = 0
    plen = tr.first_over_thresh(pg, 0.7)
    ml, tl = inp["mel_lengths"], inp["text_lengths"]
    for cut in (ml, np.minimum(ml, plen)):
        for b in range(al.shape[0]):
            tot = al[b, :cut[b], :tl[b]].sum(axis=0)
            if np.abs(tot - 0.7).min() < 1e-3:
                return "an encoder total within 1e-3 of enc_min_thresh"
    return None


def run_reference(inp, hp, loss_scalars, dtype):
    from CookieTTS._2_ttm.tacotron2_tm.loss_function import Tacotron2Loss
    t = lambda k: torch.from_numpy(np.array(inp[k])).to(dtype)
    B = inp["gt_mel"].shape[0]
    paths = [f"clip_{i}.wav" for i in range(B)]
    pred = {"pred_mel": t("pred_mel"), "pred_mel_postnet": t("pred_mel_postnet"), "pred_gate_logits": t("pred_gate_logits"),
            "pred_sylps": t("pred_sylps").unsqueeze(1), "pred_sylps_mu": t("pred_sylps_mu"), "pred_sylps_logvar": t("pred_sylps_logvar"),
            "alignments": t("alignments")}
    gt = {"gt_mel": t("gt_mel"), "mel_lengths": torch.from_numpy(inp["mel_lengths"].astype(np.int64)),
          "text_lengths": torch.from_numpy(inp["text_lengths"].astype(np.int64)), "gt_gate_logits": t("gt_gate_logits"),
          "gt_sylps": t("gt_sylps"), "pres_prev_state": torch.from_numpy(np.array(inp["pres_prev_state"])),
          "audiopath": paths, "speaker_id_ext": list(range(B))}
    crit = Tacotron2Loss(SimpleNamespace(masked_select=True, **tr.hparams_of(hp)))
    # shim: utils.py:53 parses torch.__version__ with int(); the "+rocm" local tag of this build breaks that parse
    real_version, torch.__version__ = torch.__version__, torch.__version__.split("+")[0]
    try:
        ld, fl = crit(pred, gt, dict(loss_scalars))
    finally:
        torch.__version__ = real_version
    assert list(ld) == list(tr.TERMS), list(ld)
    assert [p for p in paths if "att_score" in fl[p]] == paths[-1:]                  # :285: the last path only
    ld = np.array([float(ld[k]) for k in tr.TERMS], dtype=np.float64)
    flt = np.array([[float(fl[p][k]) for k in tr.FILE_KEYS] for p in paths], dtype=np.float64)
    return ld, flt, float(fl[paths[-1]]["att_score"]), paths


def make(case):
    args, hp, scalars = CASES[case]
    for seed in range(100, 200):
        inp = tr.random_inputs(seed=seed, **args)
        why = away_from_discontinuities(inp)
        if why is None:
            break
        print(f"{case}: seed {seed} refused: {why}")
    else:
        raise SystemExit(f"{case}: no seed keeps away from the discontinuities")
    ld32, fl32, as32, paths = run_reference(inp, hp, scalars, torch.float32)
    ld64, fl64, as64, _ = run_reference(inp, hp, scalars, torch.float64)
    pg = 1 / (1 + np.exp(-inp["pred_gate_logits"].astype(np.float64)))
    pg[:, :5] = 0
    plen = tr.first_over_thresh(pg, 0.7)
    rel = np.abs(ld32 - ld64) / np.maximum(np.abs(ld64), 1e-30)
    print(f"{case}: seed {seed}; fp32 vs fp64 relative, loss_dict: {rel.min():.1e} .. {rel.max():.1e}; pred_len {plen.tolist()}")
    if case == "edges":
        ml, tl = inp["mel_lengths"], inp["text_lengths"]
        r = tr.taco_loss(inp, np.float64, hp, scalars)
        assert ml[1] == 1 and inp["pres_prev_state"][2] == 1 and plen[3] > ml[3] and plen[0] < ml[0] and tl[4] <= 12
        assert tl[3] > 12 and ml[3] < 0.75 * ml.max() and r["metric_pred"][5][3] > 0.08, r["metric_pred"][5]
    hpd = tr.hparams_of(hp)
    out = dict(inp)
    out.update(seed=np.int64(seed), hp_keys=np.array(list(hpd)), hp_vals=np.array([float(v) for v in hpd.values()]),
               scalar_keys=np.array(list(scalars), dtype=str), scalar_vals=np.array([np.nan if v is None else v for v in scalars.values()], dtype=np.float64),
               audiopath=np.array(paths), ld32=ld32, ld64=ld64, ld_e32=np.abs(ld32 - ld64), fl32=fl32, fl64=fl64,
               fl_e32=np.abs(fl32 - fl64), att_score32=np.float64(as32), att_score64=np.float64(as64),
               att_score_e32=np.float64(abs(as32 - as64)), pred_len=plen)
    path = os.path.join(HERE, f"taco_loss_{case}.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for name in sys.argv[1:] or list(CASES):
        make(name)
