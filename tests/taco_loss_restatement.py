"""numpy restatement of the reference's ``Tacotron2Loss.forward`` (_2_ttm/tacotron2_tm/loss_function.py:167-290) with the two
helpers it calls (utils/model/utils.py:47-56 ``get_first_over_thresh``, :59-120 ``alignment_metric``), parameterised by dtype.

``taco_loss(inp, dtype)`` evaluates the loss with every tensor in ``dtype`` (float32: the arithmetic of the reference as it runs;
float64: the arithmetic of the reference handed ``.double()`` inputs).  What the reference keeps in float32 whatever it is handed
stays float32 here too: the arg-max track and its path length (:74-78), the guided-attention weights (:70-72, built from
``.float()`` grids), the gate fed to ``get_first_over_thresh`` (:50), ``p_missing_enc`` (:103), and ``torch.tensor(scores)``
(:286).  Reductions use numpy's pairwise sums, so float32 results differ from torch's by summation order only.

Restated as written:
  * the FIRST ``alignment_metric`` call (:251) zeroes its argument past ``mel_lengths`` in place (utils.py:81), and the SECOND
    call (:270) scores that tensor against the length predicted from the gate - an item whose predicted length exceeds its true
    length gets zero rows there (arg-max 0, value 0);
  * :285 ``file_losses[audiopath]['att_score']`` uses the loop variable of :257-264, stale: the score lands on the LAST path only
    (``file_losses`` below).
``T > max(mel_lengths)`` is accepted (masks are built at width T), where the reference needs equality.

``perturb`` (a set of names) breaks the restatement ON PURPOSE, one mistake each; tests/test_taco_loss.py asserts on the goldens
that each moves some key by far more than its bound:
  'second_metric_unmasked'  the second metric call reads the alignments as they came, not as the first call left them
  'gate_masked'             the gate term averaged over frames t < mel_length only
  'guided_batch_max'        the guided-attention grid normalised by the batch's maximal lengths, not the item's own
  'no_pos_weight'           BCEWithLogits without pos_weight
  'pres_ignored'            items with pres_prev_state != 0 take part in the guided-attention term
  'mfse_batch_mean'         the MFSE frame mean taken over the whole batch
"""
from __future__ import annotations

import os
import warnings

import numpy as np

F32 = np.float32
F64 = np.float64
FACTOR = 8                      # the project's factor on e32 (tests/ax_cond_f64_restatement.py:50)
EPS32 = 2.0 ** -23
PERTURBATIONS = ("second_metric_unmasked", "gate_masked", "guided_batch_max", "no_pos_weight", "pres_ignored", "mfse_batch_mean")

TERMS = ("spec_MSE", "postnet_MSE", "spec_MFSE", "postnet_MFSE", "gate_loss", "sylps_kld", "sylps_MAE", "sylps_MSE", "diag_att",
         "loss", "diagonality", "avg_max_attention", "weighted_score")
FILE_KEYS = ("spec_MSE", "avg_max_attention", "att_diagonality", "p_missing_enc", "char_max_dur", "char_min_dur", "char_avg_dur")
INPUT_KEYS = ("pred_mel", "pred_mel_postnet", "gt_mel", "pred_gate_logits", "gt_gate_logits", "alignments", "pred_sylps_mu",
              "pred_sylps_logvar", "pred_sylps", "gt_sylps", "mel_lengths", "text_lengths", "pres_prev_state")
# hparams.py:166, 300-312
HP_DEFAULTS = dict(gate_positive_weight=10, spec_MSE_weight=0.0, spec_MFSE_weight=1.0, postnet_MSE_weight=0.0,
                   postnet_MFSE_weight=1.0, gate_loss_weight=1.0, sylps_kld_weight=0.0020, sylps_MSE_weight=0.01,
                   sylps_MAE_weight=0.00, diag_att_weight=0.05, DiagonalGuidedAttention_sigma=0.5)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("small", "edges", "weights")


def bound(e32, y64):
    """The project's parity bound: FACTOR * max(|fp32 reference - fp64 reference|, 4 ulp of the fp64 value)."""
    return FACTOR * np.maximum(np.asarray(e32, F64), 4 * EPS32 * np.abs(np.asarray(y64, F64)))


def first_over_thresh(x, threshold):
    """utils.py:47-56 (the branch for torch >= 1.7): float32 whatever comes in; the last step always qualifies."""
    x = np.array(x, dtype=F32)
    x[:, -1] = threshold
    x[x > F32(threshold)] = threshold
    return x.argmax(axis=1).astype(np.int32)


def _rdiv(n, lengths):
    """``n / lengths.float()`` with a Python int on the left: torch's ``__rtruediv__`` is ``reciprocal() * n``, in float32."""
    return (F32(1) / np.asarray(lengths).astype(F32)) * F32(n)


def alignment_metric(al, in_len, out_len, thresh=0.7):
    """utils.py:59-120 on ``al`` [B, dec, enc], which is MODIFIED in place as the reference's argument is (:81).
    -> diagonalitys (float64), avg_prob, max / min / avg focus (dtype of ``al``), p_missing_enc (float32)."""
    dt = al.dtype
    B, dec, enc = al.shape
    in_len, out_len = np.asarray(in_len), np.asarray(out_len)
    opt = np.sqrt(in_len.astype(F64) ** 2 + out_len.astype(F64) ** 2)                       # :69
    values = al.max(axis=2)                                                                 # :72
    idx = al.argmax(axis=2).astype(F32)                                                     # first maximal index; :74
    prev = np.concatenate([idx[:, :1], idx[:, :-1]], axis=1)
    dist = np.sqrt((prev - idx) ** 2 + F32(1))                                              # float32
    omask = np.arange(dec)[None, :] < out_len[:, None]
    dist[~omask] = 0
    diag = (dist.sum(axis=1, dtype=F32) + F32(1.4142135)).astype(F64) / opt                 # :79
    al[~omask] = 0                                                                          # :81, in place
    tot = al.sum(axis=1)                                                                    # [B, enc]
    imask = np.arange(enc)[None, :] < in_len[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        tot[~imask] = 0
        emax = tot.max(axis=1)
        eavg = tot.mean(axis=1) * _rdiv(enc, in_len).astype(dt)                             # :89-90
        tot[~imask] = 1
        emin = tot.min(axis=1)
        values[~omask] = 0
        avg_prob = values.mean(axis=1) * _rdiv(dec, out_len).astype(dt)                     # :98-99
        tot[~imask] = 1e3
        pmiss = (tot < thresh).sum(axis=1).astype(F32) / in_len.astype(F32)                 # :103
    return diag, avg_prob, emax, emin, eavg, pmiss


def _sigmoid(x):
    return 1 / (1 + np.exp(-x))


def hparams_of(hp=None):
    """dict of the eleven attributes the loss reads; ``hp``: None, a dict or an attribute object."""
    out = dict(HP_DEFAULTS)
    if hp is not None:
        for k in HP_DEFAULTS:
            if isinstance(hp, dict) and k in hp:
                out[k] = hp[k]
            elif not isinstance(hp, dict) and hasattr(hp, k):
                out[k] = getattr(hp, k)
    return out


def taco_loss(inp, dtype, hp=None, loss_scalars=None, perturb=()):
    """-> dict: ``loss_dict`` {13 keys: scalar}, ``per_item`` {FILE_KEYS + 'att_score': [B]}, ``pred_len`` int32 [B],
    ``metric_gt`` / ``metric_pred`` (the two six-tuples)."""
    perturb = set(perturb)
    assert perturb <= set(PERTURBATIONS), perturb
    hp = hparams_of(hp)
    loss_scalars = loss_scalars or {}
    dt = np.dtype(dtype).type
    c = lambda k: np.asarray(inp[k], dtype=dt)
    pred_mel, post, gt_mel = c("pred_mel"), c("pred_mel_postnet"), c("gt_mel")
    gate, target, al_in = c("pred_gate_logits"), c("gt_gate_logits"), c("alignments")
    ml, tl = np.asarray(inp["mel_lengths"]).astype(np.int64), np.asarray(inp["text_lengths"]).astype(np.int64)
    pres = np.asarray(inp["pres_prev_state"]).astype(F32)
    B, n_mel, T = gt_mel.shape
    ld = {}
    item = {}
    with np.errstate(divide="ignore", invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        # ---- mel terms (:185-213)
        fm = np.arange(T)[None, :] < ml[:, None]                                            # [B, T]
        m3 = np.broadcast_to(fm[:, None, :], gt_mel.shape)
        g = gt_mel[m3]
        se = (pred_mel[m3] - g) ** 2
        ld["spec_MSE"] = se.mean()
        parts = np.split(se, np.cumsum(ml * n_mel)[:-1])
        item["spec_MSE"] = np.array([p.mean() for p in parts], dtype=dt)                    # :194-197
        ld["postnet_MSE"] = ((post[m3] - g) ** 2).mean()
        for key, x in (("spec_MFSE", pred_mel), ("postnet_MFSE", post)):
            ae = np.abs(x - gt_mel).transpose(0, 2, 1)[fm]                                  # [sum(ml), n_mel]
            fmean = ae.mean(dtype=dt) if "mfse_batch_mean" in perturb else ae.mean(axis=1, keepdims=True)
            ld[key] = (ae * fmean).mean()
        # ---- gate (:216-218): the whole [B, T]; BCEWithLogits with pos_weight in its overflow-safe form
        x, y = gate.reshape(-1), target.reshape(-1)
        pw = dt(1 if "no_pos_weight" in perturb else hp["gate_positive_weight"])
        bce = (1 - y) * x + ((pw - 1) * y + 1) * (np.log1p(np.exp(-np.abs(x))) + np.maximum(-x, 0))
        ld["gate_loss"] = bce[fm.reshape(-1)].mean() if "gate_masked" in perturb else bce.mean()
        # ---- SylpsNet (:221-232)
        mu, lv, ps, gs = (c(k).reshape(B) for k in ("pred_sylps_mu", "pred_sylps_logvar", "pred_sylps", "gt_sylps"))
        ld["sylps_kld"] = dt(-0.5) * (1 + lv - np.exp(lv) - mu ** 2).sum() / B
        ld["sylps_MAE"] = np.abs(ps - gs).mean()
        ld["sylps_MSE"] = ((ps - gs) ** 2).mean()
        # ---- guided attention (:37-72, :234-241): float32 weights per item, summed in dt
        keep = np.ones(B, bool) if "pres_ignored" in perturb else pres == 0
        sigma = hp["DiagonalGuidedAttention_sigma"]
        num = dt(0)
        for b in np.flatnonzero(keep):
            ilen, olen = int(tl[b]), int(ml[b])
            ni, no = (int(tl[keep].max()), int(ml[keep].max())) if "guided_batch_max" in perturb else (ilen, olen)
            gx, gy = np.arange(olen, dtype=F32)[:, None], np.arange(ilen, dtype=F32)[None, :]
            w = F32(1.0) - np.exp(-(gy / F32(ni) - gx / F32(no)) ** 2 / F32(2 * (sigma ** 2)))
            num = num + (w.astype(dt) * al_in[b, :olen, :ilen]).sum()
        ld["diag_att"] = num / dt(ml[keep].sum())
        # ---- :152-161
        loss = None
        for k in TERMS[:9]:
            scale = hp.get(f"{k}_weight", 1.0)
            if loss_scalars.get(f"{k}_weight") is not None:
                scale = loss_scalars[f"{k}_weight"]
            loss = ld[k] * dt(scale) if loss is None else loss + ld[k] * dt(scale)
        ld["loss"] = loss
        # ---- metrics (:249-288)
        al = al_in.copy()
        m1 = alignment_metric(al, tl, ml)                                                   # cuts `al` at mel_lengths in place
        ld["diagonality"] = m1[0].mean()
        ld["avg_max_attention"] = m1[1].mean()
        for k, j in (("avg_max_attention", 1), ("att_diagonality", 0), ("p_missing_enc", 5), ("char_max_dur", 2),
                     ("char_min_dur", 3), ("char_avg_dur", 4)):
            item[k] = m1[j]
        pg = _sigmoid(gate)
        pg[:, :5] = 0
        plen = first_over_thresh(pg, 0.7)
        m2 = alignment_metric(al_in.copy() if "second_metric_unmasked" in perturb else al, tl, plen)
        scores = []
        lim = F32(ml.max()) * F32(0.75)                                                     # int tensor * 0.75: float32
        for i in range(B):                                                                  # :274-284, Python floats
            diag, avg_prob, emax, emin, eavg, pmiss = (float(m[i]) for m in m2)
            w = avg_prob
            p1 = max(diag - 1.10, 0) * 0.25
            p2 = max(emax - 60.0, 0) * 0.005
            p3 = max(0.00 - emin, 0) * 0.5
            p4 = max(3.60 - eavg, 0)
            p5 = max(pmiss - 0.08, 0) if tl[i] > 12 and ml[i] < lim else 0.0
            w -= (p1 + p2 + p3 + p4 + p5)
            scores.append(w)
        item["att_score"] = np.array(scores, dtype=F64)
        s32 = np.array(scores, dtype=F32)                                                   # torch.tensor(scores)
        nan = np.isnan(s32)
        s32[nan] = s32[~nan].mean() if (~nan).any() else F32(np.nan)                        # :287
        ld["weighted_score"] = s32.mean()
    return {"loss_dict": ld, "per_item": item, "pred_len": plen, "metric_gt": m1, "metric_pred": m2, "scores_filled": s32}


def file_losses(per_item, audiopath, speaker_id_ext=None):
    """The dict of :170-176, :195-197, :257-264 and :285 - ``att_score`` on the last path only (stale loop variable)."""
    B = len(audiopath)
    out = {}
    for i in range(B):
        if audiopath[i] not in out:
            out[audiopath[i]] = {"speaker_id_ext": None if speaker_id_ext is None else speaker_id_ext[i]}
    for i in range(B):
        for k in FILE_KEYS:
            out[audiopath[i]][k] = float(per_item[k][i])
    out[audiopath[B - 1]]["att_score"] = float(per_item["att_score"][B - 1])
    return out


# ---- goldens ------------------------------------------------------------------------------------------------------------
_CACHE = {}


def load_golden(case):
    """tests/golden/taco_loss_<case>.npz, loaded once and shared (never modified): inputs, ``hp`` / ``loss_scalars`` dicts, the
    reference's float32 and float64 outputs and ``e32`` per value."""
    if case not in _CACHE:
        z = np.load(os.path.join(GOLDEN, f"taco_loss_{case}.npz"))
        g = {k: z[k] for k in z.files}
        g["hp"] = {str(k): float(v) for k, v in zip(g.pop("hp_keys"), g.pop("hp_vals"))}
        g["loss_scalars"] = {str(k): (None if np.isnan(v) else float(v)) for k, v in zip(g.pop("scalar_keys"), g.pop("scalar_vals"))}
        g["audiopath"] = [str(p) for p in g["audiopath"]]
        _CACHE[case] = g
    return _CACHE[case]


def random_inputs(B, T, enc, n_mel, seed, ml=None, tl=None, cross=None, cover=None, pres=None):
    """Seeded ragged inputs in the form of the goldens (peaked, roughly monotonic attention maps with noise; gates that cross
    0.7 before, at or after the true length; item 0 holds the maximal lengths).  Optional per-item lists: the lengths, the
    frame at which the gate crosses, the share of the text the attention track covers within the true length."""
    rng = np.random.default_rng(seed)
    r_ml = rng.integers(max(1, T // 3), T + 1, B)
    r_tl = rng.integers(max(1, enc // 3), enc + 1, B)
    r_ml[0], r_tl[0] = T, enc
    ml = r_ml if ml is None else np.asarray(ml)
    tl = r_tl if tl is None else np.asarray(tl)
    r_cover = rng.uniform(0.7, 1.0, B)
    cover = r_cover if cover is None else np.asarray(cover, dtype=F64)
    gt = rng.normal(-5.0, 2.0, (B, n_mel, T))
    pred = gt + rng.normal(0, 0.4, gt.shape)
    post = gt + rng.normal(0, 0.25, gt.shape)
    pos = np.linspace(0, 1, T)[None, :, None] * ((tl - 1) * (T / np.maximum(ml, 1)) * cover)[:, None, None]
    pos = np.minimum(pos, (tl - 1)[:, None, None])
    e = np.arange(enc)[None, None, :]
    logits = -0.5 * ((e - pos) / rng.uniform(0.6, 1.5, (B, 1, 1))) ** 2 + rng.normal(0, 0.3, (B, T, enc))
    al = np.exp(logits - logits.max(-1, keepdims=True))
    al = al / al.sum(-1, keepdims=True)
    gate = rng.uniform(-4.0, -0.5, (B, T))
    target = np.zeros((B, T))
    for b in range(B):
        r_cross = int(np.clip(ml[b] - 1 + rng.integers(-4, 5), 0, T - 1))
        at = r_cross if cross is None else int(cross[b])
        gate[b, at:] = rng.uniform(1.5, 4.0, T - at)
        target[b, ml[b] - 1:] = 1.0
    f = lambda a: np.ascontiguousarray(a, dtype=F32)
    return {"pred_mel": f(pred), "pred_mel_postnet": f(post), "gt_mel": f(gt), "pred_gate_logits": f(gate), "gt_gate_logits": f(target),
            "alignments": f(al), "pred_sylps_mu": f(rng.normal(0, 0.5, B)), "pred_sylps_logvar": f(rng.normal(-1, 0.5, B)),
            "pred_sylps": f(rng.uniform(2, 8, B)), "gt_sylps": f(rng.uniform(2, 8, B)), "mel_lengths": ml.astype(np.int32),
            "text_lengths": tl.astype(np.int32), "pres_prev_state": np.zeros(B, F32) if pres is None else np.asarray(pres, F32)}
