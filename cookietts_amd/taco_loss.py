"""Tacotron2Loss on the device: score a teacher-forced pass without the host.

Host side of ``csrc/taco_loss.hip``.  ``_2_ttm/tacotron2_tm/loss_function.py:96-290`` consumes the nine-key dict of
``Tacotron2.forward`` and yields the validation loss (``train.py:386-459``), the per-file score table ``file_losses``
(``get_mse_sampled_filelist``, ``train.py:323``) and the inference-style ``weighted_score``.  The reference builds its
guided-attention mask per item in a Python loop on the host, copies the mels three times through ``masked_select`` and reads six
``.item()`` per row; here every per-item number is summed on the device into ONE float64 table, which :meth:`forward` copies to
the host once and :meth:`per_item` hands out without any synchronisation.  No gradient (no backward pass), no CPU fallback.

Unlike the reference, no input is written to: it overwrites ``pred['pred_mel_postnet']`` past the lengths (:200) and
``pred['alignments']`` past the mel lengths (``utils/model/utils.py:81``, through its first ``alignment_metric`` call) in place -
and its second ``alignment_metric`` call (:270) depends on that; the library's masked metric reads the cut instead.
"""
import ctypes as C
import time

import torch
import torch.nn as nn

from . import _lib

__all__ = ["Tacotron2Loss", "COLUMNS", "TERMS"]

# include/cookietts_hip.h: the columns of the per-item table and the batch terms
COLUMNS = ("mel_length", "spec_SE", "postnet_SE", "spec_MFSE", "postnet_MFSE", "gate_BCE", "diag_att", "diag_frames", "sylps_kld",
           "sylps_AE", "sylps_SE", "att_diagonality", "avg_max_attention", "char_max_dur", "char_min_dur", "char_avg_dur",
           "p_missing_enc", "pred_mel_length", "pred_diagonality", "pred_avg_prob", "pred_char_max_dur", "pred_char_min_dur",
           "pred_char_avg_dur", "pred_p_missing_enc", "att_score", "att_score_filled", "spec_MSE")
TERMS = ("spec_MSE", "postnet_MSE", "spec_MFSE", "postnet_MFSE", "gate_loss", "sylps_kld", "sylps_MAE", "sylps_MSE", "diag_att",
         "loss", "diagonality", "avg_max_attention", "weighted_score")
# hparams.py:166, 300-312
DEFAULTS = dict(gate_positive_weight=10, spec_MSE_weight=0.0, spec_MFSE_weight=1.0, postnet_MSE_weight=0.0, postnet_MFSE_weight=1.0,
                gate_loss_weight=1.0, sylps_kld_weight=0.0020, sylps_MSE_weight=0.01, sylps_MAE_weight=0.00, diag_att_weight=0.05,
                DiagonalGuidedAttention_sigma=0.5)
_COL = {k: i for i, k in enumerate(COLUMNS)}


class Tacotron2Loss(nn.Module):
    """``Tacotron2Loss(hparams)`` of loss_function.py:96-137: reads ``gate_positive_weight``, the ``*_weight`` scalars and
    ``DiagonalGuidedAttention_sigma``; an attribute the object lacks takes the reference's default (hparams.py:166, 300-312)."""

    def __init__(self, hparams):
        super().__init__()
        own = {"gate_positive_weight": "pos_weight", "DiagonalGuidedAttention_sigma": "sigma"}      # the reference's attribute names
        for k, default in DEFAULTS.items():
            setattr(self, own.get(k, k), float(getattr(hparams, k, default)))
        self._ws = {}

    # ---------------------------------------------------------------------------------------------- arguments ----
    def _params(self, loss_scalars):
        """:152-161: the scale of a term is the attribute ``<key>_weight`` (1.0 if there is none), overridden by a non-None entry
        of ``loss_scalars``."""
        loss_scalars = {} if loss_scalars is None else loss_scalars
        p = _lib.TacoLossParams()
        p.gate_positive_weight, p.sigma = self.pos_weight, self.sigma
        for i, k in enumerate(TERMS[:9]):
            scale = getattr(self, f"{k}_weight", 1.0)
            if f"{k}_weight" in loss_scalars and loss_scalars[f"{k}_weight"] is not None:
                scale = loss_scalars[f"{k}_weight"]
            p.weights[i] = float(scale)
        return p

    @staticmethod
    def _lengths(x, name, B, limit):
        """int32 device [B].  Values are checked (1 <= length <= limit) where that costs no synchronisation: a list or a host
        tensor.  A device tensor is taken as it is and must hold values of at least 1; the library reads a larger value as
        ``limit`` everywhere (sums, counts and metrics alike) and never reads past T / enc."""
        x = torch.as_tensor(x)
        if x.numel() != B:
            raise ValueError(f"Tacotron2Loss: {name} has {x.numel()} entries for a batch of {B}")
        x = x.detach().reshape(B)
        if not x.is_cuda and B and (int(x.min()) < 1 or int(x.max()) > limit):
            raise ValueError(f"Tacotron2Loss: {name} must lie in [1, {limit}], got [{int(x.min())}, {int(x.max())}]")
        return x

    def _inputs(self, pred, gt):
        big = {"pred_mel": pred["pred_mel"], "pred_mel_postnet": pred["pred_mel_postnet"], "gt_mel": gt["gt_mel"],
               "pred_gate_logits": pred["pred_gate_logits"], "gt_gate_logits": gt["gt_gate_logits"],
               "alignments": pred["alignments"]}
        small = {"pred_sylps_mu": pred["pred_sylps_mu"], "pred_sylps_logvar": pred["pred_sylps_logvar"],
                 "pred_sylps": pred["pred_sylps"], "gt_sylps": gt["gt_sylps"]}
        for k, v in {**big, **small}.items():
            if not torch.is_tensor(v):
                raise ValueError(f"Tacotron2Loss: {k} is not a tensor ({type(v).__name__})")
            if v.requires_grad and torch.is_grad_enabled():
                raise NotImplementedError(f"Tacotron2Loss on the HIP path has no backward pass: {k} requires grad (the validation "
                                          "loss, file_losses and weighted_score need none; call under torch.no_grad() or detach)")
        if gt["gt_mel"].dim() != 3:
            raise ValueError(f"Tacotron2Loss: gt_mel must be [B, n_mel, T], got {tuple(gt['gt_mel'].shape)}")
        B, n_mel, T = gt["gt_mel"].shape
        if big["alignments"].dim() != 3 or tuple(big["alignments"].shape[:2]) != (B, T) or big["alignments"].shape[2] < 1:
            raise ValueError(f"Tacotron2Loss: alignments must be [B, T, enc] = [{B}, {T}, enc], got {tuple(big['alignments'].shape)}")
        enc = big["alignments"].shape[2]
        if min(B, n_mel, T) < 1:
            raise ValueError(f"Tacotron2Loss: gt_mel {tuple(gt['gt_mel'].shape)} has an empty dimension")
        for k in ("pred_mel", "pred_mel_postnet"):
            if tuple(big[k].shape) != (B, n_mel, T):
                raise ValueError(f"Tacotron2Loss: {k} {tuple(big[k].shape)} does not match gt_mel {(B, n_mel, T)}")
        for k in ("pred_gate_logits", "gt_gate_logits"):
            if tuple(big[k].shape) != (B, T):
                raise ValueError(f"Tacotron2Loss: {k} {tuple(big[k].shape)} is not [B, T] = {(B, T)}")
        for k, v in small.items():
            if v.numel() != B:
                raise ValueError(f"Tacotron2Loss: {k} {tuple(v.shape)} does not hold one value per item (B = {B})")
        ml = self._lengths(gt["mel_lengths"], "mel_lengths", B, T)
        tl = self._lengths(gt["text_lengths"], "text_lengths", B, enc)
        pres = gt.get("pres_prev_state")
        if pres is not None and torch.as_tensor(pres).numel() != B:
            raise ValueError(f"Tacotron2Loss: pres_prev_state has {torch.as_tensor(pres).numel()} entries for a batch of {B}")
        for k, v in {**big, **small}.items():
            if not v.is_cuda:
                raise _lib.HipLibraryError(f"Tacotron2Loss: {k}: expected a CUDA/HIP tensor (this path has no CPU fallback)")
        dev = big["gt_mel"].device
        f32 = lambda v: v.detach().to(device=dev, dtype=torch.float32).contiguous()
        t = {k: f32(v) for k, v in big.items()}
        t.update({k: f32(v).reshape(B) for k, v in small.items()})
        t["mel_lengths"] = ml.to(device=dev, dtype=torch.int32).contiguous()
        t["text_lengths"] = tl.to(device=dev, dtype=torch.int32).contiguous()
        t["pres_prev_state"] = (torch.zeros(B, dtype=torch.float32, device=dev) if pres is None
                                else f32(torch.as_tensor(pres)).reshape(B))
        return t, (B, n_mel, T, enc), dev

    def _workspace(self, dev, geom):
        key = (dev,) + geom
        if key not in self._ws:
            n = _lib.nbytes(_lib.lib().ctts_taco_loss_workspace_bytes, *geom, what="ctts_taco_loss_workspace_bytes")
            self._ws[key] = torch.empty(n, dtype=torch.uint8, device=dev)
        return self._ws[key]

    # ---------------------------------------------------------------------------------------------- the calls ----
    def _run(self, pred, gt, loss_scalars=None, metrics=None):
        t, geom, dev = self._inputs(pred, gt)
        B = geom[0]
        ws = self._workspace(dev, geom)
        table = torch.empty(B, len(COLUMNS), dtype=torch.float64, device=dev)
        terms = torch.empty(len(TERMS), dtype=torch.float64, device=dev)
        p = self._params(loss_scalars)
        lib = _lib.lib()
        small = [_lib.ptr(t[k]) for k in ("pred_sylps_mu", "pred_sylps_logvar", "pred_sylps", "gt_sylps", "mel_lengths",
                                          "text_lengths", "pres_prev_state")]
        with torch.cuda.device(dev):
            stream = _lib.stream(dev)
            if metrics is None:
                _lib.check(lib.ctts_taco_loss_f32(C.byref(p), *(_lib.ptr(t[k]) for k in (
                    "pred_mel", "pred_mel_postnet", "gt_mel", "pred_gate_logits", "gt_gate_logits", "alignments")), *small, *geom,
                    _lib.ptr(table), _lib.ptr(terms), _lib.ptr(ws), ws.numel(), stream), "ctts_taco_loss_f32")
            else:
                m = [None if x is None else x.detach().to(device=dev, dtype=torch.float64).contiguous() for x in metrics]
                for x in m:
                    if x is not None and tuple(x.shape) != (B, 6):
                        raise ValueError(f"Tacotron2Loss.finalize: a metric table must be [B, 6] = [{B}, 6], got {tuple(x.shape)}")
                _lib.check(lib.ctts_taco_loss_finalize_f32(C.byref(p), _lib.ptr(m[0]), _lib.ptr(m[1]), *small, *geom, _lib.ptr(table),
                                                           _lib.ptr(terms), _lib.ptr(ws), ws.numel(), stream),
                           "ctts_taco_loss_finalize_f32")
        return table, terms

    def per_item(self, pred, gt):
        """-> (float64 [B, K] device table, ``COLUMNS``), no host synchronisation.  Every item's own numbers: the ``att_score``
        the reference drops (:285), both metric rows, the predicted length, and the per-item sums and counts each batch term is
        formed from.  A row does not depend on the other items except for ``att_score_filled`` (the NaN substitute, :287) and the
        ``max(mel_lengths)`` inside ``att_score`` (:281).  This is what a dataset sweep wants; :meth:`forward` is built on it."""
        return self._run(pred, gt)[0], COLUMNS

    def finalize(self, pred, gt, metric_gt=None, metric_pred=None, loss_scalars=None):
        """The finalize launch alone on other metric tables (float64 [B, 6], the form ``alignment.metric_table`` returns; None =
        the call's own) -> (table, float64 terms in the order of ``TERMS``).  A test and inspection hook: it must directly follow a
        :meth:`per_item` / :meth:`forward` call ON THE SAME ``pred`` AND ``gt`` - the tile partials and the predicted lengths are
        whatever the last call at this geometry left in the cached workspace; only the small ``[B]`` vectors are read afresh."""
        key = (pred["alignments"].device,) + tuple(gt["gt_mel"].shape) + (pred["alignments"].shape[2],)
        if key not in self._ws:
            raise RuntimeError("Tacotron2Loss.finalize: no call at this geometry has filled a workspace yet")
        return self._run(pred, gt, loss_scalars, metrics=(metric_gt, metric_pred))

    def forward(self, pred, gt, loss_scalars=None):   # no torch.no_grad() here: the refusal of grad-carrying inputs must see the caller's mode
        """loss_function.py:167-290 -> (loss_dict, file_losses).  ``pred``: the dict of ``Tacotron2.forward``; ``gt``: ``gt_mel``,
        ``mel_lengths``, ``text_lengths``, ``gt_gate_logits``, ``gt_sylps``, ``pres_prev_state``, ``audiopath``,
        ``speaker_id_ext``.  ``loss_dict``: the reference's thirteen keys as 0-dim float32 device tensors, each rounded once from
        the float64 value.  ``file_losses``: Python floats per audiopath from ONE device-to-host copy.
        ``T > max(mel_lengths)`` is accepted (mel terms are masked by length; the reference needs ``T == max(mel_lengths)``, and
        there the two agree).

        :285 as written: ``file_losses[audiopath]['att_score'] = weighted_score`` sits in a loop over ``i`` that never rebinds
        ``audiopath`` - the variable is stale from the loop of :257-264 - so ``att_score`` lands only on the LAST path of the
        batch, and holds the last item's score.  Every item's own score is column ``att_score`` of :meth:`per_item`."""
        for k in ("audiopath", "speaker_id_ext"):
            if k not in gt or len(gt[k]) != gt["gt_mel"].shape[0]:
                raise ValueError(f"Tacotron2Loss: gt[{k!r}] must hold one entry per item")
        table, terms = self._run(pred, gt, loss_scalars)
        t32 = terms.to(torch.float32)
        loss_dict = {k: t32[i] for i, k in enumerate(TERMS)}
        rows = table.cpu().tolist()                                         # the one host read
        B = len(rows)
        file_losses = {}
        for i in range(B):                                                  # :173-176
            path = gt["audiopath"][i]
            if path not in file_losses:
                file_losses[path] = {"speaker_id_ext": gt["speaker_id_ext"][i], "time": time.time()}
        for i in range(B):                                                  # :195-197, :257-264
            f = file_losses[gt["audiopath"][i]]
            f["spec_MSE"] = rows[i][_COL["spec_MSE"]]
            for k in ("avg_max_attention", "att_diagonality", "p_missing_enc", "char_max_dur", "char_min_dur", "char_avg_dur"):
                f[k] = rows[i][_COL[k]]
        file_losses[gt["audiopath"][B - 1]]["att_score"] = rows[B - 1][_COL["att_score"]]          # :285, stale loop variable
        return loss_dict, file_losses
