"""DTW on the device: time-warp a batch of predicted mels onto the ground truth, frame by frame.

Host side of ``csrc/dtw.hip``.  The reference runs ``DTW`` (``_4_mtw/waveglow/mel2samp.py:81-118``) wherever a vocoder meets mels that
a Tacotron wrote: ``_4_mtw/waveglow/train.py:232-236`` (``validate()``: ``DTW(mel, gt_mel, scale_factor=8, range_=5)``),
``_4_mtw/hifigan/meldataset.py:188`` (``DTW(mel, gt_mel, 5, 3)``, the GTA mels a HiFi-GAN is fine-tuned on) and
``utils/dataset/data_utils.py:257-293, 684-686`` (``dtw_scale_factor=5, dtw_range=5``).  It is a Python loop per item there - pad,
``F.interpolate``, ``scale_factor * range_`` strided slices and an ``l1_loss`` / ``sum`` / ``where`` triple per slice; here it is one
launch for the batch.  No gradient, no CPU fallback, no synchronisation.

Stated divergences from the reference loop: the interpolation weights of candidate ``j`` are formed once, at frame 0, instead of at every
expanded index (in fp32 they differ in the last bits where ``1 / scale_factor`` is inexact), and the channel sums run in the kernel's
fixed order; the batch may be ragged (``lengths``), item ``b`` then being treated as the reference treats ``pred[b, :, :lengths[b]]``
alone.  A length given as a DEVICE tensor is not checked: the kernel reads a value outside ``[1, T]`` as the nearest bound.
"""
import torch

from . import _lib

__all__ = ["DTW", "MAX_CANDIDATES"]

MAX_CANDIDATES = 64      # scale_factor * range_ of an accepted call (the reference uses 40, 25 and 15)


def _lengths(lengths, B, T, dev):
    if lengths is None:
        return None
    x = torch.as_tensor(lengths)
    if x.numel() != B:
        raise ValueError(f"DTW: lengths has {x.numel()} entries for a batch of {B}")
    x = x.detach().reshape(B)
    if not x.is_cuda:
        for b, v in enumerate(x.tolist()):
            if not 1 <= int(v) <= T:
                raise ValueError(f"DTW: lengths[{b}] = {int(v)} must lie in [1, {T}]")
    return x.to(device=dev, dtype=torch.int32).contiguous()


def _run(batch_pred, batch_target, scale_factor, range_, lengths=None, return_info=False, generic=False):
    assert range_ % 2 == 1, 'range_ must be an odd integer.'
    assert batch_pred.shape == batch_target.shape, 'pred and target shapes must match.'
    named = {"batch_pred": batch_pred, "batch_target": batch_target}
    for k, v in named.items():
        if not torch.is_tensor(v):
            raise ValueError(f"DTW: {k} is not a tensor ({type(v).__name__})")
        if not v.is_floating_point():
            raise ValueError(f"DTW: {k} must be a floating-point tensor, got {v.dtype}")
        if v.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError(f"DTW on the HIP path has no backward pass: {k} requires grad (call under torch.no_grad() or "
                                      "detach)")
    if batch_pred.dim() != 3 or min(batch_pred.shape) < 1:
        raise ValueError(f"DTW: batch_pred must be [B, C, T] with no empty dimension, got {tuple(batch_pred.shape)}")
    scale_factor, range_ = int(scale_factor), int(range_)
    if scale_factor < 1 or range_ < 1 or scale_factor * range_ > MAX_CANDIDATES:
        raise ValueError(f"DTW: scale_factor = {scale_factor}, range_ = {range_}: both must be at least 1 and their product at most "
                         f"{MAX_CANDIDATES}")
    B, C, T = batch_pred.shape
    for k, v in named.items():
        if not v.is_cuda:
            raise _lib.HipLibraryError(f"DTW: {k}: expected a CUDA/HIP tensor (this path has no CPU fallback)")
    dev = batch_pred.device
    lengths = _lengths(lengths, B, T, dev)
    pred = batch_pred.detach().to(dtype=torch.float32).contiguous()
    target = batch_target.detach().to(device=dev, dtype=torch.float32).contiguous()
    out = torch.empty_like(pred)
    choice = l1 = None
    if return_info:
        choice = torch.empty(B, T, dtype=torch.int32, device=dev)
        l1 = torch.empty(B, 2, T, dtype=torch.float32, device=dev)
    lib = _lib.lib()
    fn = lib.ctts_mel_dtw_generic_f32 if generic else lib.ctts_mel_dtw_f32
    with torch.cuda.device(dev):
        _lib.check(fn(_lib.ptr(pred), _lib.ptr(target), _lib.ptr(lengths), _lib.ptr(out), _lib.ptr(choice), _lib.ptr(l1), B, C, T,
                      scale_factor, range_, _lib.stream(dev)), "ctts_mel_dtw_f32")
    out = out.to(batch_pred.dtype)
    if return_info:
        return out, {"choice": choice, "l1_before": l1[:, 0], "l1_after": l1[:, 1]}
    return out


def DTW(batch_pred, batch_target, scale_factor, range_, lengths=None, return_info=False):
    """``mel2samp.DTW(batch_pred, batch_target, scale_factor, range_)`` -> the aligned copy of ``batch_pred`` ``[B, C, T]``: at every
    frame the candidate - ``batch_pred`` shifted by up to ``range_ / 2`` frames in steps of ``1 / scale_factor``, linearly interpolated,
    zeros past both ends - whose L1 distance from ``batch_target``'s frame is smallest; the unshifted frame wins every tie, an earlier
    candidate a tie with a later one.  Device tensors of any float dtype, computed in fp32 and returned in the input's dtype;
    non-contiguous inputs are made contiguous.  ``lengths`` ``[B]`` (frames per item; list, host or device tensor): item ``b`` is
    aligned as ``batch_pred[b, :, :lengths[b]]`` alone would be and columns past its length are copied from ``batch_pred``.
    ``return_info=True`` -> ``(out, info)`` with the device tensors ``choice`` (int32 ``[B, T]``: the winning candidate, ``-1`` for the
    unshifted frame and past an item's length), ``l1_before`` and ``l1_after`` (fp32 ``[B, T]``: the L1 of the unshifted frame and of
    the winner).  Nothing is synchronised (``lengths`` given as a list or host tensor are checked on the host and copied to the device;
    given as a device tensor they are neither read nor checked here)."""
    return _run(batch_pred, batch_target, scale_factor, range_, lengths, return_info)
