"""The T2S server's retry loop on the device: best-of-N selection, the vocoder batch and the int16 PCM tail.

Host side of ``csrc/retry.hip``.  ``_5_infer/t2s_server/text2speech.py:548-651`` runs Tacotron passes until every text has
a candidate that scores ``target_score`` (or a stop rule fires) and reads every candidate back to the host to decide - six
``.item()`` calls and three ``isnan().any()`` reductions per row; :675-695 then convert each utterance to int16 in numpy.
:class:`BestOfN` keeps the loop's state on the device and reads ONE 32-byte status block per pass; :func:`pcm16_concat` is
the tail.  No CPU fallback: a CPU tensor or a missing library raises.
"""
import collections
import ctypes as C

import torch

from . import _lib
from .alignment import get_first_over_thresh, metric_table

__all__ = ["BestOfN", "RetryStatus", "pcm16_concat"]

RetryStatus = collections.namedtuple("RetryStatus", "done n_passes min_best_score min_tries n_without_winner max_best_length "
                                                    "max_best_T")
_SECTIONS = ("status", "best_score", "detail", "tries", "best_length", "best_T", "best_pass", "best_row", "changed", "best_mel",
             "best_alignments", "row_score", "row_detail", "row_flags")
DETAIL_KEYS = ("weighted_score", "diagonality_punishment", "max_dur_punishment", "min_dur_punishment", "avg_dur_punishment",
               "mis_dur_punishment")
PAD_VALUE = -11.52                 # text2speech.py:651


def _device(x, dtype, what):
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.HipLibraryError(f"{what}: expected a CUDA/HIP tensor (this path has no CPU fallback)")
    return x.detach().to(dtype).contiguous()


class BestOfN:
    """State of one request's retry loop (text2speech.py:548-551) for ``n_texts`` texts with ``per_text`` candidates each per
    pass; row ``j * per_text + k`` of a pass is candidate ``k`` of text ``j`` (``repeat_interleave``, :537)."""

    def __init__(self, n_texts, per_text, n_mel, max_decoder_steps, *, max_attempts, target_score, absolute_maximum_tries=2048,
                 absolutely_required_score=-1e3, diagonality_weighting=0.5, max_focus_weighting=1.0, min_focus_weighting=0.5,
                 avg_focus_weighting=1.0, keep_alignments=False, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.HipLibraryError("BestOfN: expected a CUDA/HIP device (this path has no CPU fallback)")
        self.n_texts, self.per_text, self.n_mel = int(n_texts), int(per_text), int(n_mel)
        self.keep_alignments = bool(keep_alignments)
        self._cfg = _lib.RetryConfig(diagonality_weighting, max_focus_weighting, min_focus_weighting, avg_focus_weighting,
                                     target_score, absolutely_required_score, max_attempts, absolute_maximum_tries, self.n_texts,
                                     self.per_text, self.n_mel, int(max_decoder_steps), 0)
        self._state = None
        self.reset()

    def _allocate(self, enc):
        """The state is sized at the first pass: the encoder length of the kept alignments is known only then."""
        lib = _lib.lib()
        self._cfg.enc_cap = int(enc) if self.keep_alignments else 0
        nbytes = _lib.nbytes(lib.ctts_retry_state_bytes, C.byref(self._cfg), what="ctts_retry_state_bytes")
        offsets = (C.c_size_t * len(_SECTIONS))()
        _lib.check(lib.ctts_retry_state_layout(C.byref(self._cfg), offsets), "ctts_retry_state_layout")
        self._off = dict(zip(_SECTIONS, offsets))
        self._state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.reset()

    def _section(self, name, count, dtype):
        n = count * torch.empty(0, dtype=dtype).element_size()
        return self._state[self._off[name]:self._off[name] + n].view(dtype)

    def reset(self):
        """Back to :548-551: no winners, no tries."""
        self._status = RetryStatus(0, 0, -1e5, 0, self.n_texts, 0, 0)
        if self._state is not None:
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().ctts_retry_reset(C.byref(self._cfg), _lib.ptr(self._state), _lib.stream(self.device)),
                           "ctts_retry_reset")

    @property
    def status(self):
        """The status block as of the last :meth:`update` (no device access)."""
        return self._status

    @property
    def done(self):
        return self._status.done != 0

    def update(self, outputs, text_lengths, gate_threshold=0.7, end_mode='thresh', return_detail=False):
        """One pass of :563-625 on the dict ``Tacotron2.inference`` returns (rows = n_texts * per_text); ``text_lengths``
        [n_texts].  Returns the status after ONE host read; with ``return_detail`` also every row's scores (float64 [rows])
        and detail (float64 [rows, 6]) as device tensors."""
        assert end_mode in ('max', 'thresh'), f"end_mode of {end_mode} is not valid."          # :363
        mel = _device(outputs['pred_mel_postnet'], torch.float32, "BestOfN.update")
        gate = _device(outputs['pred_gate'], torch.float32, "BestOfN.update")
        al = _device(outputs['alignments'], torch.float32, "BestOfN.update")
        tl = _device(text_lengths, torch.int32, "BestOfN.update").reshape(-1)
        rows = self.n_texts * self.per_text
        T, enc = al.shape[1], al.shape[2]
        if tuple(mel.shape) != (rows, self.n_mel, T) or tuple(gate.shape) != (rows, T) or al.shape[0] != rows or tl.numel() != self.n_texts:
            raise ValueError(f"BestOfN.update: mel {tuple(mel.shape)}, gate {tuple(gate.shape)}, alignments {tuple(al.shape)}, "
                             f"text_lengths {tuple(tl.shape)} do not fit {self.n_texts} texts x {self.per_text} candidates")
        if self._state is None:
            self._allocate(enc)
        if end_mode == 'thresh':                                                                   # :564-567
            ol = get_first_over_thresh(gate, gate_threshold)
        else:
            ol = gate.argmax(dim=1).to(torch.int32)
        metrics = metric_table(al, input_lengths=tl.repeat_interleave(self.per_text), output_lengths=ol)          # :568
        detail = torch.empty(rows, 6, dtype=torch.float64, device=self.device) if return_detail else None
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ctts_retry_update_f32(C.byref(self._cfg), _lib.ptr(mel), _lib.ptr(gate), _lib.ptr(al),
                                                        _lib.ptr(metrics), _lib.ptr(ol), _lib.ptr(tl), T, enc, _lib.ptr(detail),
                                                        _lib.ptr(self._state), _lib.stream(self.device)), "ctts_retry_update_f32")
        block = self._state[:C.sizeof(_lib.RetryStatus)].cpu().numpy().tobytes()                  # the one host read
        s = _lib.RetryStatus.from_buffer_copy(block)
        self._status = RetryStatus(*(getattr(s, f) for f in RetryStatus._fields))
        if return_detail:
            return self._status, self._section("row_score", rows, torch.float64).clone(), detail
        return self._status

    def _need_state(self, what):
        if self._state is None:
            raise RuntimeError(f"BestOfN.{what}: no pass has been scored yet")

    def best_scores(self):
        """float64 [n_texts] (device): ``best_score`` of :548."""
        self._need_state("best_scores")
        return self._section("best_score", self.n_texts, torch.float64).clone()

    def best_detail(self):
        """What ``best_score_str`` (:606-613, :618) is formatted from, read once at the end: per text a dict of the winner's
        ``DETAIL_KEYS`` plus ``score``, ``tries``, ``output_length``, ``pass`` and ``row``."""
        self._need_state("best_detail")
        n = self.n_texts
        det = self._section("detail", n * 6, torch.float64).cpu().reshape(n, 6).tolist()
        score = self._section("best_score", n, torch.float64).cpu().tolist()
        ints = {k: self._section(k, n, torch.int32).cpu().tolist() for k in ("tries", "best_length", "best_pass", "best_row")}
        return [dict(zip(DETAIL_KEYS, det[j]), score=score[j], tries=ints["tries"][j], output_length=ints["best_length"][j],
                     **{"pass": ints["best_pass"][j], "row": ints["best_row"][j]}) for j in range(n)]

    def best_alignments(self):
        """float32 [n_texts, max_best_T, enc] of the winners (``keep_alignments=True``); rows past a winner's own pass length
        are undefined."""
        self._need_state("best_alignments")
        if not self._cfg.enc_cap:
            raise RuntimeError("BestOfN.best_alignments: built with keep_alignments=False")
        full = self._section("best_alignments", self.n_texts * self._cfg.t_cap * self._cfg.enc_cap, torch.float32)
        return full.view(self.n_texts, self._cfg.t_cap, self._cfg.enc_cap)[:, :self._status.max_best_T].clone()

    def vocoder_batch(self, pad_value=PAD_VALUE):
        """:645-651 -> (mel [n_texts, n_mel, max_length] padded with ``pad_value``, output_lengths int32 [n_texts])."""
        self._need_state("vocoder_batch")
        if self._status.n_without_winner:                                                          # :636
            raise RuntimeError('Tacotron Failed to generate one of the texts after multiple attempts.')
        t_out = self._status.max_best_length
        mel = torch.empty(self.n_texts, self.n_mel, t_out, dtype=torch.float32, device=self.device)
        if t_out > 0:
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().ctts_retry_vocoder_batch_f32(C.byref(self._cfg), _lib.ptr(self._state), _lib.ptr(mel), t_out,
                                                                   float(pad_value), _lib.stream(self.device)),
                           "ctts_retry_vocoder_batch_f32")
        return mel, self._section("best_length", self.n_texts, torch.int32).clone()


def pcm16_concat(audio, output_lengths, hop_length, silence_samples=0):
    """:675-695 for a vocoder batch ``audio`` [B, 1, T] or [B, T] (fp32 or fp16): per row the first ``output_lengths[b] *
    hop_length`` samples, ``silence_samples`` zeros, ``* 2**15`` truncated to int16 - rows back to back, as the server's
    ``sox`` merge leaves them.  Returns (int16 [total], int64 offsets [B + 1], both on the device).  Unlike numpy's
    ``astype('int16')``, values outside the int16 range saturate and NaN gives 0."""
    if not (torch.is_tensor(audio) and audio.is_cuda):
        raise _lib.HipLibraryError("pcm16_concat: expected a CUDA/HIP tensor (this path has no CPU fallback)")
    if audio.dim() == 3 and audio.shape[1] == 1:
        audio = audio[:, 0]
    if audio.dim() != 2 or audio.shape[0] < 1 or audio.shape[1] < 1:
        raise ValueError(f"pcm16_concat expects [B, 1, T] or [B, T], got {tuple(audio.shape)}")
    if audio.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"pcm16_concat takes float32 or float16, got {audio.dtype}")
    audio = audio.detach().contiguous()
    B, ld = audio.shape
    dev = audio.device
    frames = _device(torch.as_tensor(output_lengths).to(dev), torch.int32, "pcm16_concat").reshape(-1)
    if frames.numel() != B:
        raise ValueError(f"pcm16_concat: {frames.numel()} output_lengths for {B} rows")
    cap = B * (ld + int(silence_samples))
    pcm = torch.empty(cap, dtype=torch.int16, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ctts_pcm16_concat(_lib.ptr(audio), int(audio.dtype == torch.float16), _lib.ptr(frames), B, ld,
                                                int(hop_length), int(silence_samples), _lib.ptr(pcm), cap, _lib.ptr(offsets),
                                                _lib.stream(dev)), "ctts_pcm16_concat")
    return pcm[:int(offsets[-1])], offsets
