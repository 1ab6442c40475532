"""Vocoder validation score on the device: multi-window log-mel MSE / MAE of a ragged batch.

Host side of ``csrc/mel_error.hip``.  The reference judges a vocoder by the log-mel error between generated and ground-truth audio:
``_4_mtw/waveglow/train.py:184-341`` (``validate()``) compares two ``TacotronSTFT.mel_spectrogram`` results per validation file and
per window of ``data_config['validation_windows']`` and reads two ``.item()`` per pair - ``average_MSE`` drives its LR scheduler and
best-model selection (:666-690); ``_4_mtw/hifigan/train.py:205-223`` takes ``F.l1_loss(y_mel, STFT.get_mel(y_g_hat))`` per batch,
with the framing of ``nvSTFT.get_mel``.  Here a whole batch of files with their own lengths is scored in one call: every number is
summed in float64 on the device, in a fixed order, into ONE table which :meth:`MelSpectrogramError.forward` copies to the host once
and :meth:`MelSpectrogramError.per_item` hands out without any synchronisation.  No gradient, no CPU fallback.

Stated divergences from the reference loops: the batch is ragged (each item is reflect-padded at its own end, and item ``b`` scored in a
padded batch equals item ``b`` scored alone, bit for bit); no input tensor is written to (:259-260 are applied as the audio is
read); lengths given as device tensors are not checked (see :meth:`MelSpectrogramError._lengths`).
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from .audio import STFT, slaney_mel_filterbank

__all__ = ["MelSpectrogramError", "COLUMNS", "TERMS"]

# include/cookietts_hip.h: the columns of a (item, window) row and the batch terms behind the rows
COLUMNS = ("n_frames", "SAE", "SSE", "MAE", "MSE")
TERMS = ("average_MSE", "average_MAE") + tuple(f"l1_{w}" for w in range(8))
FRAMINGS = {"tacotron": 0, "nv": 1}
_COL = {k: i for i, k in enumerate(COLUMNS)}


class MelSpectrogramError(nn.Module):
    """``windows``: the ``filter_length`` of each STFT (1 to 8 of them, train.py:402-407); each ``win_length`` equals its window
    unless ``win_lengths`` is given.  The defaults are ``validate()``'s own.  ``framing="tacotron"`` is ``utils/audio/stft.py:79-111,
    180-207`` (reflect-pad ``N/2``, ``T // hop + 1`` frames); ``framing="nv"`` is ``hifigan/nvSTFT.py:92-101`` (reflect-pad
    ``int((n_fft - hop) / 2)``, no centring, ``(T + 2 pad - n_fft) // hop + 1`` frames, magnitude ``sqrt(re^2 + im^2 + 1e-9)``, the
    Hann window of ``win_size`` zero-padded centrally to ``n_fft``).  The mel filterbank is ``audio.slaney_mel_filterbank``."""

    def __init__(self, windows, hop_length, sampling_rate, n_mel_channels=160, mel_fmin=0.0, mel_fmax=16000.0, clamp_val=1e-5,
                 win_lengths=None, framing="tacotron"):
        super().__init__()
        windows = [int(w) for w in windows]
        if not 1 <= len(windows) <= 8:
            raise ValueError(f"MelSpectrogramError: windows must hold 1 to 8 filter lengths, got {len(windows)}")
        win_lengths = windows if win_lengths is None else [int(w) for w in win_lengths]
        if len(win_lengths) != len(windows):
            raise ValueError(f"MelSpectrogramError: win_lengths has {len(win_lengths)} entries for {len(windows)} windows")
        if framing not in FRAMINGS:
            raise ValueError(f"MelSpectrogramError: framing must be one of {sorted(FRAMINGS)}, got {framing!r}")
        for n, wl in zip(windows, win_lengths):
            if n % 16 or not 32 <= n <= 4096:
                raise ValueError(f"MelSpectrogramError: filter_length {n} must be a multiple of 16 in [32, 4096]")
            if not 1 <= wl <= n:
                raise ValueError(f"MelSpectrogramError: win_length {wl} must lie in [1, {n}]")
            if not 1 <= int(hop_length) <= n:
                raise ValueError(f"MelSpectrogramError: hop_length {hop_length} must lie in [1, {n}]")
        if not 1 <= int(n_mel_channels) <= 256:
            raise ValueError(f"MelSpectrogramError: n_mel_channels {n_mel_channels} must lie in [1, 256]")
        self.windows, self.win_lengths, self.hop_length = tuple(windows), tuple(win_lengths), int(hop_length)
        self.sampling_rate, self.n_mel_channels, self.framing = sampling_rate, int(n_mel_channels), framing
        self.clamp_val = float(clamp_val)
        self.mag_eps = 1e-9 if framing == "nv" else 0.0
        self.pads = tuple(int((n - self.hop_length) / 2) if framing == "nv" else n // 2 for n in windows)
        for i, (n, wl) in enumerate(zip(windows, win_lengths)):
            self.register_buffer(f"forward_basis_{i}", STFT(n, self.hop_length, wl).forward_basis.squeeze(1).contiguous(),
                                 persistent=False)
            fb = slaney_mel_filterbank(sampling_rate, n, self.n_mel_channels, mel_fmin, mel_fmax)
            self.register_buffer(f"mel_basis_{i}", torch.from_numpy(fb).float(), persistent=False)
        self._packed, self._ws = {}, {}

    def _apply(self, fn, *a, **kw):
        self._packed, self._ws = {}, {}
        return super()._apply(fn, *a, **kw)

    # ---------------------------------------------------------------------------------------------- arguments ----
    def _config(self):
        cfg = _lib.MelErrorConfig(n_windows=len(self.windows), hop_length=self.hop_length, n_mel_channels=self.n_mel_channels,
                                  framing=FRAMINGS[self.framing], clamp_val=self.clamp_val, mag_eps=self.mag_eps)
        for i, n in enumerate(self.windows):
            cfg.filter_lengths[i] = n
        return cfg

    def frames(self, samples, window=0):
        """Frames of a signal of ``samples`` under this object's framing at window ``window``."""
        n, pad = self.windows[window], self.pads[window]
        if self.framing == "nv":
            return (samples + 2 * pad - n) // self.hop_length + 1 if samples + 2 * pad >= n else 0
        return samples // self.hop_length + 1

    @staticmethod
    def _lengths(x, name, B, width):
        """-> (int32 tensor [B], host list or None).  ``None`` means the full width.  Lengths given as a list or a host tensor are
        checked by the caller (no synchronisation needed).  A DEVICE tensor is taken as it is, without a synchronisation - unlike the
        reference, which knows every length on the host: the library then scores ``min(gt frames, pred frames)`` frames of an item,
        reads a length outside ``[1, width]`` as the nearest bound, folds reflect indices into ``[0, length)``, and never reads outside
        an item's row; a length at or below the reflect pad is then folded more than once instead of being refused."""
        if x is None:
            return None, [width] * B
        x = torch.as_tensor(x)
        if x.numel() != B:
            raise ValueError(f"MelSpectrogramError: {name} has {x.numel()} entries for a batch of {B}")
        x = x.detach().reshape(B)
        return x, (None if x.is_cuda else [int(v) for v in x.tolist()])

    def _check_host_lengths(self, pl, gl, T_pred, T_gt, gt_is_mel, mel_frames):
        pad = max(self.pads)
        for name, host, width in (("pred_lengths", pl, T_pred),) + ((("gt_lengths", gl, T_gt),) if not gt_is_mel else ()):
            if host is None:
                continue
            for b, v in enumerate(host):
                if v > width:
                    raise ValueError(f"MelSpectrogramError: {name}[{b}] = {v} exceeds the tensor width {width}")
                if v <= pad:
                    raise ValueError(f"MelSpectrogramError: {name}[{b}] = {v} must exceed the reflect pad {pad}")
        if gt_is_mel and gl is not None:
            for b, v in enumerate(gl):
                if not 1 <= v <= mel_frames:
                    raise ValueError(f"MelSpectrogramError: gt_lengths[{b}] = {v} frames must lie in [1, {mel_frames}] (the width of gt_mel)")
        if pl is None or gl is None:
            return
        for w in range(len(self.windows)):
            for b in range(len(pl)):
                gf = gl[b] if gt_is_mel else self.frames(gl[b], w)
                pf = self.frames(pl[b], w)
                if pf < gf:
                    raise ValueError(f"MelSpectrogramError: pred_lengths[{b}] = {pl[b]} gives {pf} frames at window {self.windows[w]}, fewer than "
                                     f"the ground truth's {gf} (train.py:268 crops the generated mel to the ground truth, never the reverse)")

    def _inputs(self, pred_audio, gt_audio, gt_mel, pred_lengths, gt_lengths):
        if (gt_audio is None) == (gt_mel is None):
            raise ValueError("MelSpectrogramError: exactly one of gt_audio and gt_mel must be given")
        if gt_mel is not None and len(self.windows) > 1:
            raise ValueError(f"MelSpectrogramError: gt_mel is a single-window input, this object has {len(self.windows)} windows")
        named = {"pred_audio": pred_audio, ("gt_audio" if gt_mel is None else "gt_mel"): gt_audio if gt_mel is None else gt_mel}
        for k, v in named.items():
            if not torch.is_tensor(v):
                raise ValueError(f"MelSpectrogramError: {k} is not a tensor ({type(v).__name__})")
            if v.requires_grad and torch.is_grad_enabled():
                raise NotImplementedError(f"MelSpectrogramError on the HIP path has no backward pass: {k} requires grad (a validation "
                                          "score needs none; call under torch.no_grad() or detach)")
        squeeze = lambda v: v.squeeze(1) if v.dim() == 3 and v.shape[1] == 1 else v
        pred_audio = squeeze(pred_audio)
        if pred_audio.dim() != 2 or min(pred_audio.shape) < 1:
            raise ValueError(f"MelSpectrogramError: pred_audio must be [B, T], got {tuple(pred_audio.shape)}")
        B, T_pred = pred_audio.shape
        T_gt = mel_frames = 0
        if gt_mel is None:
            gt_audio = squeeze(gt_audio)
            if gt_audio.dim() != 2 or gt_audio.shape[0] != B or gt_audio.shape[1] < 1:
                raise ValueError(f"MelSpectrogramError: gt_audio must be [B, T] = [{B}, T], got {tuple(gt_audio.shape)}")
            T_gt = gt_audio.shape[1]
        else:
            if gt_mel.dim() != 3 or tuple(gt_mel.shape[:2]) != (B, self.n_mel_channels) or gt_mel.shape[2] < 1:
                raise ValueError(f"MelSpectrogramError: gt_mel must be [B, n_mel, frames] = [{B}, {self.n_mel_channels}, frames], got "
                                 f"{tuple(gt_mel.shape)}")
            mel_frames = gt_mel.shape[2]
        pl_t, pl = self._lengths(pred_lengths, "pred_lengths", B, T_pred)
        gl_t, gl = self._lengths(gt_lengths, "gt_lengths", B, mel_frames if gt_mel is not None else T_gt)
        self._check_host_lengths(pl, gl, T_pred, T_gt, gt_mel is not None, mel_frames)
        for k, v in named.items():
            if not v.is_cuda:
                raise _lib.HipLibraryError(f"MelSpectrogramError: {k}: expected a CUDA/HIP tensor (this path has no CPU fallback)")
        dev = pred_audio.device
        f32 = lambda v: v.detach().to(device=dev, dtype=torch.float32).contiguous()
        i32 = lambda t, host: (torch.tensor(host, dtype=torch.int32, device=dev) if t is None or not t.is_cuda
                               else t.to(device=dev, dtype=torch.int32).contiguous())
        t = {"pred": f32(pred_audio), "gt": None if gt_mel is not None else f32(gt_audio),
             "gt_mel": None if gt_mel is None else f32(gt_mel), "pred_lengths": i32(pl_t, pl), "gt_lengths": i32(gl_t, gl)}
        return t, (B, T_pred, T_gt, mel_frames), dev

    def _blob(self, dev, cfg):
        if dev not in self._packed:
            lib = _lib.lib()
            n = _lib.nbytes(lib.ctts_mel_error_packed_bytes, C.byref(cfg), what="unsupported MelSpectrogramError config")
            blob = torch.empty(n // 4, dtype=torch.float32, device=dev)
            stream = _lib.stream(dev)
            for i in range(len(self.windows)):
                fb = getattr(self, f"forward_basis_{i}").detach().float().contiguous().to(dev)
                mb = getattr(self, f"mel_basis_{i}").detach().float().contiguous().to(dev)
                _lib.check(lib.ctts_mel_error_pack(C.byref(cfg), i, _lib.ptr(fb), _lib.ptr(mb), _lib.ptr(blob), stream),
                           "ctts_mel_error_pack")
            torch.cuda.current_stream(dev).synchronize()          # fb / mb may be freed once this returns (pack time only)
            self._packed[dev] = blob
        return self._packed[dev]

    def _workspace(self, dev, cfg, B, T_pred, T_gt):
        key = (dev, B, T_pred, T_gt)
        ws = self._ws.pop(key, None)
        if ws is None:
            n = _lib.nbytes(_lib.lib().ctts_mel_error_workspace_bytes, C.byref(cfg), B, T_pred, T_gt,
                            what="ctts_mel_error_workspace_bytes")
            ws = torch.empty(n, dtype=torch.uint8, device=dev)
            while len(self._ws) >= 2:                              # the two most recent geometries are kept
                self._ws.pop(next(iter(self._ws)))
        self._ws[key] = ws
        return ws

    # ---------------------------------------------------------------------------------------------- the calls ----
    def _run(self, pred_audio, gt_audio, gt_mel, pred_lengths, gt_lengths, sanitize, return_maps):
        t, (B, T_pred, T_gt, mel_frames), dev = self._inputs(pred_audio, gt_audio, gt_mel, pred_lengths, gt_lengths)
        W = len(self.windows)
        cfg = self._config()
        with torch.cuda.device(dev):
            blob = self._blob(dev, cfg)
            ws = self._workspace(dev, cfg, B, T_pred, T_gt)
            table = torch.empty(B * W * len(COLUMNS) + len(TERMS), dtype=torch.float64, device=dev)
            maps, map_frames = None, 0
            if return_maps:
                cap = lambda w: min(self.frames(T_pred, w), mel_frames if gt_mel is not None else self.frames(T_gt, w))
                map_frames = max(cap(w) for w in range(W))
                maps = {k: torch.zeros(B, W, self.n_mel_channels, map_frames, dtype=torch.float32, device=dev)
                        for k in ("mae_spec", "pred_mel", "gt_mel")}
            m = [None if maps is None else _lib.ptr(maps[k]) for k in ("mae_spec", "pred_mel", "gt_mel")]
            _lib.check(_lib.lib().ctts_mel_error_f32(
                C.byref(cfg), _lib.ptr(blob), _lib.ptr(t["pred"]), _lib.ptr(t["pred_lengths"]), _lib.ptr(t["gt"]),
                _lib.ptr(t["gt_lengths"]), _lib.ptr(t["gt_mel"]), 1 if sanitize else 0, B, T_pred, T_gt, mel_frames, _lib.ptr(table),
                *m, map_frames, _lib.ptr(ws), ws.numel(), _lib.stream(dev)), "ctts_mel_error_f32")
        return table, maps, (B, W)

    def per_item(self, pred_audio, gt_audio=None, *, gt_mel=None, pred_lengths=None, gt_lengths=None, sanitize=True,
                 return_maps=False):
        """-> float64 device table ``[B, W, 5]`` in the order of ``COLUMNS`` (with ``return_maps=True``: ``(table, maps)``), without
        any host synchronisation.  ``pred_audio`` ``[B, T]``: the generated audio; ``gt_audio`` ``[B, T']`` or ``gt_mel``
        ``[B, n_mel, frames]`` (one window: an already-computed log-mel, as HiFi-GAN's loader supplies ``y_mel``); ``pred_lengths`` /
        ``gt_lengths``: samples per item (``gt_lengths`` counts frames of ``gt_mel`` in that form), default the full width.
        ``n_frames`` of an item is the ground truth's frame count (train.py:268 crops the generated mel to it).  ``sanitize=True``
        reads the generated audio as train.py:259-260 leave it: clamped to +-0.999 (which also maps +-inf), then NaN -> 0."""
        table, maps, (B, W) = self._run(pred_audio, gt_audio, gt_mel, pred_lengths, gt_lengths, sanitize, return_maps)
        rows = table[:B * W * len(COLUMNS)].view(B, W, len(COLUMNS))
        return (rows, maps) if return_maps else rows

    def forward(self, pred_audio, gt_audio=None, *, gt_mel=None, pred_lengths=None, gt_lengths=None, sanitize=True,
                return_maps=False):   # no torch.no_grad() here: the refusal of grad-carrying inputs must see the caller's mode
        """The arguments of :meth:`per_item` -> dict from ONE device-to-host copy: ``average_MSE`` / ``average_MAE`` (Python floats:
        ``total_MSE / total`` of train.py:271-278, 294-295 - the mean over (file, window) pairs of the pair means, file-major and
        window-minor), ``l1`` (a list per window of ``sum(SAE) / sum(count)``: ``F.l1_loss`` on an equal-length batch,
        hifigan/train.py:208-210), ``table`` (the ``[B, W, 5]`` host tensor) and, with ``return_maps=True``, the DEVICE tensors
        ``mae_spec``, ``pred_mel``, ``gt_mel`` ``[B, W, n_mel, frames_max]``, zero past each item's frames (what train.py:299-314
        plots)."""
        table, maps, (B, W) = self._run(pred_audio, gt_audio, gt_mel, pred_lengths, gt_lengths, sanitize, return_maps)
        host = table.cpu()                                                   # the one host read
        n = B * W * len(COLUMNS)
        out = {"average_MSE": float(host[n]), "average_MAE": float(host[n + 1]), "l1": [float(host[n + 2 + w]) for w in range(W)],
               "table": host[:n].view(B, W, len(COLUMNS))}
        if maps is not None:
            out.update(maps)
        return out
