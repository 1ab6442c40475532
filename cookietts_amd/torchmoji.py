"""torchMoji feature encoder on the HIP path: the T2S server's default style input (``style_mode == 'torchmoji_hidden'``).

Host mirror of ``utils/torchmoji/model_def.py:100-253`` with ``feature_output=True`` over ``ctts_torchmoji_*``
(``include/cookietts_hip.h``, "torchMoji feature encoder"; sources in ``csrc/torchmoji.hip`` and the hard-sigmoid form of the
packed-sequence LSTM in ``csrc/tacotron_decoder.hip``).  The module tree holds the reference's parameters under the reference's
state-dict keys and is never on the inference path; all arithmetic is in the library.  The sentence tokenizer and the
vocabulary stay the reference's.

Differences from the reference, all deliberate:

* the features come back as a **device** tensor (the reference returns numpy for numpy input; ``return_numpy=True`` does that);
* attention weights (``return_attention=True``) are in **input order**.  The reference sorts the batch by length for packing,
  un-sorts the features and returns the attention still sorted (model_def.py:194-195, 241-251);
* a row without any token raises ``ValueError`` on the host path (the reference fails there with an empty ``max``) and gives a
  zero feature row on the device path, where nothing is read back;
* the softmax of the pooling subtracts each row's own maximum, not the padded batch's (the same quotient up to rounding).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _cache, _lib

NB_TOKENS = 50000          # utils/torchmoji/global_variables.py
MAX_GROUP = 256            # rows per library call (the batched form of the packed-sequence LSTM)


class Attention(nn.Module):
    """attlayer.py:19-32: parameter holder of ``attention_vector``."""

    def __init__(self, attention_size):
        super().__init__()
        self.attention_vector = nn.Parameter(torch.empty(attention_size).normal_(std=0.05))


class TorchMoji(_cache.PackedModule):
    GPU_ONLY = "TorchMoji HIP path needs the model on a GPU (no CPU fallback)"

    def __init__(self, nb_tokens=NB_TOKENS, feature_output=True, return_attention=False, nb_classes=None, embedding_dim=256,
                 hidden_size=512):
        super().__init__()
        if not feature_output or nb_classes is not None:
            raise NotImplementedError("cookietts_amd.TorchMoji: only the feature encoder is built (feature_output=True, "
                                      "nb_classes=None); the classifier head is not")
        self.nb_tokens, self.embedding_dim, self.hidden_size = int(nb_tokens), int(embedding_dim), int(hidden_size)
        self.attention_size = 4 * self.hidden_size + self.embedding_dim
        self.return_attention = bool(return_attention)
        self._cfg = _lib.TorchMojiConfig(self.nb_tokens, self.embedding_dim, self.hidden_size)
        self.embed = nn.Embedding(self.nb_tokens, self.embedding_dim)
        self.lstm_0 = nn.LSTM(self.embedding_dim, self.hidden_size, batch_first=True, bidirectional=True)
        self.lstm_1 = nn.LSTM(2 * self.hidden_size, self.hidden_size, batch_first=True, bidirectional=True)
        self.attention_layer = Attention(self.attention_size)
        super().train(False)           # as the reference: evaluation mode from the start (model_def.py:150)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("cookietts_amd.TorchMoji is inference-only: train() mode is not built")
        return super().train(False)

    # ------------------------------------------------------------------ packing ----
    def _pack(self, device):
        lib = _lib.lib()
        keep = []
        w = _lib.TorchMojiWeights()
        with torch.cuda.device(device):
            w.embed = _cache.dev(self.embed.weight.to(device), keep)
            w.attention_vector = _cache.dev(self.attention_layer.attention_vector.to(device), keep)
            for layer, lstm in enumerate((self.lstm_0, self.lstm_1)):
                for k, sfx in enumerate(("", "_reverse")):
                    for field, name in (("w_ih", "weight_ih"), ("w_hh", "weight_hh"), ("b_ih", "bias_ih"), ("b_hh", "bias_hh")):
                        setattr(w.lstm[layer][k], field, _cache.dev(getattr(lstm, name + "_l0" + sfx).to(device), keep))
            nbytes = _lib.nbytes(lib.ctts_torchmoji_packed_bytes, C.byref(self._cfg), what="cookietts_amd.TorchMoji: unsupported shape")
            blob = torch.zeros(nbytes // 4, dtype=torch.float32, device=device)
            _lib.check(lib.ctts_torchmoji_pack_f32(C.byref(self._cfg), C.byref(w), _lib.ptr(blob), _lib.stream(device)),
                       "ctts_torchmoji_pack_f32")
            torch.cuda.current_stream(device).synchronize()     # `keep` dies with this frame
        return blob

    # ------------------------------------------------------------------ forward ----
    def _host_tokens(self, tokens):
        """Host path: lengths, the trim to the longest length and the range check, before any launch."""
        tok = tokens.numpy() if isinstance(tokens, torch.Tensor) else np.asarray(tokens)
        if tok.ndim != 2 or tok.dtype.kind not in "iu":
            raise ValueError(f"tokens must be an integer array [B, T], got {tok.dtype} {tuple(tok.shape)}")
        tok = tok.astype(np.int64)
        if tok.shape[0] < 1 or tok.shape[1] < 1:
            raise ValueError(f"tokens must be [B, T] with B, T >= 1, got {tuple(tok.shape)}")
        nz = tok != 0
        empty = np.flatnonzero(~nz.any(axis=1))
        if empty.size:
            raise ValueError(f"row {int(empty[0])} of the token batch has no token (all zeros)")
        if tok.min() < 0 or tok.max() >= self.nb_tokens:
            raise IndexError(f"token index out of range: [{int(tok.min())}, {int(tok.max())}] with nb_tokens={self.nb_tokens}")
        T = tok.shape[1]
        lengths = (T - np.argmax(nz[:, ::-1], axis=1)).astype(np.int32)
        return np.ascontiguousarray(tok[:, :int(lengths.max())]), lengths

    @torch.no_grad()
    def forward(self, tokens, return_numpy=False):
        """tokens [B, T]: a numpy array of any integer dtype or a CPU tensor (lengths, trim and range check on the host), or a
        device tensor (lengths from ``ctts_torchmoji_lengths``, every column's steps issued, nothing read back).
        Returns the features, a device fp32 tensor [B, 4 * hidden + embedding] in input order - with ``return_attention`` also
        the attention weights [B, T_used] in input order - or numpy copies of them with ``return_numpy=True``."""
        if self.training:
            raise NotImplementedError("cookietts_amd.TorchMoji is inference-only: call .eval()")
        on_device = isinstance(tokens, torch.Tensor) and tokens.is_cuda
        if on_device:
            if tokens.dim() != 2 or tokens.dtype.is_floating_point or tokens.shape[0] < 1 or tokens.shape[1] < 1:
                raise ValueError(f"tokens must be an integer tensor [B, T], got {tokens.dtype} {tuple(tokens.shape)}")
            device = tokens.device
            blob = self.packed(device, lambda: self._pack(device))
            tok = tokens.detach().to(torch.int64).contiguous()
            lens = None
        else:
            tok_np, lens_np = self._host_tokens(tokens)
            device = self.embed.weight.device
            blob = self.packed(device, lambda: self._pack(device))       # raises for a model on the CPU
            tok = torch.from_numpy(tok_np).to(device)
            lens = torch.from_numpy(lens_np).to(device)
        lib = _lib.lib()
        B, T = tok.shape
        F = self.attention_size
        with torch.cuda.device(device):
            st = _lib.stream(device)
            if lens is None:
                lens = torch.empty(B, dtype=torch.int32, device=device)
                _lib.check(lib.ctts_torchmoji_lengths(_lib.ptr(tok), _lib.ptr(lens), B, T, st), "ctts_torchmoji_lengths")
            feats = torch.empty(B, F, dtype=torch.float32, device=device)
            att = torch.empty(B, T, dtype=torch.float32, device=device) if self.return_attention else None
            for g0 in range(0, B, MAX_GROUP):
                g1 = min(g0 + MAX_GROUP, B)
                nb = g1 - g0
                ws = self.workspace((device, nb, T), lambda: _lib.nbytes(lib.ctts_torchmoji_workspace_bytes, C.byref(self._cfg), nb, T,
                                                                         what="ctts_torchmoji_workspace_bytes"), zero=False)
                _lib.check(lib.ctts_torchmoji_features_f32(
                    C.byref(self._cfg), _lib.ptr(blob), _lib.ptr(tok[g0:g1]), _lib.ptr(lens[g0:g1]), _lib.ptr(feats[g0:g1]),
                    _lib.ptr(att[g0:g1]) if att is not None else None, nb, T, _lib.ptr(ws), ws.numel() * 4, st),
                    "ctts_torchmoji_features_f32")
        if return_numpy:
            feats = feats.cpu().numpy()
            att = att.cpu().numpy() if att is not None else None
        return (feats, att) if self.return_attention else feats


def torchmoji_feature_encoding(weight_path, return_attention=False):
    """``model_def.torchmoji_feature_encoding`` (model_def.py:19-38): the pretrained ``pytorch_model.bin`` state dict into a
    ``TorchMoji(nb_tokens=50000)``, read with ``weights_only=True``.  ``output_layer.*`` is skipped, as
    ``load_specific_weights(exclude_names=['output_layer'])`` does; any other missing or unexpected key raises.  The model
    comes back on the CPU, in eval mode: move it with ``.cuda()``."""
    model = TorchMoji(nb_tokens=NB_TOKENS, return_attention=return_attention)
    sd = torch.load(weight_path, map_location='cpu', weights_only=True)
    sd = {k: v for k, v in sd.items() if not k.startswith('output_layer')}
    model.load_state_dict(sd, strict=True)
    return model
