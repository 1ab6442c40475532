"""HiFi-GAN generator on the HIP path: the vocoder the reference's server loads
(``_5_infer/t2s_server/text2speech.py:175-179, 258-263`` -> ``_4_mtw/hifigan/models.py:14-31, 94-148``).

``Generator(h)`` has the reference's module tree and state-dict keys (``conv_pre.*``, ``ups.i.*``,
``resblocks.n.convs1.m.*`` / ``convs2.m.*`` (ResBlock1) or ``convs.m.*`` (ResBlock2), ``conv_post.*``; each ``bias``,
``weight_g``, ``weight_v``), ``remove_weight_norm()`` and ``forward(mel [B, num_mels, T]) -> [B, 1, T * prod(upsample_rates)]``.
The whole forward is ``ctts_hifigan_forward_f32`` (csrc/hifigan.hip): one fp32 MFMA launch per conv, LeakyReLU / residual
adds / the resblock mean / tanh inside those launches.  There is no CPU fallback: a CPU tensor raises.

``.half()`` (text2speech.py:262): the parameters become fp16 - so ``next(vocoder.parameters()).dtype`` and the server's
``mel.to(dtype)`` work unchanged - the products stay fp32 MFMA on the fp16-rounded weights, and the waveform comes back in the
dtype of the mel it was given.  Options the kernels cannot run exactly raise ``NotImplementedError`` at construction.

``set_compute_dtype(torch.float16)`` selects the IEEE-half storage mode (``ctts_hifigan_forward_f16``, csrc/hifigan_f16.hip):
weights and every stored activation in half, products on the f16 MFMA, fp32 accumulation.  It is independent of the parameter
dtype; what the reference's server gets from ``vocoder.half()`` is ``vocoder.half().set_compute_dtype(torch.float16)`` here.

``set_f32_gemm_mode("bf16x3")`` keeps the fp32 tensors and runs every product as split bf16 (``ctts_hifigan_forward_bf16x3``,
csrc/hifigan_bf16x3.hip): hi + lo bf16 operands, three bf16 MFMA products per operand pair, fp32 accumulation.
"""
from __future__ import annotations

import ctypes as C
import json
import os

import torch
import torch.nn as nn

from . import _cache, _lib
from ._wn import WNConv

__all__ = ["Generator", "load_model", "AttrDict"]


class AttrDict(dict):
    """``config.json`` with attribute access, as the reference's loader hands it back (hifigan/env.py)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.__dict__ = self


def _get(h, name):
    return h[name] if isinstance(h, dict) else getattr(h, name)


def check_config(h):
    """Raise ``NotImplementedError`` naming the option for what the HIP generator does not run exactly."""
    def refuse(what):
        raise NotImplementedError(f"cookietts_amd.HiFiGANGenerator: {what} is not built on the HIP path")
    resblock = str(_get(h, "resblock"))
    if resblock not in ("1", "2"):
        refuse(f"resblock={resblock!r} ('1' or '2')")
    rates, ksz = list(_get(h, "upsample_rates")), list(_get(h, "upsample_kernel_sizes"))
    rk, rd = list(_get(h, "resblock_kernel_sizes")), [list(d) for d in _get(h, "resblock_dilation_sizes")]
    if not 1 <= len(rates) <= _lib.HifiganConfig.MAX_UPS or len(ksz) != len(rates):
        refuse(f"upsample_rates with {len(rates)} stages / upsample_kernel_sizes with {len(ksz)} (1..{_lib.HifiganConfig.MAX_UPS}, equal)")
    if not 1 <= len(rk) <= _lib.HifiganConfig.MAX_KERNELS or len(rd) != len(rk):
        refuse(f"resblock_kernel_sizes with {len(rk)} entries / resblock_dilation_sizes with {len(rd)} "
               f"(1..{_lib.HifiganConfig.MAX_KERNELS}, equal)")
    need = 3 if resblock == "1" else 2
    for j, (k, d) in enumerate(zip(rk, rd)):
        if k % 2 == 0:
            refuse(f"resblock_kernel_sizes[{j}]={k} (even: the reference's padding does not keep the length)")
        if len(d) < need or len(d) > _lib.HifiganConfig.MAX_DILATIONS:
            refuse(f"resblock_dilation_sizes[{j}]={d} (ResBlock{resblock} reads {need})")
    for i, (u, k) in enumerate(zip(rates, ksz)):
        if k < u or (k - u) % 2:
            refuse(f"upsample_kernel_sizes[{i}]={k} with rate {u} (kernel - rate odd: the output is not rate * T long)")


def c_config(h):
    resblock = str(_get(h, "resblock"))
    rates, ksz = list(_get(h, "upsample_rates")), list(_get(h, "upsample_kernel_sizes"))
    rk, rd = list(_get(h, "resblock_kernel_sizes")), [list(d) for d in _get(h, "resblock_dilation_sizes")]
    cfg = _lib.HifiganConfig(num_mels=int(_get(h, "num_mels")), upsample_initial_channel=int(_get(h, "upsample_initial_channel")),
                             resblock=int(resblock) if resblock.isdigit() else 0,
                             n_ups=len(rates), n_kernels=len(rk))
    for i in range(min(len(rates), cfg.MAX_UPS)):
        cfg.upsample_rates[i] = int(rates[i])
        cfg.upsample_kernel_sizes[i] = int(ksz[i]) if i < len(ksz) else 0
    for j in range(min(len(rk), cfg.MAX_KERNELS)):
        cfg.resblock_kernel_sizes[j] = int(rk[j])
        for m in range(min(len(rd[j]) if j < len(rd) else 0, cfg.MAX_DILATIONS)):
            cfg.resblock_dilation_sizes[j][m] = int(rd[j][m])
    return cfg


# library entry points of the three arithmetic paths: packed-size query, pack, workspace-size query, forward
_ENTRY = {
    "f32": ("ctts_hifigan_packed_bytes", "ctts_hifigan_pack_f32", "ctts_hifigan_workspace_bytes", "ctts_hifigan_forward_f32"),
    "f16": ("ctts_hifigan_packed_f16_bytes", "ctts_hifigan_pack_f16", "ctts_hifigan_workspace_f16_bytes", "ctts_hifigan_forward_f16"),
    "bf16x3": ("ctts_hifigan_packed_bf16x3_bytes", "ctts_hifigan_pack_bf16x3", "ctts_hifigan_workspace_bf16x3_bytes",
               "ctts_hifigan_forward_bf16x3"),
}


class _ResBlock(nn.Module):
    """Parameter tree of ResBlock1 (models.py:35-73: ``convs1`` / ``convs2``) or ResBlock2 (:75-92: ``convs``)."""

    def __init__(self, kind, channels, kernel_size):
        super().__init__()
        def convs(n):
            return nn.ModuleList([WNConv((channels, channels, kernel_size)) for _ in range(n)])
        if kind == "1":
            self.convs1, self.convs2 = convs(3), convs(3)
        else:
            self.convs = convs(2)

    def conv_list(self):
        return list(self.convs1) + list(self.convs2) if hasattr(self, "convs1") else list(self.convs)


class Generator(_cache.PackedModule):
    """``hifigan.models.Generator`` (models.py:94-148) over ``ctts_hifigan_forward_f32``."""
    GPU_ONLY = "HiFi-GAN HIP path needs the model on a GPU (no CPU fallback)"

    def __init__(self, h):
        super().__init__()
        check_config(h)
        self.h = h
        rates, ksz = list(_get(h, "upsample_rates")), list(_get(h, "upsample_kernel_sizes"))
        rk = list(_get(h, "resblock_kernel_sizes"))
        C0 = int(_get(h, "upsample_initial_channel"))
        self.num_kernels, self.num_upsamples = len(rk), len(rates)
        self.upsample_factor = 1
        for u in rates:
            self.upsample_factor *= int(u)
        self.conv_pre = WNConv((C0, int(_get(h, "num_mels")), 7))
        # ConvTranspose1d weight: [C_in, C_out, k]; weight norm's dim 0 is the INPUT channel there
        self.ups = nn.ModuleList([WNConv((C0 // 2 ** i, C0 // 2 ** (i + 1), k)) for i, k in enumerate(ksz)])
        for i, up in enumerate(self.ups):
            up.bias = nn.Parameter(torch.zeros(C0 // 2 ** (i + 1)))
        self.resblocks = nn.ModuleList()
        ch = C0
        for i in range(len(rates)):
            ch = C0 // 2 ** (i + 1)
            for k in rk:
                self.resblocks.append(_ResBlock(str(_get(h, "resblock")), ch, k))
        self.conv_post = WNConv((1, ch, 7))
        self._cfg = c_config(h)
        lib = _lib.lib()
        if lib.ctts_hifigan_packed_bytes(C.byref(self._cfg)) == 0:
            raise NotImplementedError("cookietts_amd.HiFiGANGenerator: refused by the library: " + _lib.last_error())
        self._compute_dtype = torch.float32
        self._f32_gemm_mode = None

    # ------------------------------------------------------------------ plumbing ----
    def _path(self):
        """Key into ``_ENTRY`` of the arithmetic the next call runs: ``"f16"``, ``"bf16x3"`` or ``"f32"``."""
        if self._compute_dtype == torch.float16:
            return "f16"
        return "bf16x3" if _lib.model_gemm_mode(self._f32_gemm_mode) == _lib.MODEL_GEMM_MODES["bf16x3"] else "f32"

    def set_f32_gemm_mode(self, mode):
        """Products of the fp32 tensors, same name and meaning as on the WaveGlow classes: ``None`` / ``"default"`` / ``"f32"``
        (exact fp32 MFMA) or ``"bf16x3"``: split bf16 - activations stay fp32 in the fp32 path's layout and workspace, weights
        (once, at pack time) and staged activations are carried as ``hi + lo`` bf16, and every product is ``w_hi x_hi + w_lo x_hi +
        w_hi x_lo`` on the bf16 MFMA with fp32 accumulation (16 mantissa bits per operand; the arithmetic is listed at
        ``ctts_hifigan_forward_bf16x3``).  ``"bf16x6"`` is not built for this model (``NotImplementedError``); an unknown name
        is a ``ValueError``.

        The mode acts while the compute dtype is ``torch.float32``.  Under ``set_compute_dtype(torch.float16)`` the f16 path
        runs; the mode is remembered but inert, and acts again once the compute dtype is back at ``torch.float32``.  ``.half()``
        keeps its meaning: fp16 parameters, then the selected products.  Returns ``self``; the packed blob and the workspaces
        are dropped when the selected products change and kept when they do not.  ``NotImplementedError`` - here, not at the
        first call - if the library refuses the config."""
        code = _lib.model_gemm_mode(mode)
        if code == _lib.MODEL_GEMM_MODES["bf16x6"]:
            raise NotImplementedError("cookietts_amd.HiFiGANGenerator: f32 GEMM mode 'bf16x6' is not built for this model "
                                      "('f32' or 'bf16x3')")
        if code == _lib.MODEL_GEMM_MODES["bf16x3"]:
            if _lib.lib().ctts_hifigan_packed_bf16x3_bytes(C.byref(self._cfg)) == 0:
                raise NotImplementedError("cookietts_amd.HiFiGANGenerator: split-bf16 products refused by the library: "
                                          + _lib.last_error())
        before = self._path()
        self._f32_gemm_mode = mode
        if self._path() != before:
            self._invalidate()        # the packed blob is per format
        return self

    @property
    def f32_gemm_mode(self):
        return self._f32_gemm_mode

    def set_compute_dtype(self, dtype):
        """Storage and product format of the whole generator: ``torch.float32`` (default: fp32 tensors, exact fp32 MFMA) or
        ``torch.float16``: weights and every stored activation as IEEE half, products on the f16 matrix pipe, accumulation,
        bias, residual add, resblock mean and tanh in fp32, one rounding per stored value (the rounding points are listed at
        ``ctts_hifigan_forward_f16``).  Independent of the parameter dtype (``.half()`` alone keeps fp32 products); switching
        back to ``torch.float32`` restores the fp32 path bit for bit.  Returns ``self``; the packed blob and the workspaces are
        dropped when the mode changes and kept when it does not.  ``NotImplementedError`` - here, not at the first call - if
        the library refuses the config in half storage."""
        if dtype not in (torch.float32, torch.float16):
            raise ValueError(f"compute dtype must be torch.float32 or torch.float16, not {dtype!r}")
        if dtype == torch.float16:
            lib = _lib.lib()
            if lib.ctts_hifigan_packed_f16_bytes(C.byref(self._cfg)) == 0:
                raise NotImplementedError("cookietts_amd.HiFiGANGenerator: half storage refused by the library: "
                                          + _lib.last_error())
        if dtype != self._compute_dtype:
            self._compute_dtype = dtype
            self._invalidate()        # the packed blob and the workspaces are per format
        return self

    @property
    def compute_dtype(self):
        return self._compute_dtype

    def remove_weight_norm(self):
        for m in self.modules():
            if isinstance(m, WNConv):
                m.remove_weight_norm()
        self._invalidate()

    def _convs(self):
        """Every conv in the order of the library's flat weight buffer (ctts_hifigan_weight_floats)."""
        out = [self.conv_pre]
        for i in range(self.num_upsamples):
            out.append(self.ups[i])
            for j in range(self.num_kernels):
                out += self.resblocks[i * self.num_kernels + j].conv_list()
        return out + [self.conv_post]

    def folded_weights(self):
        """[(weight, bias)] fp32 in ``_convs`` order: ``w = g * v / ||v||`` evaluated in fp32 on the stored parameters
        (after ``.half()``: on the fp16-rounded ones).  Deliberately NOT ``_wn.folded_weight``: that one folds on the device
        through ``ctts_fold_weightnorm_f32``, this one in torch, and the two need not round alike - the packed bits would move."""
        out = []
        for m in self._convs():
            if getattr(m, "weight_v", None) is not None:
                v, g = m.weight_v.detach().float(), m.weight_g.detach().float()
                w = v * (g / v.flatten(1).norm(dim=1).view(g.shape))
            else:
                w = m.weight.detach().float()
            out.append((w, m.bias.detach().float()))
        return out

    def _ensure_packed(self, device):
        return self.packed(device, lambda: self._pack(device))

    def _pack(self, device):
        lib = _lib.lib()
        with torch.cuda.device(device):
            flat = torch.cat([t.reshape(-1) for wb in self.folded_weights() for t in wb]).to(device).contiguous()
            n = lib.ctts_hifigan_weight_floats(C.byref(self._cfg))
            packed_bytes, name, _, _ = _ENTRY[self._path()]
            nbytes = getattr(lib, packed_bytes)(C.byref(self._cfg))
            blob = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
            stream = _lib.stream(device)
            if flat.numel() != n:
                raise _lib.HipLibraryError(f"HiFi-GAN: {flat.numel()} weights in the module tree, the library expects {n}")
            _lib.check(getattr(lib, name)(C.byref(self._cfg), _lib.ptr(flat), flat.numel(), _lib.ptr(blob), stream), name)
            torch.cuda.current_stream(device).synchronize()     # `flat` dies with this frame
        return blob

    # ------------------------------------------------------------------ forward ----
    def forward(self, x):
        if x.dim() != 3 or x.shape[1] != self._cfg.num_mels:
            raise ValueError(f"mel must be [B, {self._cfg.num_mels}, T], got {tuple(x.shape)}")
        if not x.is_cuda:
            raise _lib.HipLibraryError("HiFi-GAN HIP path needs the mel on a GPU (no CPU fallback)")
        device = x.device
        blob = self._ensure_packed(device)
        lib = _lib.lib()
        B, _, T = x.shape
        _, _, ws_query, fwd = _ENTRY[self._path()]
        ws_bytes = getattr(lib, ws_query)
        mel = x.detach().float().contiguous()
        if T % 4:                                               # rows on 16-byte boundaries: vector staging in the first conv
            mel = torch.nn.functional.pad(mel, (0, 4 - T % 4))
        with torch.cuda.device(device):
            ws = self.workspace((device, B, T), lambda: _lib.nbytes(ws_bytes, C.byref(self._cfg), B, T,
                                                                    what="ctts_hifigan_workspace_bytes"), zero=False)
            audio = torch.empty(B, 1, T * self.upsample_factor, dtype=torch.float32, device=device)
            _lib.check(getattr(lib, fwd)(C.byref(self._cfg), _lib.ptr(blob), _lib.ptr(mel), mel.shape[2], _lib.ptr(audio),
                                         B, T, _lib.ptr(ws), ws.numel() * 4, _lib.stream(device)), fwd)
        return audio if x.dtype == torch.float32 else audio.to(x.dtype)


def load_model(model_path, device='cuda', trust_checkpoint=False, compute_dtype=None, f32_gemm_mode=None):
    """``hifigan.models.load_model`` (models.py:14-31): ``config.json`` beside the checkpoint, key ``'generator'`` with the
    weight-norm keys, weight norm removed after loading.  Returns ``(generator, h)``.

    The checkpoint is read with ``weights_only=True`` (no pickle code execution); one that pickles other objects needs
    ``trust_checkpoint=True`` - only for files you produced yourself.  ``compute_dtype`` (``torch.float32`` /
    ``torch.float16``) is handed to ``Generator.set_compute_dtype``, ``f32_gemm_mode`` to ``Generator.set_f32_gemm_mode``."""
    with open(os.path.join(os.path.split(model_path)[0], 'config.json')) as f:
        h = AttrDict(json.loads(f.read()))
    generator = Generator(h)
    try:
        cp_dict = torch.load(model_path, map_location='cpu', weights_only=True)
    except Exception:
        if not trust_checkpoint:
            raise
        cp_dict = torch.load(model_path, map_location='cpu', weights_only=False)
    generator.load_state_dict(cp_dict['generator'])
    generator = generator.to(device).eval()
    generator.remove_weight_norm()
    if compute_dtype is not None:
        generator.set_compute_dtype(compute_dtype)
    if f32_gemm_mode is not None:
        generator.set_f32_gemm_mode(f32_gemm_mode)
    return generator, h
