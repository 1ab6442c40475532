"""WaveFlow / "ax" WaveGlow core on the MI355X HIP path (BASELINE config 4, the ``waveflow=False`` WaveGlow the
reference's own timing notebook runs, and every other config the reference tree prints).

Host-side mirror of ``/root/reference/CookieTTS/_4_mtw/waveglow/efficient_model_ax.py``
``WaveGlow`` (:18-169 constructor, :279-357 ``inverse``, :359-388 ``infer``):

* ``waveflow=True``: ``WaveFlowCoupling`` + ``WN_2d`` (efficient_modules.py:19-65, glow_ax.py:421-635) ->
  ``ctts_waveflow_inverse_f32`` / ``ctts_waveflow_inverse_cond_f32``;
* ``waveflow=False``: ``AffineCouplingBlock`` + the 1-D ``WN`` (efficient_modules.py:68-105, glow_ax.py:245-418) ->
  ``ctts_wgax_inverse_f32``, or ``ctts_wgax_inverse_f16`` (IEEE-half WN activations, f16 matrix pipe, GTU only) after
  ``set_compute_dtype(torch.float16)``;
* on both: ``PermuteHeight`` or ``InvertibleConv1x1`` mixing in either ``mix_first`` order, early outputs, all
  fourteen gated units, ``merge_res_skip`` / ``res_skip=False``, per-layer dilations, speaker embeddings at model and
  WN level, the model-level conditioning stack (plain / residual / 1x1-conv residual, rezero), multi-layer WN
  conditioning stacks with activations, the grouped per-flow cond conv, model- and WN-level
  ``TransposedUpsampleNet``, spect shift / scale, log-variance mel channels, perceived-volume companding,
  de-emphasis; separable (depthwise + pointwise) in-layers on both cores (the 1-D core: up to 31 taps, fp32 storage,
  ``ctts_wgax_sep_inverse_f32``).

Same constructor kwargs, same ``state_dict`` keys (``WN.k.WN.{start,cond_layers.l,in_layers.i,res_skip_layers.i}.
{weight_g,weight_v,bias}``, ``WN.k.WN.end.{weight,bias}``, ``convinv.k.weight``, ``upsample_net.*``, ...), same
``infer`` / ``inverse`` contracts (output length ``(F-1)*hop`` with the default ``artifact_trimming=1``;
``return_CPU=True`` moves the result to the host like the reference).  The few options left raise
NotImplementedError.  The conditioning stacks are composed on the host from operator-level C entry points
(``ctts_conv1d_f32``, ``ctts_embed_rows_f32``, ``ctts_scale_add_rows_f32``, ``ctts_resample_rows_f32``,
``ctts_interleave_phases_f32``, ...); all arithmetic runs in the C-ABI HIP library; no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import numpy as np

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _cache, _lib
from ._wn import WNConv, folded_weight
from ._lib import PAD          # halo of the frame-rate padded rows (>= k/2 of every cond conv, k <= 11)

__all__ = ["WaveGlow"]


class _WN2d(nn.Module):
    """Parameter tree of glow_ax.WN_2d (:427-543)."""

    def __init__(self, cond_in, wn):
        super().__init__()
        C_, n_layers = wn['n_channels'], wn['n_layers']
        kh, kw = wn['kernel_size_h'], wn['kernel_size_w']
        self.n_layers, self.n_channels = n_layers, C_
        sdim = wn.get('speaker_embed_dim', 0)
        self.start = WNConv((C_, 1, 1, 1))
        self.end = nn.Module()
        self.end.weight = nn.Parameter(torch.zeros(2, C_, 1, 1))                # zero-init, glow_ax.py:454-457
        self.end.bias = nn.Parameter(torch.zeros(2))
        if sdim:
            self.speaker_embed = nn.Embedding(512, sdim)                        # glow_ax.py:459-461
        k = 2 * wn.get('cond_kernel_size', 1) - 1                               # glow_ax.py:474
        cond_out = 2 * C_ * n_layers
        if wn.get('transposed_conv_scales') and wn.get('transposed_conv_hidden_dim', 256) and wn.get('transposed_conv_kernel_size', 4):
            # the WN's own TransposedUpsampleNet behind its cond stack (upsample_first is False): the stack ends at the
            # net's hidden width, the net ends at 2C*n_layers (glow_ax.py:286-295 / 462-470)
            hid = wn.get('transposed_conv_hidden_dim', 256)
            self.upsample_net = _TransposedUpsampleNet(hid, cond_out, hid, wn.get('transposed_conv_kernel_size', 4),
                                                       wn['transposed_conv_scales'], False, False, False, False)
            cond_out = hid
        dims = [cond_in + sdim] + [wn['cond_hidden_channels']] * (wn['cond_layers'] - 1) + [cond_out]
        self.cond_layers = nn.ModuleList([WNConv((dims[l + 1], dims[l], k)) for l in range(wn['cond_layers'])])
        if wn.get('seperable_conv', False) and not (kh == 1 and kw == 1):       # glow_ax.py:521-531
            self.in_layers = nn.ModuleList([nn.ModuleList([WNConv((C_, 1, kh, kw)), WNConv((2 * C_, C_, 1, 1))])
                                            for _ in range(n_layers)])
        else:
            self.in_layers = nn.ModuleList([WNConv((2 * C_, C_, kh, kw)) for _ in range(n_layers)])
        merge = bool(wn.get('merge_res_skip', False))                            # glow_ax.py:535-538
        self.res_skip_layers = nn.ModuleList([
            WNConv((2 * C_ if (i < n_layers - 1 and not merge) else C_, C_, 1, 1)) for i in range(n_layers)]
            if wn.get('res_skip', True) else [])                                 # res_skip=False: acts are the skip (:609)


class _WN1d(nn.Module):
    """Parameter tree of the 1-D glow_ax.WN (:251-360)."""

    def __init__(self, n_in, cond_in, wn):
        super().__init__()
        C_, n_layers = wn['n_channels'], wn['n_layers']
        ks = wn.get('kernel_size_w') or wn.get('kernel_size')                    # glow_ax.py:256
        assert ks % 2 == 1 and C_ % 2 == 0
        self.n_layers, self.n_channels = n_layers, C_
        sdim = wn.get('speaker_embed_dim', 0)
        self.start = WNConv((C_, n_in, 1))
        self.end = nn.Module()
        self.end.weight = nn.Parameter(torch.zeros(2 * n_in, C_, 1))            # zero-init, glow_ax.py:278-281
        self.end.bias = nn.Parameter(torch.zeros(2 * n_in))
        if sdim:
            self.speaker_embed = nn.Embedding(512, sdim)                        # glow_ax.py:283-285
        k = 2 * wn.get('cond_kernel_size', 1) - 1                               # glow_ax.py:299
        cond_out = 2 * C_ * n_layers
        if wn.get('transposed_conv_scales') and wn.get('transposed_conv_hidden_dim', 256) and wn.get('transposed_conv_kernel_size', 4):
            # the WN's own TransposedUpsampleNet behind its cond stack (upsample_first is False): the stack ends at the
            # net's hidden width, the net ends at 2C*n_layers (glow_ax.py:286-295 / 462-470)
            hid = wn.get('transposed_conv_hidden_dim', 256)
            self.upsample_net = _TransposedUpsampleNet(hid, cond_out, hid, wn.get('transposed_conv_kernel_size', 4),
                                                       wn['transposed_conv_scales'], False, False, False, False)
            cond_out = hid
        dims = [cond_in + sdim] + [wn['cond_hidden_channels']] * (wn['cond_layers'] - 1) + [cond_out]
        self.cond_layers = nn.ModuleList([WNConv((dims[l + 1], dims[l], k)) for l in range(wn['cond_layers'])])
        if wn.get('seperable_conv', False) and ks != 1:                          # glow_ax.py:337-348
            self.in_layers = nn.ModuleList([nn.ModuleList([WNConv((C_, 1, ks)), WNConv((2 * C_, C_, 1))])
                                            for _ in range(n_layers)])
        else:
            self.in_layers = nn.ModuleList([WNConv((2 * C_, C_, ks)) for _ in range(n_layers)])
        merge = bool(wn.get('merge_res_skip', False))                            # glow_ax.py:352-355
        self.res_skip_layers = nn.ModuleList([
            WNConv((2 * C_ if (i < n_layers - 1 and not merge) else C_, C_, 1)) for i in range(n_layers)]
            if wn.get('res_skip', True) else [])                                 # res_skip=False: acts are the skip (:401)


class InvertibleConv1x1(nn.Module):
    """Parameter holder of efficient_modules.InvertibleConv1x1 (:235-253): ``weight`` [c, c, 1], random orthonormal
    with det > 0.  ``W_inverse`` is cached on the module after the first inference like the reference (:271-276)."""

    def __init__(self, c):
        super().__init__()
        W = torch.linalg.qr(torch.randn(c, c))[0]
        if torch.det(W) < 0:
            W[:, 0] = -1 * W[:, 0]
        self.weight = nn.Parameter(W.view(c, c, 1).contiguous())


class _Coupling(nn.Module):
    def __init__(self, wn):
        super().__init__()
        self.WN = wn


def _act_code(name, negative_slope):
    """The reference's activation table (ax:100-111 = glow_ax.py:493-504) -> (ctts_conv1d act, slope).
    As written there, 'lrelu' selects ``F.relu`` and 'relu' selects ``LeakyReLU(negative_slope)``."""
    name = (name or 'none').lower()
    if name == 'none':
        return 0, 0.0
    if name == 'lrelu':
        return 1, 0.0
    if name == 'relu':
        assert negative_slope, "negative_slope not defined in wn_config"
        return 1, float(negative_slope)
    if name == 'tanh':
        return 2, 0.0
    if name == 'sigmoid':
        return 3, 0.0          # composed in _CondConv: sigmoid(x) = (tanh(x / 2) + 1) / 2
    raise NotImplementedError(name)                                            # ax:111


class _CondConv:
    """One ``ctts_conv1d`` operator of a conditioning stack: dense [out, in, k] weight, input channels zero-padded
    to the primitive's multiple of 16."""

    batched = True      # one launch for the whole batch when the buffers allow it (tests turn it off to compare)

    def __init__(self, w, b, act, slope, device, stream, gemm_mode=0):
        lib = _lib.lib()
        out_c, in_c, k = w.shape
        self.c_in, self.c_out = -(-in_c // 16) * 16, out_c
        self.sigmoid = act == 3
        wp = torch.zeros(out_c, self.c_in, k, dtype=torch.float32, device=device)
        wp[:, :in_c] = w
        b = b.detach().float().contiguous()
        if self.sigmoid:       # tanh epilogue on the halved pre-activation, then (t + 1) / 2 with ctts_affine_rows_f32
            wp, b, act = wp * 0.5, b * 0.5, 2
        self.desc = _lib.Conv1dDesc(c_in=self.c_in, c_out=out_c, kernel_size=k, act=act, slope=slope,
                                    f32_gemm_mode=gemm_mode)
        nbytes = _lib.nbytes(lib.ctts_conv1d_packed_bytes, C.byref(self.desc), what="unsupported cond conv")
        self.blob = torch.zeros(nbytes // 4, dtype=torch.float32, device=device)
        _lib.check(lib.ctts_conv1d_pack_f32(C.byref(self.desc), _lib.ptr(wp), _lib.ptr(b), None, None, None, None, 1e-5,
                                           _lib.ptr(self.blob), stream), "ctts_conv1d_pack_f32")
        self._keep = (wp, b)

    def __call__(self, x, y, B, T, ld, stream, padding_mode='zeros'):
        # x [B][>= c_in rows][ld], y [B][>= c_out rows][ld]: the row counts of the buffers are rounded up to 16, so the
        # primitive (dense [batch][c][ld] strides) is driven one utterance at a time
        k = self.desc.kernel_size
        if padding_mode == 'replicate' and k > 1:      # edge values into the halo the taps reach (nn.Conv1d padding_mode)
            _lib.check(_lib.lib().ctts_replicate_halo_f32(_lib.ptr(x), B, x.shape[1], T, ld, PAD, k // 2, stream),
                       "ctts_replicate_halo_f32")
        if (self.batched and not self.sigmoid and x.shape[1] == self.c_in and y.shape[1] == self.c_out
                and tuple(x.stride()) == (self.c_in * ld, ld, 1) and tuple(y.stride()) == (self.c_out * ld, ld, 1)):
            # both buffers have exactly the operator's row counts: the dense [batch][c][ld] strides of the primitive hold
            # for the whole batch, one launch (B x the workgroups) instead of B
            _lib.check(_lib.lib().ctts_conv1d_f32(C.byref(self.desc), _lib.ptr(self.blob), _lib.ptr(x), _lib.ptr(y),
                                                 0, B, T, ld, PAD, stream), "ctts_conv1d_f32")
            return
        for b in range(B):
            _lib.check(_lib.lib().ctts_conv1d_f32(C.byref(self.desc), _lib.ptr(self.blob), _lib.ptr(x[b]), _lib.ptr(y[b]),
                                                 0, 1, T, ld, PAD, stream), "ctts_conv1d_f32")
            if self.sigmoid:
                _lib.check(_lib.lib().ctts_affine_rows_f32(_lib.ptr(y[b]), 1, y.shape[1], self.c_out, T, ld, PAD, 1.0, 0.5,
                                                           stream), "ctts_affine_rows_f32")


def _r16(n):
    return -(-n // 16) * 16


def _ld_for(T):
    """Row stride of a padded [B][rows][ld] buffer with T valid columns (a few spare columns for the transposed-conv
    phases, which run a little past the input length)."""
    return -(-(T + 8) // 128) * 128 + 2 * PAD


class _TransposedConv:
    """``nn.ConvTranspose1d(in, out, k, stride=s, padding=(k - s) // 2)`` (+ LeakyReLU) of ``TransposedUpsampleNet``
    (glow_ax.py:222-226) as ``s`` stride-1 convolutions, one per output residue r = (n + p) mod s:
    out[n] = sum_q W[:, :, r + q s]^T x[(n + p) // s - q], run by ``ctts_conv1d_f32`` over the input positions and
    interleaved by ``ctts_interleave_phases_f32``."""

    def __init__(self, w, b, s, act, slope, device, stream, gemm_mode=0):
        in_c, out_c, k = w.shape                                   # ConvTranspose1d weight layout
        if (k - s) % 2 or k < s:
            raise NotImplementedError(f"transposed conv with kernel {k}, stride {s}: output length is not stride * T")
        Q = -(-k // s)
        wr = torch.zeros(s, out_c, in_c, 2 * Q - 1, dtype=torch.float32, device=device)
        for r in range(s):
            for q in range(Q):
                if r + q * s < k:
                    wr[r, :, :, Q - 1 - q] = w[:, :, r + q * s].t()   # tap offset -q of a 'same' conv with 2Q-1 taps
        self.ops = [_CondConv(wr[r], b, act, slope, device, stream, gemm_mode) for r in range(s)]
        self.s, self.p, self.out_c = s, (k - s) // 2, out_c
        self.extra = (k - self.p - 1) // s                          # phase positions needed past the input length

    def __call__(self, x, B, T, ld, stream):
        dev = x.device
        Tp, T_out = T + self.extra, T * self.s
        assert ld >= PAD + Tp + PAD
        ph = torch.zeros(self.s, B, _r16(self.out_c), ld, dtype=torch.float32, device=dev)
        for r, op in enumerate(self.ops):
            op(x, ph[r], B, Tp, ld, stream)
        ld_out = _ld_for(T_out)
        y = torch.zeros(B, _r16(self.out_c), ld_out, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().ctts_interleave_phases_f32(_lib.ptr(ph), _lib.ptr(y), B, y.shape[1], self.s, self.p, Tp, ld,
                                                         PAD, T_out, ld_out, PAD, stream), "ctts_interleave_phases_f32")
        return y, T_out, ld_out


class _TransposedUpsampleNet(nn.Module):
    """Parameter holder with the reference's ``state_dict`` layout (glow_ax.py:201-242): ``t_convs`` alternates
    ConvTranspose1d and LeakyReLU(0.4) modules, ``res_weight`` exists with rezero."""

    def __init__(self, in_channels, out_channels, hidden_channels, kernel_size, scales, use_last_layer_act_func, residual,
                 residual_linear, rezero):
        super().__init__()
        self.residual, self.residual_linear = bool(residual), bool(residual_linear)
        self.res_weight = nn.Parameter(torch.rand(1) * 0.02 + 0.01) if rezero else None
        self.scales = list(scales)
        self.t_convs = nn.ModuleList()
        self.acts = []
        for i, scale in enumerate(self.scales):
            last = i + 1 == len(self.scales)
            in_dim = in_channels if i == 0 else hidden_channels
            out_dim = out_channels if last else hidden_channels
            k = kernel_size[i] if isinstance(kernel_size, (list, tuple)) else kernel_size
            self.t_convs.append(nn.ConvTranspose1d(in_dim, out_dim, k, scale, padding=(k - scale) // 2))
            act = (not last) or use_last_layer_act_func
            if act:
                self.t_convs.append(nn.LeakyReLU(negative_slope=0.4))
            self.acts.append(act)
        self.res_channels = min(in_channels, out_channels)
        self.out_channels = out_channels

    def convs(self):
        return [m for m in self.t_convs if isinstance(m, nn.ConvTranspose1d)]


class WaveGlow(_cache.PackedModule):
    GPU_ONLY = "WaveFlow HIP path needs the model on a GPU (no CPU fallback)"

    def __init__(self, n_mel_channels, n_flows, n_group, n_early_every, n_early_size, memory_efficient,
                 spect_scaling, upsample_mode, upsample_first, speaker_embed, cond_layers, cond_hidden_channels,
                 cond_output_channels, cond_kernel_size, cond_residual, cond_padding_mode, WN_config, win_length,
                 hop_length, sampling_rate=48000, cond_res_rezero=False, cond_activation_func='none',
                 negative_slope=None, channel_mixing='1x1conv', mix_first=True, preceived_vol_scaling=False,
                 waveflow=True, yoyo='depreciated', yoyo_WN='depreciated', shift_spect=0., scale_spect=1.,
                 preempthasis=None, use_logvar_channels=False, load_hidden_from_disk=False,
                 transposed_conv_hidden_dim=256, transposed_conv_kernel_size=4, transposed_conv_scales=None,
                 transposed_conv_output_dim=256, transposed_conv_residual=False, transposed_conv_residual_linear=False,
                 transposed_conv_res_rezero=False, group_conv_output_dim=None, group_conv_groupped=True, iso226_empthasis=False):
        super().__init__()
        assert n_group % 2 == 0
        assert hop_length % n_group == 0, "hop_length is not int divisible by n_group"
        wn = dict(WN_config)

        def need(cond, what):
            if not cond:
                raise NotImplementedError(f"ax-core option not built on the HIP path yet: {what}")
        assert any(channel_mixing.lower() in x for x in ("1x1convinvertibleconv1x1invconv",
                                                         "waveflowpermuteheightpermutechannelpermute")), \
            "channel_mixing option is invalid. Options are '1x1conv' or 'permuteheight'"          # ax:24
        mixing = '1x1conv' if channel_mixing.lower() in "1x1convinvertibleconv1x1invconv" else 'permuteheight'   # ax:25
        if waveflow:
            need(n_group <= 64, "waveflow=True with n_group > 64")
        else:
            need(wn['n_channels'] % 32 == 0, "waveflow=False with n_channels not a multiple of 32")
            need(n_group <= 32, "waveflow=False with n_group > 32")
        need(cond_residual in (False, True, 0, 1, '1x1conv'), f"cond_residual={cond_residual!r}")
        use_tconv = bool(transposed_conv_scales) and bool(transposed_conv_hidden_dim) and bool(transposed_conv_kernel_size)
        need(upsample_first is False or upsample_first is True or upsample_first is None or upsample_first == 0,
             f"upsample_first={upsample_first!r}")
        if upsample_first is True:                                # ax:121-126, 174-186: cond upsampled at model level
            need(use_tconv, "upsample_first=True without a TransposedUpsampleNet")
            need(transposed_conv_residual_linear or not transposed_conv_residual,
                 "transposed_conv_residual with 'nearest' interpolation (F.interpolate rejects align_corners there: the "
                 "reference raises ValueError, glow_ax.py:231)")
        else:
            need(not use_tconv, "TransposedUpsampleNet with upsample_first != True")
        wn_tconv = bool(wn.get('transposed_conv_scales')) and bool(wn.get('transposed_conv_hidden_dim', 256)) \
            and bool(wn.get('transposed_conv_kernel_size', 4))
        need(not (wn_tconv and upsample_first is True), "WN-level TransposedUpsampleNet together with upsample_first=True")
        need(not wn_tconv or wn.get('cond_layers', 1) >= 1, "WN-level TransposedUpsampleNet without WN cond layers")
        self._wn_tconv_factor = int(np.prod(wn['transposed_conv_scales'])) if wn_tconv else 0
        need(cond_padding_mode in ('zeros', 'replicate') and wn.get('cond_padding_mode', 'zeros') in ('zeros', 'replicate'),
             "cond_padding_mode other than 'zeros' / 'replicate'")
        need(not iso226_empthasis, "iso226 emphasis")
        need(wn.get('cond_layers', 1) >= 1, "WN without cond layers")
        need(wn.get('upsample_mode', 'linear') == 'linear', "WN upsample_mode != 'linear'")
        if waveflow:                                                            # glow_ax.py:259 / :433
            assert wn.get('res_skip', True) or wn.get('merge_res_skip', False), \
                "Cannot remove res_skip without using merge_res_skip"
        else:
            assert (wn.get('res_skip', True) or wn.get('merge_res_skip', False)) or wn['n_layers'] == 1, \
                "Cannot remove res_skip without using merge_res_skip"
        if str(wn.get('gated_unit', 'GTU')).upper() not in _lib.GATED_UNITS:
            raise Exception("gated_unit is invalid\nOptions are ('GTU','GTRU','GLU').")     # glow_ax.py:198
        assert not wn.get('rezero', False), "WN ReZero is depreciated"                         # glow_ax.py:272, 450
        need(wn['n_layers'] <= 12, "more than 12 WN layers")
        if waveflow:
            dh = wn.get('n_layers_dilations_h', 1)
            dh = [dh] * wn['n_layers'] if isinstance(dh, int) else list(dh)
            need(all(d >= 1 for d in dh), "height dilation < 1")
            need(wn.get('seperable_conv', False) or wn['kernel_size_h'] * wn['kernel_size_w'] <= 11,
                 "dense in-layer kernels with more than 11 taps (use seperable_conv)")
        else:
            ks1 = wn.get('kernel_size_w') or wn.get('kernel_size')
            if wn.get('seperable_conv', False) and ks1 != 1:
                need(ks1 <= 31, "separable 1-D in-layer kernels wider than 31")
            else:
                need(ks1 <= 11, "dense 1-D in-layer kernels wider than 11 (use seperable_conv)")
        need(2 * cond_kernel_size - 1 <= 11 and 2 * wn.get('cond_kernel_size', 1) - 1 <= 11, "cond kernels wider than 11")
        assert mixing != 'permuteheight' or n_flows % 2 == 0, "PermuteHeight requires even n_flows"

        self.waveflow = bool(waveflow)
        self.n_flows, self.n_group = n_flows, n_group
        self.n_early_every, self.n_early_size = n_early_every, n_early_size
        self.sampling_rate, self.win_size, self.hop_length = sampling_rate, win_length, hop_length
        self.n_mel_channels = n_mel_channels
        self.channel_mixing, self.mix_first = mixing, bool(mix_first)
        self.cond_padding_mode = cond_padding_mode
        self.ignore_nan = True                                                   # ax:50
        self.has_logvar_channels = bool(use_logvar_channels)
        self.preempthasis = preempthasis
        self.speaker_embed_dim = speaker_embed
        self.multispeaker = speaker_embed > 0 or wn.get('speaker_embed_dim', 0) > 0
        self.cond_residual, self.cond_res_rezero = cond_residual, cond_res_rezero
        self.shift_spect, self.scale_spect = float(shift_spect), float(scale_spect)
        self.vol_scaling = bool(preceived_vol_scaling)
        self.use_hidden_cond = load_hidden_from_disk                              # ax:36: a data-loader hint, not used by the model
        self.upsample_early = upsample_first is True
        self.WN_config = wn
        # activation tables (validated now so that an unsupported name fails at construction)
        self._act_model = _act_code(cond_activation_func if cond_layers else 'none', negative_slope)
        self._act_wn = _act_code(wn.get('cond_activation_func', 'none'), wn.get('negative_slope'))

        if speaker_embed:
            self.speaker_embed = nn.Embedding(512, speaker_embed)                # ax:59-61
        self.cond_in_channels = n_mel_channels * (2 if use_logvar_channels else 1) + speaker_embed   # ax:64
        wn_cond = self.cond_in_channels
        if cond_res_rezero:
            self.alpha = nn.Parameter(torch.rand(1) * 0.02 + 0.01)               # ax:75-76
        self.cond_layers = nn.ModuleList()
        if cond_layers:
            out_c = self.cond_in_channels if (cond_residual is True or cond_residual == 1) else cond_output_channels  # ax:72-73
            if cond_residual == '1x1conv':
                self.res_conv = nn.Conv1d(self.cond_in_channels, out_c, 1)       # ax:80-81
            k = 2 * cond_kernel_size - 1                                         # ax:83
            dims = [self.cond_in_channels] + [cond_hidden_channels] * (cond_layers - 1) + [out_c]
            self.cond_layers = nn.ModuleList([WNConv((dims[l + 1], dims[l], k)) for l in range(cond_layers)])
            wn_cond = out_c
        if self.upsample_early:                                                  # ax:116-126
            t_out = transposed_conv_output_dim if transposed_conv_output_dim is not None else wn_cond
            self.upsample_net = _TransposedUpsampleNet(wn_cond, t_out, transposed_conv_hidden_dim,
                                                       transposed_conv_kernel_size, transposed_conv_scales, True,
                                                       transposed_conv_residual, transposed_conv_residual_linear,
                                                       transposed_conv_res_rezero)
            self.model_cond_channels = wn_cond
            wn_cond = t_out
        self.group_conv_in = 0
        if group_conv_output_dim:                                                # ax:131-134: per-flow 1x1 conv of the cond
            groups = n_flows if group_conv_groupped else 1
            assert wn_cond % groups == 0, "in_channels must be divisible by groups"
            self.n_flow_group_conv = nn.Conv1d(wn_cond, group_conv_output_dim * n_flows, 1, groups=groups)
            self.group_conv_in = wn_cond
            wn_cond = group_conv_output_dim
        self.wn_cond_channels = wn_cond
        if waveflow:                                                             # ax:166-189 (the 2-D WN does not
            self.WN = nn.ModuleList([_Coupling(_WN2d(wn_cond, wn)) for _ in range(n_flows)])   # depend on the row count)
            self.convinv = nn.ModuleList() if mixing == '1x1conv' else []        # PermuteHeight: no parameters (ax:144)
            n_rem = n_group
            self.z_split_sizes = []
            for k in range(n_flows):
                if k % n_early_every == 0 and k > 0:
                    n_rem -= n_early_size
                    self.z_split_sizes.append(n_early_size)
                assert n_rem > 0, "n_remaining_channels is 0. (increase n_group or decrease n_early_every/n_early_size)"
                if mixing == '1x1conv':
                    self.convinv.append(InvertibleConv1x1(n_rem))
            self.z_split_sizes.append(n_rem)
        else:
            self.WN = nn.ModuleList()
            self.convinv = nn.ModuleList() if mixing == '1x1conv' else []
            n_rem = n_group
            self.z_split_sizes = []
            for k in range(n_flows):
                if k % n_early_every == 0 and k > 0:
                    n_rem -= n_early_size
                    self.z_split_sizes.append(n_early_size)
                assert n_rem > 0, "n_remaining_channels is 0. (increase n_group or decrease n_early_every/n_early_size)"
                need(n_rem % 2 == 0, "odd number of remaining channels")
                if mixing == '1x1conv':
                    self.convinv.append(InvertibleConv1x1(n_rem))
                self.WN.append(_Coupling(_WN1d(n_rem // 2, wn_cond, wn)))
            self.z_split_sizes.append(n_rem)
        # one k=1 linear WN cond layer on the bare mel commutes with the interpolation: folded into the in-layer GEMM
        self._folded = (bool(waveflow) and not cond_layers and not speaker_embed and not wn.get('speaker_embed_dim', 0)
                        and not group_conv_output_dim and not wn_tconv and not self.upsample_early
                        and self.shift_spect == 0. and self.scale_spect == 1.
                        and wn.get('cond_layers', 1) == 1 and wn.get('cond_kernel_size', 1) == 1
                        and self._act_wn[0] == 0)
        # separable (depthwise + pointwise) in-layers of the 1-D core: the ctts_wgax_sep_* entry points
        self._sep1d = (not waveflow) and isinstance(self.WN[0].WN.in_layers[0], nn.ModuleList)
        self._f32_gemm_mode = None
        self._compute_dtype = torch.float32
        self._fwd = None             # (the inverse blob it belongs to, forward-mix blob or None, log|det W_k| per column, fp32 on the host)

    # ------------------------------------------------------------------ plumbing ----
    def c_config(self):
        wn = self.WN_config
        return _lib.WaveFlowConfig(n_mel_channels=self.cond_in_channels, n_flows=self.n_flows, n_group=self.n_group,
                                   n_layers=wn['n_layers'], n_channels=wn['n_channels'],
                                   kernel_size_w=wn['kernel_size_w'], kernel_size_h=wn['kernel_size_h'], dilation_h=1,
                                   seperable_conv=1 if wn.get('seperable_conv', False) else 0,
                                   gated_unit=_lib.GATED_UNITS[str(wn.get('gated_unit', 'GTU')).upper()],
                                   merge_res_skip=1 if (wn.get('merge_res_skip', False) or not wn.get('res_skip', True)) else 0,
                                   n_early_every=self.n_early_every, n_early_size=self.n_early_size,
                                   mixing=_lib.MIX_CONV1X1 if self.channel_mixing == '1x1conv' else _lib.MIX_PERMUTE,
                                   mix_first=1 if self.mix_first else 0,
                                   dilation_w=_lib.dilation_array(wn.get('n_layers_dilations_w'), wn['n_layers']),
                                   dilation_h_l=_lib.dilation_array(wn.get('n_layers_dilations_h', 1), wn['n_layers']),
                                   cond_precomputed=0 if self._folded else 1,
                                   f32_gemm_mode=_lib.model_gemm_mode(self._f32_gemm_mode))

    def set_f32_gemm_mode(self, mode):
        """Main loop of THIS model's GEMMs (both cores, and the conditioning operators in front of them): ``"f32"``,
        ``"bf16x3"``, ``"bf16x6"`` or ``None`` / ``"default"`` (the library default).  See ``waveglow.WaveGlow.set_f32_gemm_mode``."""
        _lib.model_gemm_mode(mode)
        self._f32_gemm_mode = mode
        self._invalidate()            # the conditioning operators carry the mode in their packed descriptors
        return self

    def set_compute_dtype(self, dtype):
        """Storage and product format of the 1-D core's (``waveflow=False``) WN stacks: ``torch.float32`` (default) or
        ``torch.float16`` - the reference's ``.half()``: x, the gated activations and the skip sum live as IEEE half in
        the K8-blocked layout, in-layer and res/skip products run on the f16 matrix pipe with fp32 accumulation
        (``ctts_wgax_inverse_f16``).  The latent rows, the coupling, the mixing matrices, ``start`` / ``end``, every
        bias and the whole conditioning side stay fp32, and so do the parameters (fp32 masters); switching back to
        ``torch.float32`` restores the fp32 path bit for bit.

        ``NotImplementedError`` - here, not at the first ``infer`` - for what half storage is not built for:
        ``waveflow=True`` (the 2-D core's <= 128-channel row queue is latency-bound: narrower tensors buy nothing there,
        ``set_f32_gemm_mode("bf16x3")`` is its reduced-precision mode), a gated unit other than GTU (the 16-bit gate
        epilogue is tanh * sigmoid only; the sin(16 x) units would leave the 1e-3 waveform bound), ``seperable_conv``
        in-layers (the depthwise stage is built on fp32 rows only), or a plan the library refuses (kernel_size *
        n_channels / 32 beyond the 16-bit GEMM's chunk table)."""
        if dtype not in (torch.float32, torch.float16):
            raise ValueError(f"compute dtype must be torch.float32 or torch.float16, not {dtype!r}")
        if dtype == torch.float16:
            if self.waveflow:
                raise NotImplementedError("half storage is not built for waveflow=True (latency-bound row queue); "
                                          "use set_f32_gemm_mode('bf16x3')")
            if self._sep1d:
                raise NotImplementedError("half storage is not built for seperable_conv in-layers (fp32 depthwise stage); "
                                          "use set_f32_gemm_mode('bf16x3')")
            unit = str(self.WN_config.get('gated_unit', 'GTU')).upper()
            if unit != 'GTU':
                raise NotImplementedError(f"half storage is built for gated_unit='GTU' only, this model has {unit!r}")
            lib = _lib.lib()
            cfg = self.c_config_1d()
            if lib.ctts_wgax_packed_f16_bytes(C.byref(cfg)) == 0:
                raise NotImplementedError("half storage refused by the library: " + _lib.last_error())
        if dtype != self._compute_dtype:
            self._compute_dtype = dtype
            self._invalidate()        # the packed blob and the workspaces are per format
        return self

    def c_config_1d(self):
        wn = self.WN_config
        return _lib.WgaxConfig(n_flows=self.n_flows, n_group=self.n_group, n_early_every=self.n_early_every,
                               n_early_size=self.n_early_size, n_layers=wn['n_layers'], n_channels=wn['n_channels'],
                               kernel_size=wn.get('kernel_size_w') or wn.get('kernel_size'),
                               mixing=_lib.MIX_CONV1X1 if self.channel_mixing == '1x1conv' else _lib.MIX_PERMUTE,
                               mix_first=1 if self.mix_first else 0, ignore_nan=1 if self.ignore_nan else 0,
                               gated_unit=_lib.GATED_UNITS[str(wn.get('gated_unit', 'GTU')).upper()],
                               merge_res_skip=1 if (wn.get('merge_res_skip', False) or not wn.get('res_skip', True)) else 0,
                               dilation_w=_lib.dilation_array(wn.get('n_layers_dilations_w'), wn['n_layers']),
                               f32_gemm_mode=_lib.model_gemm_mode(self._f32_gemm_mode))

    def _invalidate(self):
        super()._invalidate()
        self._fwd = None
        for m in (self.convinv if isinstance(self.convinv, nn.ModuleList) else []):
            if hasattr(m, 'W_inverse'):
                del m.W_inverse

    def remove_weightnorm(self):
        for m in self.modules():
            if isinstance(m, WNConv):
                m.remove_weight_norm()
        self._invalidate()

    def _ensure_packed(self, device):
        """-> (blob, cond_ops): packed WaveFlow weights, and (unless the cond layer is folded) the conv operators
        of the conditioning stacks {'model': [...], 'wn': [[...] per flow]}."""
        return self.packed(device, lambda: self._pack(device))

    def _pack(self, device):
        lib = _lib.lib()
        wn_cfg = self.WN_config
        n_layers = wn_cfg['n_layers']
        half = self._compute_dtype == torch.float16
        if self.waveflow:
            cfg = self.c_config()
            size, pack_flow, name = lib.ctts_waveflow_packed_bytes, lib.ctts_waveflow_pack_flow, "ctts_waveflow_pack_flow"
        else:
            cfg = self.c_config_1d()
            if self._sep1d:
                size, pack_flow, name = lib.ctts_wgax_sep_packed_bytes, lib.ctts_wgax_sep_pack_flow, "ctts_wgax_sep_pack_flow"
            else:
                size = lib.ctts_wgax_packed_f16_bytes if half else lib.ctts_wgax_packed_bytes
                pack_flow, name = (lib.ctts_wgax_pack_flow_f16 if half else lib.ctts_wgax_pack_flow), "ctts_wgax_pack_flow"
        nbytes = _lib.nbytes(size, C.byref(cfg), what="unsupported ax-core config")
        sep = isinstance(self.WN[0].WN.in_layers[0], nn.ModuleList)
        with torch.cuda.device(device):
            stream = _lib.stream(device)
            blob = torch.zeros(nbytes // 4, dtype=torch.float32, device=device)
            keep = []

            def arr(fn):
                a = (C.c_void_p * n_layers)()
                for i in range(n_layers):
                    a[i] = fn(i)
                return a
            # res_skip=False (glow_ax.py:401 / :609: `res_skip_acts = acts`): the same launch with an identity weight
            no_rs = not wn_cfg.get('res_skip', True)
            if no_rs:
                eye = torch.eye(wn_cfg['n_channels'], dtype=torch.float32, device=device).contiguous()
                zero_b = torch.zeros(wn_cfg['n_channels'], dtype=torch.float32, device=device)
                keep += [eye, zero_b]

            for k in range(self.n_flows):
                # start / in / rs / end / w_inverse are the same fields in both cores' structs; the 2-D core adds cond and dw
                wn = self.WN[k].WN
                fw = _lib.WaveFlowFlowWeights() if self.waveflow else _lib.WgaxFlowWeights()
                gemm = (lambda i: wn.in_layers[i][1]) if sep else (lambda i: wn.in_layers[i])
                fw.start_w = folded_weight(wn.start, stream, keep).data_ptr()
                fw.start_b = _cache.dev(wn.start.bias, keep)
                if self._folded:
                    fw.cond_w = folded_weight(wn.cond_layers[0], stream, keep).data_ptr()
                    fw.cond_b = _cache.dev(wn.cond_layers[0].bias, keep)
                fw.in_w = arr(lambda i: folded_weight(gemm(i), stream, keep).data_ptr())
                fw.in_b = arr(lambda i: _cache.dev(gemm(i).bias, keep))
                if sep:
                    dw_w = arr(lambda i: folded_weight(wn.in_layers[i][0], stream, keep).data_ptr())
                    dw_b = arr(lambda i: _cache.dev(wn.in_layers[i][0].bias, keep))
                    if self.waveflow:
                        fw.dw_w, fw.dw_b = dw_w, dw_b
                fw.rs_w = arr(lambda i: eye.data_ptr() if no_rs else folded_weight(wn.res_skip_layers[i], stream, keep).data_ptr())
                fw.rs_b = arr(lambda i: zero_b.data_ptr() if no_rs else _cache.dev(wn.res_skip_layers[i].bias, keep))
                fw.end_w = _cache.dev(wn.end.weight, keep)
                fw.end_b = _cache.dev(wn.end.bias, keep)
                if self.channel_mixing == '1x1conv':
                    # efficient_modules.py:271-276: W.float().inverse(), cached on the module as W_inverse
                    W = self.convinv[k].weight.detach().squeeze(-1)
                    W_inverse = W.float().cpu().inverse().to(device).contiguous()
                    self.convinv[k].W_inverse = W_inverse[..., None]
                    keep.append(W_inverse)
                    fw.w_inverse = W_inverse.data_ptr()
                if self._sep1d:       # the 1-D struct has no depthwise fields: they travel as arguments
                    _lib.check(pack_flow(C.byref(cfg), k, C.byref(fw), dw_w, dw_b, _lib.ptr(blob), stream), f"{name}({k})")
                else:
                    _lib.check(pack_flow(C.byref(cfg), k, C.byref(fw), _lib.ptr(blob), stream), f"{name}({k})")
            ops = None
            gm = _lib.model_gemm_mode(self._f32_gemm_mode)
            if not self._folded:
                def stack(layers, act, act_last):
                    out = []
                    for l, layer in enumerate(layers):
                        a = act if (act_last or l != len(layers) - 1) else (0, 0.0)
                        out.append(_CondConv(folded_weight(layer, stream, keep), layer.bias, a[0], a[1], device, stream, gm))
                    return out
                ops = {'model': stack(self.cond_layers, self._act_model, True),          # ax:293-297: every layer
                       'res_conv': (_CondConv(self.res_conv.weight.detach().float(), self.res_conv.bias, 0, 0.0, device, stream, gm)
                                    if hasattr(self, 'res_conv') else None),            # ax:303-304
                       'group': self._group_conv_ops(device, stream),                  # ax:131-134, 320-321
                       'wn_tconv': ([[_TransposedConv(m.weight.detach().float(), m.bias, sc, 1 if act else 0, 0.4, device, stream, gm)
                                      for m, sc, act in zip(c.WN.upsample_net.convs(), c.WN.upsample_net.scales,
                                                            c.WN.upsample_net.acts)] for c in self.WN]
                                    if self._wn_tconv_factor else None),                # glow_ax.py:362-373 / 545-554
                       'tconv': ([_TransposedConv(m.weight.detach().float(), m.bias, sc, 1 if act else 0, 0.4, device, stream, gm)
                                  for m, sc, act in zip(self.upsample_net.convs(), self.upsample_net.scales,
                                                        self.upsample_net.acts)]
                                 if self.upsample_early else None),                     # glow_ax.py:214-226
                       'wn': [stack(c.WN.cond_layers, self._act_wn, wn_cfg.get('cond_out_activation_func', True))
                              for c in self.WN]}                                       # glow_ax.py:573-577
            torch.cuda.current_stream(device).synchronize()
        return blob, ops

    def _to_latent_length(self, h, B, rows_n, hT, hld, T, ld, dst, interpolate, stream, two_d):
        """``_upsample_mels`` after the transposed convs (ax:177-185, glow_ax.py:365-372 / 548-553): linear interpolation
        (align_corners=True) to the latent's length when the net's factor is not hop // n_group, else a centre crop -
        the 1-D rule ``[pad_l : -pad_r]`` (the model's own net on both cores, and the 1-D WN's) or, ``two_d``, the 2-D WN's
        ``[pad : -(pad + pad % 2)]``."""
        if interpolate:
            lib = _lib.lib()
            for b in range(B):
                _lib.check(lib.ctts_resample_rows_f32(_lib.ptr(h[b]), _lib.ptr(dst[b]), 1, rows_n, hT, hld, PAD, T, ld, PAD, 0,
                                                      0.0, stream), "ctts_resample_rows_f32")
            return
        if two_d:
            pad = (hT - T) // 2
            lo, hi = pad, pad + pad % 2
        else:
            # ``pad_r = -(audio_len-cond_len)//2`` is (cond_len - audio_len) // 2 (the minus binds first): floor on both sides,
            # so an odd difference leaves one column too many in the reference and its WN fails - refused below
            lo = hi = (hT - T) // 2
        if hT - lo - hi != T or lo < 0:
            raise RuntimeError(f"upsampled conditioning of length {hT} cannot be cropped to the latent's {T} columns "
                               f"(the reference fails on the same shapes)")
        lib = _lib.lib()
        for b in range(B):      # shifted copy: 'nearest' at scale 1 from the source advanced by `lo` columns
            _lib.check(lib.ctts_resample_rows_f32(h[b].data_ptr() + 4 * lo, _lib.ptr(dst[b]), 1, rows_n, hT - lo, hld, PAD, T,
                                                  ld, PAD, 2, 1.0, stream), "ctts_resample_rows_f32")

    def _group_conv_ops(self, device, stream):
        """One dense 1x1 operator per flow out of ``n_flow_group_conv``: flow k owns output rows [k*out, (k+1)*out) and,
        when grouped, reads only its own slice of the input channels -> [(op, first input row)] or None."""
        if not self.group_conv_in:
            return None
        conv = self.n_flow_group_conv
        w, b = conv.weight.detach().float(), conv.bias.detach().float()
        out = w.shape[0] // self.n_flows
        cin_g = w.shape[1]
        ops = []
        for k in range(self.n_flows):
            row0 = k * cin_g if conv.groups > 1 else 0
            ops.append((_CondConv(w[k * out:(k + 1) * out].contiguous(), b[k * out:(k + 1) * out].contiguous(), 0, 0.0,
                                  device, stream, _lib.model_gemm_mode(self._f32_gemm_mode)), row0))
        return ops

    def _cond_frames(self, ops, cond, speaker_ids, stream, out_steps=None):
        """ax:281-307 + glow_ax.py:566-577 -> ([n_flows][B][2C*n_layers][ld] padded rows, ld, T): at frame rate
        (T = frames), or with ``upsample_first=True`` at the rate of the latent (T = out_steps)."""
        lib = _lib.lib()
        dev = cond.device
        B, Cm, Fr = cond.shape
        ld = _ld_for(Fr)
        if self.multispeaker:
            if speaker_ids is None:
                raise Exception("This WaveFlow/WaveGlow model requires speaker ids or speaker embeddings.")   # ax:288
            ids = speaker_ids.to(device=dev, dtype=torch.int64).contiguous()

        def rows(c, ld_=None):
            return torch.zeros(B, _r16(c), ld_ or ld, dtype=torch.float32, device=dev)
        # model-level input: [mel (+logvar), shifted and scaled | speaker embedding]
        x0 = rows(self.cond_in_channels)
        for b in range(B):
            _lib.check(lib.ctts_pad_rows_f32(_lib.ptr(cond[b]), 0, Fr, _lib.ptr(x0[b]), 1, Cm, Fr, ld, PAD, stream),
                       "ctts_pad_rows_f32")
        if self.shift_spect != 0. or self.scale_spect != 1.:                    # ax:281-284
            _lib.check(lib.ctts_affine_rows_f32(_lib.ptr(x0), B, x0.shape[1], Cm, Fr, ld, PAD, self.shift_spect,
                                                self.scale_spect, stream), "ctts_affine_rows_f32")
        if self.speaker_embed_dim:
            tab = self.speaker_embed.weight.detach().float().contiguous()
            _lib.check(lib.ctts_embed_rows_f32(_lib.ptr(tab), _lib.ptr(ids), _lib.ptr(x0), Cm, self.speaker_embed_dim, B,
                                               x0.shape[1], Fr, ld, PAD, stream), "ctts_embed_rows_f32")
        # conv stack, rezero, residual (identity or 1x1 conv of the input, ax:299-307)
        sdim = self.WN_config.get('speaker_embed_dim', 0)
        grp = ops.get('group')
        c_wn_in = self.group_conv_in if grp else self.wn_cond_channels       # channels of the tensor the flows share
        c_model = self.model_cond_channels if self.upsample_early else c_wn_in
        # (+16 spare rows: a grouped per-flow conv reads its input slice rounded up to the primitive's 16 channels)
        xw = rows(c_model + (0 if (self.upsample_early or grp) else sdim) + (16 if grp else 0))
        h = x0
        for op in ops['model']:
            y = rows(op.c_out)
            op(h, y, B, Fr, ld, stream, self.cond_padding_mode)
            h = y
        alpha = self.alpha.detach().float().contiguous() if (self.cond_res_rezero and len(ops['model'])) else None
        resid = None
        if self.cond_residual and len(ops['model']):
            resid = x0
            if ops['res_conv'] is not None:
                resid = rows(ops['res_conv'].c_out)
                ops['res_conv'](x0, resid, B, Fr, ld, stream)
        for b in range(B):     # row counts differ between the buffers: one utterance per call
            _lib.check(lib.ctts_scale_add_rows_f32(_lib.ptr(h[b]), _lib.ptr(alpha), _lib.ptr(None if resid is None else resid[b]),
                                                   _lib.ptr(xw[b]), 1, c_model, Fr, ld, PAD, stream),
                       "ctts_scale_add_rows_f32")
        T = Fr
        if self.upsample_early:                                                  # ax:174-186 with TransposedUpsampleNet
            net = self.upsample_net
            factor = int(np.prod(net.scales))
            h, hT, hld = xw, Fr, ld
            for tc in ops['tconv']:
                h, hT, hld = tc(h, B, hT, hld, stream)
            if net.residual:                                                     # glow_ax.py:229-241
                xi = rows(net.res_channels, hld)
                for b in range(B):
                    _lib.check(lib.ctts_resample_rows_f32(_lib.ptr(xw[b]), _lib.ptr(xi[b]), 1, net.res_channels, Fr, ld, PAD,
                                                          hT, hld, PAD, 1 if net.residual_linear else 2, float(factor),
                                                          stream), "ctts_resample_rows_f32")
                rw = net.res_weight.detach().float().contiguous() if net.res_weight is not None else None
                for b in range(B):
                    _lib.check(lib.ctts_scale_add_rows_f32(_lib.ptr(h[b]), _lib.ptr(rw), _lib.ptr(xi[b]), _lib.ptr(h[b]), 1,
                                                           net.res_channels, hT, hld, PAD, stream), "ctts_scale_add_rows_f32")
                    if net.out_channels > net.res_channels and rw is not None:
                        tail = h[b][net.res_channels:]
                        _lib.check(lib.ctts_scale_add_rows_f32(_lib.ptr(tail), _lib.ptr(rw), None, _lib.ptr(tail), 1,
                                                               net.out_channels - net.res_channels, hT, hld, PAD, stream),
                                   "ctts_scale_add_rows_f32")
            # to the length of the latent (ax:177-178: 'linear', align_corners=True)
            T = out_steps
            ld = _ld_for(T)
            xw = rows(c_wn_in + (0 if grp else sdim) + (16 if grp else 0))
            self._to_latent_length(h, B, c_wn_in, hT, hld, T, ld, xw, factor != self.hop_length // self.n_group, stream,
                                   two_d=False)                              # efficient_model_ax._upsample_mels: the 1-D rule
        # per flow: WN speaker embedding, conv stack -> 2C*n_layers rows
        C2L = 2 * self.WN_config['n_channels'] * self.WN_config['n_layers']
        wn_up = ops.get('wn_tconv')                 # per-flow TransposedUpsampleNet behind the WN cond stack
        T_out, ld_out = (out_steps, _ld_for(out_steps)) if wn_up else (T, ld)
        frames = torch.zeros(self.n_flows, B, C2L, ld_out, dtype=torch.float32, device=dev)
        xk = rows(self.wn_cond_channels + sdim) if grp else xw
        for k in range(self.n_flows):
            if grp:                                                              # this flow's chunk of the group conv
                op, row0 = grp[k]
                op(xw[:, row0:], xk, B, T, ld, stream)
            if sdim:
                tab = self.WN[k].WN.speaker_embed.weight.detach().float().contiguous()
                _lib.check(lib.ctts_embed_rows_f32(_lib.ptr(tab), _lib.ptr(ids), _lib.ptr(xk), self.wn_cond_channels, sdim,
                                                   B, xk.shape[1], T, ld, PAD, stream), "ctts_embed_rows_f32")
            h = xk
            for l, op in enumerate(ops['wn'][k]):
                y = frames[k] if (l == len(ops['wn'][k]) - 1 and not wn_up) else rows(op.c_out)
                op(h, y, B, T, ld, stream, self.WN_config.get('cond_padding_mode', 'zeros'))
                h = y
            if wn_up:                                                            # glow_ax.py:389-390 -> :362-373
                hT, hld = T, ld
                for tc in wn_up[k]:
                    h, hT, hld = tc(h, B, hT, hld, stream)
                self._to_latent_length(h, B, C2L, hT, hld, T_out, ld_out, frames[k],
                                       self._wn_tconv_factor != self.hop_length // self.n_group, stream, two_d=self.waveflow)
        return frames, ld_out, T_out

    # --------------------------------------------------------------------- the path ----
    def inverse(self, z, cond, speaker_ids=None, return_CPU=True):
        """efficient_model_ax.py:279-357: z [B, T] (noise, sigma applied), cond [B, n_mel(*2), frames].  ``waveflow=True``:
        WaveFlowCoupling + WN_2d (ctts_waveflow_inverse_f32 / _cond_f32); ``waveflow=False``: AffineCouplingBlock + the 1-D WN
        (ctts_wgax_inverse_f32, ctts_wgax_sep_inverse_f32 with separable in-layers, or ctts_wgax_inverse_f16 after
        ``set_compute_dtype(torch.float16)``)."""
        device = cond.device
        blob, ops = self._ensure_packed(device)
        lib = _lib.lib()
        half = self._compute_dtype == torch.float16
        if self.waveflow:
            cfg, ws_bytes, what = self.c_config(), lib.ctts_waveflow_workspace_bytes, "WaveFlow workspace query failed"
        else:
            cfg, what = self.c_config_1d(), "ax WaveGlow workspace query failed"
            ws_bytes = (lib.ctts_wgax_sep_workspace_bytes if self._sep1d else
                        lib.ctts_wgax_workspace_f16_bytes if half else lib.ctts_wgax_workspace_bytes)
        mel = cond.detach().float().contiguous()
        zz = z.detach().to(device=device, dtype=torch.float32).contiguous()
        B, T = zz.shape
        assert mel.shape[0] == B and mel.shape[1] == self.n_mel_channels * (2 if self.has_logvar_channels else 1)
        assert self.waveflow or T % self.n_group == 0, "z length is not a multiple of n_group"
        ws = self.workspace((device, B, T, self._compute_dtype), lambda: _lib.nbytes(ws_bytes, C.byref(cfg), B, T, what=what))
        audio = torch.empty(B, T, dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            stream = _lib.stream(device)
            if self._folded:
                _lib.check(lib.ctts_waveflow_inverse_f32(C.byref(cfg), _lib.ptr(blob), _lib.ptr(zz), _lib.ptr(mel),
                                                        _lib.ptr(audio), B, T, mel.shape[2], _lib.ptr(ws),
                                                        ws.numel() * 4, stream), "ctts_waveflow_inverse_f32")
            else:
                frames, ld, n_cond = self._cond_frames(ops, mel, speaker_ids, stream, out_steps=T // self.n_group)
                if self.waveflow:
                    _lib.check(lib.ctts_waveflow_inverse_cond_f32(C.byref(cfg), _lib.ptr(blob), _lib.ptr(zz), _lib.ptr(frames),
                                                                 ld, PAD, _lib.ptr(audio), B, T, n_cond, _lib.ptr(ws),
                                                                 ws.numel() * 4, stream), "ctts_waveflow_inverse_cond_f32")
                else:
                    name = ("ctts_wgax_sep_inverse_f32" if self._sep1d else
                            "ctts_wgax_inverse_f16" if half else "ctts_wgax_inverse_f32")
                    _lib.check(getattr(lib, name)(C.byref(cfg), _lib.ptr(blob), _lib.ptr(zz), _lib.ptr(frames), ld, PAD, n_cond,
                                                  _lib.ptr(audio), B, T, _lib.ptr(ws), ws.numel() * 4, stream), name)
            if self.vol_scaling:       # ax:342-344
                _lib.check(lib.ctts_vol_unscale_f32(_lib.ptr(audio), audio.numel(), stream), "ctts_vol_unscale_f32")
            if self.preempthasis:      # ax:351-355 (scipy lfilter on the host there; here on the device, in place)
                _lib.check(lib.ctts_deemphasis_f32(_lib.ptr(audio), _lib.ptr(audio), B, T, float(self.preempthasis),
                                                  stream), "ctts_deemphasis_f32")
        if return_CPU:
            audio = audio.cpu()
            if self.waveflow:
                # the copy synchronised the stream: a row-queue abort of THIS call is known now - raise instead of handing out
                # its NaN audio (a call that stays on the device reports it through the next call on this workspace: CTTS_E_ABORT)
                with torch.cuda.device(device):
                    _lib.check(lib.ctts_waveflow_abort_status(C.byref(cfg), B, T, _lib.ptr(ws), ws.numel() * 4, stream),
                               "WaveFlow.inverse")
        return audio, None

    def _drop_workspaces(self):
        """Forget the cached WaveFlow workspaces (another shape is coming) - but not an abort one of them still holds: a
        row-queue call that stayed on the device (``return_CPU=False``) reports a given-up wait through the workspace's status
        word, and dropping the workspace would drop the report.  Raises HipLibraryError (CTTS_E_ABORT) then."""
        old, self._ws = self._ws, {}
        if not self.waveflow:
            return
        lib = _lib.lib()
        cfg = self.c_config()
        for key, ws in old.items():
            if len(key) != 4:              # a forward workspace: the analysis pass never runs the row queue
                continue
            device, B, T, _ = key
            with torch.cuda.device(device):
                stream = _lib.stream(device)
                _lib.check(lib.ctts_waveflow_abort_status(C.byref(cfg), B, T, _lib.ptr(ws), ws.numel() * 4, stream),
                           "WaveFlow.inverse (an earlier call on a workspace that is being replaced)")

    def _prep_spect(self, spect, artifact_trimming):
        p = next(self.parameters())
        spect = spect.to(p.device, p.dtype)
        if spect.dim() == 2:
            spect = spect[None, ...]
        if artifact_trimming > 0:
            spect = F.pad(spect, (0, artifact_trimming), value=0.0)
        return spect

    @torch.no_grad()
    def infer(self, spect, speaker_ids=None, artifact_trimming=1, sigma=1., t_scaler=1.0, return_CPU=True):
        """efficient_model_ax.py:359-388."""
        input_dtype = spect.dtype
        spect = self._prep_spect(spect, artifact_trimming)
        batch_dim, _, steps = spect.shape
        samples = (steps - 1) * self.hop_length * t_scaler
        samples = int(samples - (samples % self.n_group))
        z = spect.new_empty((batch_dim, samples))
        if sigma > 0:
            z.normal_(std=sigma)
        else:
            z.zero_()
        audio, _ = self.inverse(z, spect, speaker_ids, return_CPU=return_CPU)
        if artifact_trimming > 0:
            audio = audio[:, :-artifact_trimming * self.hop_length]
        return audio.to(input_dtype)

    @torch.no_grad()
    def infer_from_noise(self, spect, z_scaled, speaker_ids=None, artifact_trimming=1, return_CPU=True):
        """Deterministic entry: ``infer`` (efficient_model_ax.py:359-388) with the latent it would draw at :376-378 given
        by the caller - ``z_scaled`` [B, (F + artifact_trimming - 1) * hop - remainder], sigma already applied."""
        input_dtype = spect.dtype
        spect = self._prep_spect(spect, artifact_trimming)
        samples = (spect.shape[2] - 1) * self.hop_length
        samples -= samples % self.n_group
        if tuple(z_scaled.shape) != (spect.shape[0], samples):
            raise ValueError(f"z_scaled is {tuple(z_scaled.shape)}, this mel needs {(spect.shape[0], samples)}")
        audio, _ = self.inverse(z_scaled, spect, speaker_ids, return_CPU=return_CPU)
        if artifact_trimming > 0:
            audio = audio[:, :-artifact_trimming * self.hop_length]
        return audio.to(input_dtype)

    # ------------------------------------------------------------- the analysis pass ----
    def _forward_refusals(self, audio):
        """Everything ``forward`` / ``nll`` refuse, by name and in this order, before anything is packed or launched."""
        if self.training and torch.is_grad_enabled():
            raise NotImplementedError("training direction is outside the inference hot path: no backward pass - "
                                      "WaveGlow.forward on the HIP path is the analysis pass only (call model.eval() or run "
                                      "it under torch.no_grad())")
        if not self.waveflow:
            raise NotImplementedError("waveflow=False: the 1-D ax core has no forward form on the HIP path (the analysis pass is "
                                      "built for waveflow=True)")
        if audio is None:
            raise ValueError("WaveGlow.forward needs the audio [B, T] or [B, 1, T] (efficient_model_ax.py:184); audio is None")
        if audio.dim() not in (2, 3) or (audio.dim() == 3 and audio.shape[1] != 1) or audio.shape[-1] == 0 \
                or audio.shape[-1] % self.n_group != 0:
            raise ValueError(f"audio of shape {tuple(audio.shape)}: forward needs [B, T] or [B, 1, T] with T a multiple of "
                             f"n_group = {self.n_group} (efficient_model_ax.py:225)")
        if self.vol_scaling:
            raise NotImplementedError("preceived_vol_scaling: the reference rewrites the caller's audio in place there "
                                      "(efficient_model_ax.py:198-200); not built")

    def _ensure_forward_packed(self, device):
        """-> (inverse blob, forward-mix blob or None, log|det W_k| [n_flows] per column as fp32 on the host).  Packed on the
        first forward call and kept while the inverse blob it was packed beside is the live one; ``infer`` alone never builds it."""
        blob, ops = self._ensure_packed(device)
        if self._fwd is None or self._fwd[0] is not blob:
            lib = _lib.lib()
            cfg = self.c_config()
            fwd, unit = None, []
            if self.channel_mixing == '1x1conv':
                nbytes = _lib.nbytes(lib.ctts_waveflow_forward_packed_bytes, C.byref(cfg), what="unsupported WaveFlow config")
                with torch.cuda.device(device):
                    stream = _lib.stream(device)
                    fwd = torch.zeros(nbytes // 4, dtype=torch.float32, device=device)
                    keep = []
                    for k in range(self.n_flows):
                        W = self.convinv[k].weight.detach().squeeze(-1).float()
                        unit.append(W.cpu().slogdet()[1])                       # efficient_modules.py:265: log|det|, host fp32
                        Wd = W.to(device).contiguous()
                        keep.append(Wd)
                        _lib.check(lib.ctts_waveflow_pack_forward_mix(C.byref(cfg), k, _lib.ptr(Wd), _lib.ptr(fwd), stream),
                                   f"ctts_waveflow_pack_forward_mix({k})")
                    torch.cuda.current_stream(device).synchronize()
                unit = torch.stack(unit)
            else:
                unit = None                                                    # PermuteHeight: L * const (efficient_modules.py:384, 397)
            self._fwd = (blob, fwd, unit)
        return self._fwd + (ops,)

    def _log_det_W(self, unit, L):
        """log_det_W_k of every flow as the reference takes it, fp32 on the host: ``L * slogdet(W_k)[1]`` (efficient_modules.py:265)
        or PermuteHeight's ``L * const`` with sigma = 1 (:384, :397; ax:165)."""
        if unit is not None:
            return (L * unit).float()
        const = -(0.5 * np.log(2 * np.pi) + np.log(1.0)) / self.n_flows
        return torch.tensor([L * const] * self.n_flows, dtype=torch.float32)

    def _forward_core(self, cond, audio, speaker_ids, want_log_s):
        """-> (z [B, T], log_s [B, S, L] or None, log_s_sum [B, L], sums float64 [B, n_flows], log_det_W [n_flows] fp32 host)."""
        self._forward_refusals(audio)
        if cond.dim() == 2:
            cond = cond[None, ...]
        device = cond.device
        blob, fwd, unit, ops = self._ensure_forward_packed(device)
        lib = _lib.lib()
        cfg = self.c_config()
        mel = cond.detach().float().contiguous()
        wave = audio.detach().to(device=device, dtype=torch.float32).reshape(audio.shape[0], -1).contiguous()
        B, T = wave.shape
        assert mel.shape[0] == B and mel.shape[1] == self.n_mel_channels * (2 if self.has_logvar_channels else 1)
        L = T // self.n_group
        nbytes = _lib.nbytes(lib.ctts_waveflow_forward_workspace_bytes, C.byref(cfg), B, T, what="WaveFlow forward workspace query failed")
        ws = self.workspace((device, B, T, "forward", nbytes), lambda: nbytes)
        n_rem, S = self.n_group, 0
        self._log_s_rows = []
        for k in range(self.n_flows):
            if k % self.n_early_every == 0 and k > 0:
                n_rem -= self.n_early_size
            self._log_s_rows.append(n_rem - 1)
            S += n_rem - 1
        z = torch.empty(B, T, dtype=torch.float32, device=device)
        log_s = torch.empty(B, S, L, dtype=torch.float32, device=device) if want_log_s else None
        log_s_sum = torch.empty(B, L, dtype=torch.float32, device=device)
        sums = torch.empty(B, self.n_flows, dtype=torch.float64, device=device)
        pre = float(self.preempthasis) if self.preempthasis else 0.0
        with torch.cuda.device(device):
            stream = _lib.stream(device)
            if self._folded:
                _lib.check(lib.ctts_waveflow_forward_f32(C.byref(cfg), _lib.ptr(blob), _lib.ptr(fwd), _lib.ptr(wave), _lib.ptr(mel),
                                                        pre, 1 if self.ignore_nan else 0, _lib.ptr(z), _lib.ptr(log_s),
                                                        _lib.ptr(log_s_sum), _lib.ptr(sums), B, T, mel.shape[2], _lib.ptr(ws),
                                                        ws.numel() * 4, stream), "ctts_waveflow_forward_f32")
            else:
                frames, ld, n_cond = self._cond_frames(ops, mel, speaker_ids, stream, out_steps=L)
                _lib.check(lib.ctts_waveflow_forward_cond_f32(C.byref(cfg), _lib.ptr(blob), _lib.ptr(fwd), _lib.ptr(wave),
                                                             _lib.ptr(frames), ld, PAD, pre, 1 if self.ignore_nan else 0,
                                                             _lib.ptr(z), _lib.ptr(log_s), _lib.ptr(log_s_sum), _lib.ptr(sums), B, T,
                                                             n_cond, _lib.ptr(ws), ws.numel() * 4, stream),
                           "ctts_waveflow_forward_cond_f32")
        return z, log_s, log_s_sum, sums, self._log_det_W(unit, L)

    def forward(self, cond, audio=None, speaker_ids=None, return_log_s=False):
        """``efficient_model_ax.WaveGlow.forward`` (ax:184-277) of a ``waveflow=True`` model without a gradient: cond
        [B, n_mel(*2), frames], audio [B, T] or [B, 1, T] (T a multiple of n_group) -> the reference's tuple ``(z [B, T],
        logdet [B], logdet_w_sum [], log_s_sum [B, L])`` as fp32 device tensors; the stream is not synchronised.  ``z`` has the
        early outputs first, in peel order: the latent ``inverse`` / ``infer_from_noise`` take.  ``log_det_W_k`` is taken on the
        host in fp32 as the reference takes it; ``logdet = sum_k (log_det_W_k + sum log_s_k)`` from the device's fp64 sums, rounded
        once.  ``return_log_s=True`` appends the per-flow ``log_s`` [B, n_rem_k - 1, L] as views of one buffer.

        Models whose layers are the fused C = 64 GTU dense form (BASELINE config 4) run one launch per WN layer over all rows; every
        other model - and a fused one under ``set_f32_gemm_mode("bf16x3" | "bf16x6")`` or ``CTTS_WF_FWD_ROWWISE=1`` - runs row by
        row through the launches of ``inverse``."""
        z, log_s, log_s_sum, sums, ldw = self._forward_core(cond, audio, speaker_ids, want_log_s=return_log_s)
        ldw_dev = ldw.to(device=z.device, dtype=torch.float64)
        logdet = (ldw_dev[None, :] + sums).sum(dim=1).float()
        out = (z, logdet, ldw.sum().to(z.device), log_s_sum)
        if return_log_s:
            views, off = [], 0
            for n in self._log_s_rows:
                views.append(log_s[:, off:off + n])
                off += n
            out = out + (views,)
        return out

    def nll(self, cond, audio, speaker_ids=None, sigma=1.0):
        """``efficient_loss.WaveGlowLoss(sigma)`` (:33-44) of ``forward``'s output from the fp64 sums (``log_s`` is not
        materialised): ``{"loss": 0-dim fp32 tensor, "per_item": [B] float64}`` with item b's own
        ``(sum z^2 / 2 sigma^2 - sum_k (log_det_W_k + sum log_s_k)) / T``, whose mean is the loss."""
        z, _, _, sums, ldw = self._forward_core(cond, audio, speaker_ids, want_log_s=False)
        z2 = z.double().pow(2).sum(dim=1)
        logdet = (ldw.to(device=z.device, dtype=torch.float64)[None, :] + sums).sum(dim=1)
        per_item = (z2 / (2.0 * sigma * sigma) - logdet) / z.shape[1]
        return {"loss": per_item.mean().float(), "per_item": per_item}


class WaveFlowLoss(nn.Module):
    """``efficient_loss.WaveGlowLoss`` (:24-44) on ``WaveGlow.forward``'s tuple ``(z, logdet, logdet_w_sum, log_s_sum)``:
    ``mean_b((sum z_b^2 / 2 sigma^2 - logdet_b) / T)``."""

    def __init__(self, sigma=1., elementwise_mean=True):
        super().__init__()
        self.sigma2 = sigma ** 2
        self.sigma2_2 = self.sigma2 * 2
        self.mean = elementwise_mean

    def forward(self, model_outputs):
        z, logdet = model_outputs[0].float(), model_outputs[1].float()
        loss = z.pow(2).sum(1) / self.sigma2_2
        loss = loss - logdet
        loss = loss / z.size(1)
        return loss.mean()
