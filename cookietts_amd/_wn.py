"""Weight-normed conv parameters as checkpoints store them, and their fold into a dense weight on the device."""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import _lib


class WNConv(nn.Module):
    """``nn.utils.weight_norm(conv)`` as stored in checkpoints: ``bias``, ``weight_g`` [out, 1, ...], ``weight_v`` of ``shape``
    = [out, in, *kernel] (any kernel rank), drawn like the conv's default init (``weight_v`` first, then the bias)."""

    def __init__(self, shape):
        super().__init__()
        fan_in = 1
        for d in shape[1:]:
            fan_in *= d
        v = torch.empty(*shape)
        nn.init.kaiming_uniform_(v, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(fan_in)
        self.bias = nn.Parameter(torch.empty(shape[0]).uniform_(-bound, bound))
        self.weight_g = nn.Parameter(v.flatten(1).norm(dim=1).view(shape[0], *([1] * (len(shape) - 1))).clone())
        self.weight_v = nn.Parameter(v)

    def remove_weight_norm(self):
        if getattr(self, "weight_v", None) is not None:
            v, g = self.weight_v.data, self.weight_g.data
            w = v * (g / v.flatten(1).norm(dim=1).view(g.shape))
            del self._parameters["weight_g"], self._parameters["weight_v"]
            self.weight = nn.Parameter(w)


def folded_weight(layer, stream, keep):
    """fp32 contiguous dense weight of ``layer`` on its device: ``g * v / ||v||`` through ``ctts_fold_weightnorm_f32``, or the
    plain ``weight`` once weight norm is removed.  The tensors the launch reads are parked in ``keep``."""
    if getattr(layer, 'weight_v', None) is not None:
        v = layer.weight_v.detach().float().contiguous()
        g = layer.weight_g.detach().float().contiguous()
        w = torch.empty_like(v)
        _lib.check(_lib.lib().ctts_fold_weightnorm_f32(_lib.ptr(v), _lib.ptr(g), _lib.ptr(w), v.shape[0], v[0].numel(), stream),
                   "ctts_fold_weightnorm_f32")
        keep += [v, g, w]
        return w
    w = layer.weight.detach().float().contiguous()
    keep.append(w)
    return w
