"""Reduced-precision restatement of the 1-D ax WaveGlow (helper of test_waveglow_ax_f16.py, TEST INFRASTRUCTURE ONLY).

``oracle.waveglow_ax_oracle`` with the rounding points of the half-storage path (``ctts_wgax_inverse_f16``) put in,
everything else the fp32 oracle's own code.  A rounding point is one round-to-nearest-even to the 16-bit format:

* in-layer and res/skip weights, once (the packed weights);
* ``x`` after ``start`` and after every ``x + res``;
* the gated activations;
* the skip sum after every layer's accumulation (layer 0 stores its skip rows).

fp32 everywhere else: ``start`` / ``end`` weights, every bias, products and sums inside a contraction, the conditioning
rows, the coupling, the mixing.  ``fmt`` = "f16" (IEEE half: what the library runs) or "bf16" (the same points with 8-bit
significands: what half storage is NOT - the tests use it to show that the restatement rounds at all, and by how much a
format with fewer bits misses the bound).  Reads nothing but its arguments.
"""
from contextlib import contextmanager

import numpy as np

from oracle import waveglow_ax_oracle as ao
from oracle.waveflow_oracle import F32, _shift, _w, activation, conv1d_same, gated_unit, wn_upsample


def round_to(v, fmt):
    v = np.ascontiguousarray(v, dtype=F32)
    if fmt == "f16":
        with np.errstate(over="ignore"):
            return v.astype(np.float16).astype(F32)
    assert fmt == "bf16", fmt
    u = v.view(np.uint32)
    r = ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)).view(F32)
    return np.where(np.isfinite(v), r, v).astype(F32)


def wn1d_rounded(fmt):
    """``ao.wn1d`` (glow_ax.py:375-418) with the rounding points above."""
    def r(v):
        return round_to(v, fmt)

    def wn1d(sd, p, wn, a0, frames, speaker_ids, L, upsample_factor=None):
        C, n_layers = wn["n_channels"], wn["n_layers"]
        ks = wn.get("kernel_size_w") or wn.get("kernel_size")
        x = r(np.matmul(_w(sd, p + ".start")[:, :, 0], a0) + sd[p + ".start.bias"][None, :, None])
        spect = frames
        if wn.get("speaker_embed_dim", 0) and speaker_ids is not None:
            emb = sd[p + ".speaker_embed.weight"][np.asarray(speaker_ids)]
            spect = np.concatenate([spect, np.repeat(emb[:, :, None], spect.shape[2], axis=2)], axis=1)
        act = activation(wn.get("cond_activation_func", 'none'), wn.get("negative_slope"))
        for l in range(wn["cond_layers"]):
            spect = conv1d_same(spect, _w(sd, f"{p}.cond_layers.{l}"), sd[f"{p}.cond_layers.{l}.bias"],
                                wn.get("cond_padding_mode", 'zeros'))
            if act is not None and (wn.get("cond_out_activation_func", True) or l != wn["cond_layers"] - 1):
                spect = act(spect).astype(F32)
        cond = spect if upsample_factor is None else wn_upsample(sd, p, wn, spect, L, upsample_factor, False)
        out = None
        for i in range(n_layers):
            dl = wn.get("n_layers_dilations_w")
            d = 2 ** i if dl is None else (dl if isinstance(dl, int) else dl[i])
            w = r(_w(sd, f"{p}.in_layers.{i}"))
            u = sd[f"{p}.in_layers.{i}.bias"][None, :, None] + np.zeros((x.shape[0], 2 * C, L), F32)
            for t in range(ks):
                u = u + np.matmul(np.ascontiguousarray(w[:, :, t]), _shift(x, (t - ks // 2) * d))
            u = (u.astype(F32) + cond[:, 2 * C * i:2 * C * (i + 1)]).astype(F32)
            g = r(gated_unit(wn.get("gated_unit", 'GTU'), u, C))
            if wn.get("res_skip", True):
                rs = (np.matmul(r(_w(sd, f"{p}.res_skip_layers.{i}"))[:, :, 0], g)
                      + sd[f"{p}.res_skip_layers.{i}.bias"][None, :, None]).astype(F32)
            else:
                rs = g
            if i < n_layers - 1 and not wn.get("merge_res_skip", False) and wn.get("res_skip", True):
                x = r(x + rs[:, :C])
                out = r(rs[:, C:]) if out is None else r(out + rs[:, C:])
            else:
                out = r(rs) if out is None else r(out + rs)
        e = (np.matmul(sd[p + ".end.weight"][:, :, 0], out) + sd[p + ".end.bias"][None, :, None]).astype(F32)
        h = e.shape[1] // 2
        return e[:, :h], e[:, h:]
    return wn1d


@contextmanager
def _rounded_wn(fmt):
    saved = ao.wn1d
    ao.wn1d = wn1d_rounded(fmt)       # waveglow_ax_inverse resolves wn1d in its module at call time
    try:
        yield
    finally:
        ao.wn1d = saved


def inverse(sd, cfg, z, mel, speaker_ids=None, fmt="f16"):
    """``ao.waveglow_ax_inverse`` with every WN replaced by its rounded restatement."""
    with _rounded_wn(fmt):
        return ao.waveglow_ax_inverse(sd, cfg, z, mel, speaker_ids)


def with_gtu(cfg):
    """The same model with the GTU unit (the gated units have no parameters: the state dict is unchanged)."""
    return dict(cfg, WN_config=dict(cfg["WN_config"], gated_unit='GTU'))
