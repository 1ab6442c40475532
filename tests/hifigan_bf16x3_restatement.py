"""Restatement of the HiFi-GAN generator's SPLIT-BF16 arithmetic (helper of test_hifigan_bf16x3.py; TEST INFRASTRUCTURE ONLY -
the product path is ``cookietts_amd.hifigan`` with ``set_f32_gemm_mode("bf16x3")`` over csrc/hifigan_bf16x3.hip).

Written from the contract at ``ctts_hifigan_forward_bf16x3``, not from the kernel: it is ``hifigan_restatement.generator``
with every conv replaced by three float64 convs on the split operands and every stored activation rounded to fp32.

    split(v) = (hi, lo),  hi = bf16_rne(v),  lo = bf16_rne(v - hi)                 (v fp32; hi, lo held as fp32 values)
    W = g * v / ||v|| folded in fp32, split once; biases fp32
    lrelu(x, s) = x where x >= 0, else x * s in fp32                               (then split: the activation operand)
    conv(x, W) = conv64(x_hi, W_hi) + conv64(x_hi, W_lo) + conv64(x_lo, W_hi) + b  (float64 sums; no lo * lo term)
    stored tensors (conv_pre / ups outputs, c1 outputs, residual states, the stage's running sum) are rounded to fp32

``terms`` names the products that are summed - ``"hh"`` = W_hi x_hi, ``"lh"`` = W_lo x_hi, ``"hl"`` = W_hi x_lo - so that a test
can plant the faults it must tell apart (a dropped cross term, hi * hi only).
"""
import numpy as np
import torch
import torch.nn.functional as F

from hifigan_restatement import folded_weights

TERMS = ("hh", "lh", "hl")


def split(v):
    """fp32 tensor -> (hi, lo) as float64 tensors holding bf16 values."""
    v = v.float()
    hi = v.to(torch.bfloat16).to(torch.float32)
    lo = (v - hi).to(torch.bfloat16).to(torch.float32)
    return hi.double(), lo.double()


def f32(v):
    return v.to(torch.float32)


def generator(cfg, w, mel, terms=TERMS, final_slope=0.01):
    """``w``: ``hifigan_restatement.folded_weights(..., torch.float32)``; ``mel`` [B, num_mels, T] fp32 -> fp32 [B, 1, T prod(u)]."""
    assert set(terms) <= set(TERMS)

    def lrelu(x, s):
        return torch.where(x >= 0, x, x * torch.tensor(s, dtype=torch.float32))

    def conv(fn, x, name, **kw):
        """float64 result of the split products of the fp32 activation ``x`` with the layer's weights, bias added."""
        weight, bias = w[name]
        xh, xl = split(x)
        wh, wl = split(weight)
        out = None
        for t, (a, b) in (("hh", (xh, wh)), ("lh", (xh, wl)), ("hl", (xl, wh))):
            if t in terms:
                y = fn(a, b, None, **kw)
                out = y if out is None else out + y
        return out + bias.double().view(1, -1, 1)

    n_k = len(cfg["resblock_kernel_sizes"])
    x = f32(conv(F.conv1d, mel.float(), "conv_pre", padding=3))
    for i, (u, ku) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        x = f32(conv(F.conv_transpose1d, lrelu(x, 0.1), f"ups.{i}", stride=u, padding=(ku - u) // 2))
        xs = None
        for j, (k, dil) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            p = f"resblocks.{i * n_k + j}"
            r = x
            steps = 3 if cfg["resblock"] == "1" else 2
            for m in range(steps):
                d = dil[m]
                if cfg["resblock"] == "1":
                    t = f32(conv(F.conv1d, lrelu(r, 0.1), f"{p}.convs1.{m}", dilation=d, padding=(k * d - d) // 2))
                    v = conv(F.conv1d, lrelu(t, 0.1), f"{p}.convs2.{m}", padding=(k - 1) // 2) + r.double()
                else:
                    v = conv(F.conv1d, lrelu(r, 0.1), f"{p}.convs.{m}", dilation=d, padding=(k * d - d) // 2) + r.double()
                r = f32(v)
            s = r.double() if xs is None else xs.double() + r.double()
            if j == n_k - 1:
                s = s / n_k
            xs = f32(s)
        x = xs
    return f32(torch.tanh(conv(F.conv1d, lrelu(x, final_slope), "conv_post", padding=3)))


def generator_np(cfg, sd, mel, terms=TERMS, final_slope=0.01):
    """numpy in, numpy out, on the CPU."""
    with torch.no_grad():
        w = folded_weights(cfg, sd, torch.float32)
        return generator(cfg, w, torch.from_numpy(np.ascontiguousarray(mel, dtype=np.float32)), terms, final_slope).numpy()
