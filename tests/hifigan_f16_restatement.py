"""Restatement of the HiFi-GAN generator's HALF-STORAGE arithmetic (helper of test_hifigan_f16.py; TEST INFRASTRUCTURE ONLY -
the product path is ``cookietts_amd.hifigan`` with ``set_compute_dtype(torch.float16)`` over csrc/hifigan_f16.hip).

Written from the spec like ``hifigan_restatement.py`` (plain ``torch.nn.functional`` on folded weights, no reference code),
with the rounding points the library documents at ``ctts_hifigan_forward_f16``.  ``q`` = one rounding to the 16-bit format
(round-to-nearest-even, overflow to infinity); everything between two ``q`` is fp32:

    W = q(g * v / ||v||) from the fp32 parameters, biases fp32;  m = q(mel)
    lrelu(x, s) = x where x >= 0, else q(x * s)        (x holds 16-bit values, s is the fp32 slope: F.leaky_relu on a half tensor)
    x = q(conv1d(m, Wpre) + b)
    for each stage i:  x = q(conv_transpose1d(lrelu(x, 0.1), Wup_i) + b)
                       per resblock j, r = x:
                           ResBlock1, m = 0..2:  t = q(c1_m(lrelu(r, 0.1)) + b);  v = c2_m(lrelu(t, 0.1)) + b + r
                           ResBlock2, m = 0..1:                                    v = c_m(lrelu(r, 0.1)) + b + r
                           r = q(v) for every step but the last; the last step's v stays fp32 and feeds the sum:
                           xs = q(v) (j = 0),  q(xs + v) (0 < j < n_k - 1),  q((xs + v) / n_k) (j = n_k - 1)
                       x = xs
    y = tanh(conv1d(lrelu(x, 0.01), Wpost) + b)         fp32, not rounded

Rounding point 4 - the sum over a stage's resblocks - is ALL HALF here: every partial sum is a stored 16-bit value (one
rounding each, taken from the unrounded fp32 ``v``), no fp32 running sum exists.  That is also what the reference does in its
half mode (``xs += resblock(x)`` on half tensors), and it keeps the workspace at half the fp32 path's bytes.

``fmt`` = "f16" (IEEE half: what the library runs) or "bf16" (the same points with an 8-bit mantissa: the control that tells
a bf16 implementation from an f16 one).  The convolutions run in fp32 on the 16-bit values, i.e. exact products and an fp32
sum as on the MFMA; only the order of that sum differs from the kernel's.
"""
import numpy as np
import torch
import torch.nn.functional as F

from hifigan_restatement import folded_weights

FORMATS = {"f16": torch.float16, "bf16": torch.bfloat16}


def round_to(v, fmt):
    """One rounding of an fp32 tensor to ``fmt``, returned as fp32."""
    return v.to(FORMATS[fmt]).to(torch.float32)


def generator(cfg, w, mel, fmt="f16", final_slope=0.01):
    """``w``: ``hifigan_restatement.folded_weights(..., torch.float32)``; ``mel`` [B, num_mels, T] fp32 -> fp32 [B, 1, T prod(u)]."""
    def q(v):
        return round_to(v, fmt)

    def lrelu(x, s):
        return torch.where(x >= 0, x, q(x * torch.tensor(s, dtype=torch.float32, device=x.device)))

    def wb(name):
        weight, bias = w[name]
        return q(weight.float()), bias.float()

    n_k = len(cfg["resblock_kernel_sizes"])
    x = q(F.conv1d(q(mel.float()), *wb("conv_pre"), padding=3))
    for i, (u, ku) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        x = q(F.conv_transpose1d(lrelu(x, 0.1), *wb(f"ups.{i}"), stride=u, padding=(ku - u) // 2))
        xs = None
        for j, (k, dil) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            p = f"resblocks.{i * n_k + j}"
            r = x
            steps = 3 if cfg["resblock"] == "1" else 2
            for m in range(steps):
                d = dil[m]
                if cfg["resblock"] == "1":
                    t = q(F.conv1d(lrelu(r, 0.1), *wb(f"{p}.convs1.{m}"), dilation=d, padding=(k * d - d) // 2))
                    v = F.conv1d(lrelu(t, 0.1), *wb(f"{p}.convs2.{m}"), padding=(k - 1) // 2) + r
                else:
                    v = F.conv1d(lrelu(r, 0.1), *wb(f"{p}.convs.{m}"), dilation=d, padding=(k * d - d) // 2) + r
                if m < steps - 1:
                    r = q(v)
            s = v if xs is None else xs + v
            if j == n_k - 1:
                s = s / torch.tensor(float(n_k), dtype=torch.float32, device=s.device)
            xs = q(s)
        x = xs
    return torch.tanh(F.conv1d(lrelu(x, final_slope), *wb("conv_post"), padding=3))


def generator_np(cfg, sd, mel, fmt="f16", final_slope=0.01):
    """numpy in, numpy out, on the CPU."""
    with torch.no_grad():
        w = folded_weights(cfg, sd, torch.float32)
        return generator(cfg, w, torch.from_numpy(np.ascontiguousarray(mel, dtype=np.float32)), fmt, final_slope).numpy()


def generator_bytes(cfg, frames, esz=2):
    """Algorithmic bytes one utterance of ``frames`` mel frames moves through memory with ``esz``-byte activations, from the
    shapes as ``hifigan_restatement.generator_macs`` counts its products: every conv reads its input tensor once and writes its
    output once, a residual conv reads the residual, the last conv of a resblock read-modify-writes the stage's sum
    (the first resblock of a stage only writes it).  Weights and halos are not counted."""
    C0, n_k = cfg["upsample_initial_channel"], len(cfg["resblock_kernel_sizes"])
    L = frames
    total = cfg["num_mels"] * L * 4 + C0 * L * esz                   # conv_pre: fp32 mel in
    ch = C0
    for u in cfg["upsample_rates"]:
        total += ch * L * esz                                          # ups reads
        ch //= 2
        L *= u
        t = ch * L * esz                                               # one C-row tensor of the stage
        total += t                                                     # ups writes
        for j in range(n_k):
            if cfg["resblock"] == "1":
                per_step = 2 * t + 3 * t                               # c1: read, write; c2: read, residual, write
                steps = 3
            else:
                per_step = 3 * t
                steps = 2
            total += steps * per_step + (0 if j == 0 else t)           # the sum's read-modify-write replaces the last write
    return total + ch * L * esz + L * 4                                # conv_post: read, fp32 waveform out
