"""Restatement of the HiFi-GAN generator's arithmetic (helper of test_hifigan.py and of the ``hifigan`` bench row; TEST
INFRASTRUCTURE ONLY - the product path is ``cookietts_amd.hifigan`` over csrc/hifigan.hip).

Written from the spec, not from the reference's classes: folded weights (``w = g * v / ||v||``, the norm over every dim but
dim 0 - for a ConvTranspose1d dim 0 is the INPUT channel) and plain ``torch.nn.functional`` calls:

    x = conv1d(mel, Wpre, pad 3) + b
    for each stage i:  x = conv_transpose1d(lrelu(x, 0.1), Wup_i, stride u_i, padding (ku_i - u_i) // 2) + b
                       x = sum_j resblock_{i n_k + j}(x) / n_k
    y = tanh(conv1d(lrelu(x, 0.01), Wpost, pad 3) + b)          (0.01: the default slope of F.leaky_relu)
    ResBlock1:  x = x + c2_m(lrelu(c1_m(lrelu(x, 0.1)), 0.1)), m = 0..2 (c1_m dilated by d_m, c2_m not)
    ResBlock2:  x = x + c_m(lrelu(x, 0.1)), m = 0..1

In fp64 on the CPU it is what the goldens are checked against without a GPU; in fp32 on the GPU (``dtype=torch.float32``,
tensors on the device) it is the "what a user gets today through PyTorch-ROCm" arm of the bench row.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_cases():
    """Names of the hifigan_*.npz fixtures, the ``full_length`` one last."""
    names = sorted(f[len("hifigan_"):-len(".npz")] for f in os.listdir(GOLDEN)
                   if f.startswith("hifigan_") and f.endswith(".npz") and not f.endswith(".mel.npz"))
    return sorted(names, key=lambda n: "full_length" in n)


def load_case(name):
    """One fixture as a dict (the mel of a case too large for one committed file lives in ``hifigan_<name>.mel.npz``)."""
    z = dict(np.load(os.path.join(GOLDEN, f"hifigan_{name}.npz")))
    if "mel" not in z:
        z["mel"] = np.load(os.path.join(GOLDEN, f"hifigan_{name}.mel.npz"))["mel"]
    return z


def fold(sd, prefix, dtype=torch.float64, device=None):
    """(weight, bias) of one conv from a state dict with weight-norm keys (or an already folded ``weight``)."""
    def t(v):
        v = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v.detach()
        return v.to(device=device, dtype=dtype)
    b = t(sd[prefix + ".bias"])
    if prefix + ".weight" in sd:
        return t(sd[prefix + ".weight"]), b
    v, g = t(sd[prefix + ".weight_v"]), t(sd[prefix + ".weight_g"])
    norm = v.flatten(1).norm(dim=1).view(g.shape)
    return v * (g / norm), b


def folded_weights(cfg, sd, dtype=torch.float64, device=None):
    """prefix -> (weight, bias) for every conv of the generator."""
    prefixes = sorted({k.rsplit(".", 1)[0] for k in sd})
    return {p: fold(sd, p, dtype, device) for p in prefixes}


def generator(cfg, w, mel, final_slope=0.01):
    """``w``: ``folded_weights`` output; ``mel`` [B, num_mels, T] tensor of the weights' dtype/device -> [B, 1, T prod(u)]."""
    n_k = len(cfg["resblock_kernel_sizes"])
    x = F.conv1d(mel, *w["conv_pre"], padding=3)
    for i, (u, ku) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        x = F.conv_transpose1d(F.leaky_relu(x, 0.1), *w[f"ups.{i}"], stride=u, padding=(ku - u) // 2)
        xs = None
        for j, (k, dil) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            p = f"resblocks.{i * n_k + j}"
            r = x
            if cfg["resblock"] == "1":
                for m in range(3):
                    d = dil[m]
                    t = F.conv1d(F.leaky_relu(r, 0.1), *w[f"{p}.convs1.{m}"], dilation=d, padding=(k * d - d) // 2)
                    t = F.conv1d(F.leaky_relu(t, 0.1), *w[f"{p}.convs2.{m}"], padding=(k - 1) // 2)
                    r = t + r
            else:
                for m in range(2):
                    d = dil[m]
                    r = F.conv1d(F.leaky_relu(r, 0.1), *w[f"{p}.convs.{m}"], dilation=d, padding=(k * d - d) // 2) + r
            xs = r if xs is None else xs + r
        x = xs / n_k
    return torch.tanh(F.conv1d(F.leaky_relu(x, final_slope), *w["conv_post"], padding=3))


def generator_np(cfg, sd, mel, dtype=torch.float64, final_slope=0.01):
    """numpy in, numpy out, on the CPU."""
    with torch.no_grad():
        w = folded_weights(cfg, sd, dtype)
        return generator(cfg, w, torch.from_numpy(np.ascontiguousarray(mel)).to(dtype), final_slope).numpy()


def generator_macs(cfg, frames):
    """Multiply-accumulates of one utterance of ``frames`` mel frames, from the shapes."""
    C0, n_k = cfg["upsample_initial_channel"], len(cfg["resblock_kernel_sizes"])
    L = frames
    macs = cfg["num_mels"] * C0 * 7 * L
    ch = C0
    for u, ku in zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"]):
        macs += ch * (ch // 2) * ku * L          # every input sample meets every tap once
        ch //= 2
        L *= u
        convs = (2 * 3) if cfg["resblock"] == "1" else 2
        macs += sum(ch * ch * k * convs for k in cfg["resblock_kernel_sizes"]) * L
    return macs + ch * 7 * L
