#!/usr/bin/env python3
"""sha256 of the packed blobs (``_ensure_packed`` / ``_ops``) and of one deterministic call per model family and arithmetic mode:
the check of a host-only change, which cannot move a bit.  Run it in two checkouts and diff the listings.
usage: host_hashes.py TREE_ROOT   (the checkout whose ``cookietts_amd`` is imported; ``.`` for this one)"""
import hashlib
import os
import sys

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import numpy as np
import torch

import cookietts_amd
from cookietts_amd import synthetic, WaveGlow, WaveFlow, HiFiGANGenerator, Tacotron2, TacotronSTFT

assert os.path.dirname(os.path.dirname(os.path.abspath(cookietts_amd.__file__))) == root, cookietts_amd.__file__
dev = torch.device("cuda", 0)


def sha(*ts):
    d = hashlib.sha256()
    for t in ts:
        if t is None:
            d.update(b"none")
        else:
            d.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes() if t.dtype != torch.uint8 else t.cpu().numpy().tobytes())
    return d.hexdigest()


def out(name, what, *ts):
    print(f"{name:44s} {what:8s} {sha(*ts)}", flush=True)


def flat(x):
    if x is None:
        return []
    if torch.is_tensor(x):
        return [x]
    if isinstance(x, (list, tuple)):
        return [t for y in x for t in flat(y)]
    if isinstance(x, dict):
        return [t for k in sorted(x) for t in flat(x[k])]
    if hasattr(x, "blob"):
        return [x.blob]
    if hasattr(x, "ops"):
        return flat(x.ops)
    return []


# glow.py WaveGlow toy
cfg = synthetic.WAVEGLOW_CONFIGS["toy"]
mel = torch.from_numpy(synthetic.synthetic_mel(2, 11, seed=5)).to(dev)
z = torch.from_numpy(synthetic.synthetic_noise(2, cfg["n_group"], 11 * cfg["hop_length"] // cfg["n_group"], seed=6) * np.float32(0.6)).to(dev)
for mode in ("fp32", "bf16x3", "bfloat16", "float16"):
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(synthetic.waveglow_state_dict(cfg, seed=42)))
    m = m.to(dev).eval()
    if mode != "fp32":
        m.set_compute_dtype({"bf16x3": "bf16x3", "bfloat16": torch.bfloat16, "float16": torch.float16}[mode])
    out(f"waveglow/toy/{mode}", "packed", *m._ensure_packed(dev))
    out(f"waveglow/toy/{mode}", "output", m.infer_from_noise(mel, z))

# ax WaveGlow: 2-D toy, 1-D notebook (toy and full size)
for table, make, key in ((synthetic.WAVEFLOW_CONFIGS, synthetic.waveflow_state_dict, "toy"),
                         (synthetic.WAVEGLOW_AX_CONFIGS, synthetic.waveglow_ax_state_dict, "notebook_toy"),
                         (synthetic.WAVEGLOW_AX_CONFIGS, synthetic.waveglow_ax_state_dict, "notebook")):
    cfg = table[key]
    n_mel = cfg["n_mel_channels"] * (2 if cfg.get("use_logvar_channels") else 1)
    frames = 9
    mel = torch.from_numpy(synthetic.synthetic_mel(2, frames, n_mel=n_mel, seed=7)).to(dev)
    samples = frames * cfg["hop_length"]
    samples -= samples % cfg["n_group"]
    zz = torch.from_numpy(np.random.default_rng(8).standard_normal((2, samples)).astype(np.float32) * np.float32(0.6)).to(dev)
    for mode in ("fp32", "float16"):
        m = WaveFlow(**cfg)
        m.load_state_dict(synthetic.to_torch(make(cfg, seed=42)))
        m = m.to(dev).eval()
        name = f"ax/{'waveflow' if cfg.get('waveflow', True) else 'wgax'}/{key}/{mode}"
        if mode == "float16":
            try:
                m.set_compute_dtype(torch.float16)
            except NotImplementedError as e:
                print(f"{name:44s} refused  {type(e).__name__}", flush=True)
                continue
        ids = torch.zeros(2, dtype=torch.int64, device=dev) if m.multispeaker else None
        blob, ops = m._ensure_packed(dev)
        out(name, "packed", blob, *flat(ops))
        out(name, "output", m.infer_from_noise(mel, zz, speaker_ids=ids, return_CPU=False))

# HiFi-GAN
for key, T in (("toy_rb1", 13), ("v1", 21)):
    cfg = synthetic.HIFIGAN_CONFIGS[key]
    mel = torch.from_numpy(synthetic.synthetic_mel(2, T, n_mel=cfg["num_mels"], seed=9)).to(dev)
    for mode in ("fp32", "float16"):
        m = HiFiGANGenerator(cfg)
        m.load_state_dict(synthetic.to_torch(synthetic.hifigan_state_dict(cfg, seed=42)))
        m = m.to(dev).eval()
        if mode == "float16":
            m.set_compute_dtype(torch.float16)
        out(f"hifigan/{key}/{mode}", "packed", m._ensure_packed(dev))
        out(f"hifigan/{key}/{mode}", "output", m(mel))

# Tacotron2
hp = synthetic.tacotron_hparams()
m = Tacotron2(hp)
m.load_state_dict(synthetic.to_torch(synthetic.tacotron_state_dict(hp, seed=1234)))
m = m.to(dev).eval()
for B in (4, 16):
    T, steps = 40, 24
    rng = np.random.default_rng(100 + B)
    text = torch.from_numpy(rng.integers(1, 179, size=(B, T))).to(dev)
    lens = torch.from_numpy(np.sort(rng.integers(20, T + 1, size=B))[::-1].copy()).to(dev)
    lens[0] = T
    spk = torch.arange(B).to(dev)
    tm = torch.from_numpy(rng.standard_normal((B, 2304)).astype(np.float32)).to(dev)
    masks = synthetic.prenet_dropout_masks(steps, B, hp.prenet_dim, seed=200 + B)
    o = m.inference(text, lens, spk, tm, keep_masks=masks, fixed_steps=steps)
    out(f"tacotron2/B{B}", "packed", m.decoder._ensure_packed(dev), *flat(m.postnet._ops(dev)), *flat(m.encoder._ops(dev)))
    out(f"tacotron2/B{B}", "output", o["pred_mel_postnet"], o["pred_gate"], o["alignments"], o["pred_sylps"])
    out(f"tacotron2/B{B}", "form", torch.tensor([len(next(iter(m.decoder._ws.values())))]))

# TacotronSTFT
stft = TacotronSTFT().to(dev)
y = torch.from_numpy(np.random.default_rng(10).uniform(-0.9, 0.9, size=(2, 8192)).astype(np.float32)).to(dev)
mel = stft.mel_spectrogram(y)
out("stft/mel_spectrogram", "packed", *[stft.stft_fn._packed[k] for k in sorted(stft.stft_fn._packed, key=str)])
out("stft/mel_spectrogram", "output", mel)
torch.cuda.synchronize()
print("done", flush=True)
