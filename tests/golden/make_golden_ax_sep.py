#!/usr/bin/env python3
"""Generate tests/golden/waveglow_ax_sep_*.npz by RUNNING THE REFERENCE ITSELF: efficient_model_ax.WaveGlow with
``waveflow=False`` and ``WN_config['seperable_conv']`` (glow_ax.py:337-348: depthwise + pointwise in-layers).

Run where the reference tree is checked out (it is not on the GPU box):

    COOKIETTS_REFERENCE=<path of the reference tree> python tests/golden/make_golden_ax_sep.py [key ...]

The reference is imported with the stand-ins of ``make_golden.py`` (``_ref_waveflow``: librosa / iso226 stubs, np.product), the
recipe weights of ``cookietts_amd.synthetic.waveglow_ax_state_dict`` go in through its own ``load_state_dict(strict=True)``, and
its own ``infer`` and ``inverse`` run with the noise replayed from the seed.  Data only, the fields of ``waveglow_ax_*.npz``:
config_key, seed, sigma, mel, z, audio, inverse_full (, speaker_ids).
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if os.environ.get("COOKIETTS_REFERENCE"):
    sys.path.insert(0, os.environ["COOKIETTS_REFERENCE"])

from make_golden import _ref_waveflow  # noqa: E402  (puts the repository root on sys.path)
from cookietts_amd import synthetic  # noqa: E402

MAX_FILE = 1 << 20
# key, batch, frames, sigma, seed
CASES = [("sep_toy", 2, 13, 0.8, 81), ("sep_k7_dil_c96", 2, 11, 0.8, 82), ("sep_k13_merge_c160", 1, 14, 0.8, 83),
         ("sep_deep", 1, 13, 0.8, 84), ("sep_k1", 1, 4, 0.8, 85), ("sep_notebook_toy", 2, 6, 0.8, 86)]


def main():
    torch.set_num_threads(8)
    only = sys.argv[1:]
    for key, B, F, sigma, seed in CASES:
        if only and key not in only:
            continue
        cfg = synthetic.WAVEGLOW_AX_SEP_CONFIGS[key]
        sd = synthetic.waveglow_ax_state_dict(cfg, seed=seed)
        model = _ref_waveflow(copy.deepcopy(cfg), sd)
        sep = cfg["WN_config"]["kernel_size_w"] != 1
        assert isinstance(model.WN[0].WN.in_layers[0], torch.nn.Sequential) == sep
        mel = synthetic.synthetic_mel(B, F, cfg["n_mel_channels"], seed=seed)
        multispeaker = bool(cfg["speaker_embed"] or cfg["WN_config"]["speaker_embed_dim"])
        ids = np.array([3, 17, 250, 511][:B], np.int64) if multispeaker else None
        tids = None if ids is None else torch.from_numpy(ids)
        samples = F * cfg["hop_length"]
        samples -= samples % cfg["n_group"]
        torch.manual_seed(seed)
        z = torch.empty(B, samples).normal_(std=sigma).numpy()
        torch.manual_seed(seed)
        with torch.no_grad():
            audio = model.infer(torch.from_numpy(mel.copy()), speaker_ids=tids, sigma=sigma).numpy()
            melp = np.pad(mel, ((0, 0), (0, 0), (0, 1)))
            inv, _ = model.inverse(torch.from_numpy(z.copy()), torch.from_numpy(melp.copy()), speaker_ids=tids)
        inv = inv.numpy()
        assert audio.shape == (B, samples - cfg["hop_length"]) and np.isfinite(inv).all()
        assert np.array_equal(inv[:, :audio.shape[1]], audio), "noise replay out of sync with infer()"
        path = os.path.join(HERE, f"waveglow_ax_{key}.npz")
        extra = {} if ids is None else {"speaker_ids": ids}
        np.savez_compressed(path, config_key=key, seed=seed, sigma=np.float32(sigma), mel=mel, z=z, audio=audio,
                            inverse_full=inv.astype(np.float32), **extra)
        assert os.path.getsize(path) < MAX_FILE
        print(f"[golden] waveglow_ax {key}: audio {audio.shape} rms={audio.std():.4f} max={np.abs(audio).max():.2f} -> "
              f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
