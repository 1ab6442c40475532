#!/usr/bin/env python3
"""Goldens of the teacher-forced pass: the reference's own ``Tacotron2.forward`` in ``eval()`` (model.py:976-1028), called the
way GTA.py calls it (``teacher_force_till=0, p_teacher_forcing=1.0, drop_frame_rate=0.0``, GTA.py:117), on the CPU with the
shims of make_golden.py.

Run in the build container only:

    python tests/golden/make_golden_taco_forced.py

Data only: inputs and the reference's outputs.  Weights come from ``cookietts_amd.synthetic`` by seed.  The prenet's always-on
``F.dropout`` (model.py:189-190) is replaced by a stand-in that applies OUR keep-masks to the two ``[T + 1, B, P]`` tensors the
reference's one-shot prenet sees (model.py:813, 823): mask t goes to row t - the prenet input of step t; row T (the prenet of
the last ground-truth frame, which no step reads) is dropped entirely.

Per case two files: ``tacotron_forced_<case>.npz`` (inputs, eight of the nine dict keys, the bottlenecked memory) and
``tacotron_forced_<case>_hidden.npz`` (``hidden_att_contexts``, the ninth), so that each stays well inside the size limit.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the repository and the reference on sys.path)
from cookietts_amd import synthetic  # noqa: E402

# name -> (hparam overrides, weight seed, B, symbols, text lengths, T, mel lengths, non-zero init_mel)
CASES = {
    "default": ({}, 1234, 3, 60, [60, 41, 12], 37, [37, 30, 21], False),
    "small": (synthetic.TACOTRON_SMALL_OVERRIDES, 4321, 3, 60, [60, 41, 12], 37, [37, 30, 21], False),
    "init": ({}, 1234, 2, 30, [30, 22], 9, [9, 7], True),
}


class _FrameMaskedDropout:
    """Stand-in for F.dropout inside the reference's model.py: call k (k = 0, 1: the prenet's two layers) multiplies the
    ``[T + 1, B, P]`` activations by ``masks[:, k] * 2`` on rows 0 .. T - 1 and by zero on row T."""

    def __init__(self, masks):
        self.masks, self.calls = masks, 0

    def __call__(self, x, p=0.5, training=True, inplace=False):
        if not training or p == 0:
            return x
        T = self.masks.shape[0]
        assert p == 0.5 and tuple(x.shape) == (T + 1,) + self.masks.shape[2:] and self.calls < 2, (x.shape, self.calls)
        keep = np.concatenate([self.masks[:, self.calls], np.zeros_like(self.masks[:1, 0])], axis=0).astype(np.float32)
        self.calls += 1
        return x * torch.from_numpy(keep) * 2.0


def inputs(name):
    """The inputs of one case (also what the tests would rebuild: everything is seeded)."""
    over, seed, B, n_sym, lens, T, mel_lens, with_init = CASES[name]
    hp = synthetic.tacotron_hparams(**over)
    rng = np.random.default_rng(seed + 606)
    lengths = np.array(lens, dtype=np.int64)
    text = rng.integers(1, hp.n_symbols, size=(B, n_sym)).astype(np.int64)
    for b in range(B):
        text[b, lengths[b]:] = 0
    speakers = np.array([3, 17, 250][:B], dtype=np.int64)
    tm = rng.standard_normal((B, hp.torchMoji_attDim)).astype(np.float32)
    gt_sylps = rng.uniform(2.5, 6.5, size=B).astype(np.float32)
    mel_lengths = np.array(mel_lens, dtype=np.int64)
    gt_mel = synthetic.synthetic_mel(B, T, hp.n_mel_channels, seed=seed)
    for b in range(B):
        gt_mel[b, :, mel_lengths[b]:] = 0.0                   # the reference's collate pads with zeros
    masks = synthetic.prenet_dropout_masks(T, B, hp.prenet_dim, seed=seed + 5)
    init_mel = (rng.standard_normal((B, hp.n_mel_channels, 1)) * 2.0 - 5.0).astype(np.float32) if with_init else None
    return hp, dict(seed=seed, text=text, lengths=lengths, speakers=speakers, torchmoji=tm, gt_sylps=gt_sylps,
                    mel_lengths=mel_lengths, gt_mel=gt_mel, masks=masks, **({"init_mel": init_mel} if with_init else {}))


def make(name):
    torch.set_num_threads(8)
    hp, d = inputs(name)
    small = bool(CASES[name][0])
    model, ref_model, _ = mg._ref_tacotron(hp, d["seed"],
                                           shapes_file="tacotron_small_state_shapes.json" if small else "tacotron_state_shapes.json")
    assert not model.training
    saved = ref_model.F.dropout
    ref_model.F.dropout = _FrameMaskedDropout(d["masks"])
    try:
        t = torch.from_numpy
        out = model(t(d["gt_mel"].copy()), t(d["mel_lengths"]), t(d["text"]), t(d["lengths"]), t(d["speakers"]), t(d["gt_sylps"]),
                    t(d["torchmoji"]), None, None, t(d["init_mel"].copy()) if "init_mel" in d else None,
                    teacher_force_till=0, p_teacher_forcing=1.0, drop_frame_rate=0.0, return_hidden_state=True)
        with torch.no_grad():
            memory = model.decoder.memory
    finally:
        ref_model.F.dropout = saved
    out = {k: v.detach().numpy().astype(np.float32) for k, v in out.items()}
    B, T = d["gt_mel"].shape[0], d["gt_mel"].shape[2]
    assert sorted(out) == sorted(["pred_mel", "pred_mel_postnet", "pred_gate_logits", "pred_sylps", "pred_sylps_mu",
                                  "pred_sylps_logvar", "alignments", "hidden_att_contexts", "encoder_outputs"])
    assert out["pred_mel"].shape == (B, hp.n_mel_channels, T) and out["pred_gate_logits"].shape == (B, T)
    assert out["hidden_att_contexts"].shape == (B, hp.second_decoder_rnn_dim + hp.memory_bottleneck_dim, T)
    assert all(np.isfinite(v).all() for v in out.values())
    hidden = out.pop("hidden_att_contexts")
    path = os.path.join(HERE, f"tacotron_forced_{name}.npz")
    np.savez_compressed(path, **d, **out, memory=memory.detach().numpy().astype(np.float32))
    hpath = os.path.join(HERE, f"tacotron_forced_{name}_hidden.npz")
    np.savez_compressed(hpath, hidden_att_contexts=hidden)
    print(f"[golden] tacotron_forced_{name}: mel {out['pred_mel'].shape} |mel| max {np.abs(out['pred_mel']).max():.3f}, mean max "
          f"weight {out['alignments'].max(-1).mean():.3f} -> {os.path.getsize(path) / 1024:.0f} + "
          f"{os.path.getsize(hpath) / 1024:.0f} KiB")


if __name__ == "__main__":
    for case in (sys.argv[1:] or list(CASES)):
        make(case)
