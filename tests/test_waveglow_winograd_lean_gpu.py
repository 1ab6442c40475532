"""The leaner Winograd layer of the fp32 WaveGlow against the five-launch form it replaces (CTTS_F32_WINOGRAD_PLAIN): bit for bit.

Default: the GATE launches of the layers with d % 4 == 0 read the cond rows where they lie in h_all, through their pair map
(the transform writes V only), T2 | T3 and even | odd are the two parts of one launch each (one round peel per pair) and the
d = 2 transform takes a vector path.  None of it changes a product or the order of a sum, so every comparison here is
torch.equal.  CTTS_F32_WINOGRAD_MIN=0 takes the Winograd form at every size.
"""
import numpy as np
import pytest
import torch

from cookietts_amd import WaveGlow, synthetic

pytestmark = pytest.mark.gpu


def _model(key, seed):
    cfg = synthetic.WAVEGLOW_CONFIGS[key] if isinstance(key, str) else key
    sd = synthetic.waveglow_state_dict(cfg, seed=seed)
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(sd))
    return m.cuda().eval(), cfg


def _inputs(cfg, B, F, seed):
    G = cfg["n_group"]
    mel = torch.from_numpy(synthetic.synthetic_mel(B, F, seed=seed)).cuda()
    z = torch.from_numpy(synthetic.synthetic_noise(B, G, F * cfg["hop_length"] // G, seed=seed) * np.float32(0.7)).cuda()
    return mel, z


def _lean_and_plain(m, tuning, mel, z):
    """(default, CTTS_F32_WINOGRAD_PLAIN) of one call under CTTS_F32_WINOGRAD_MIN=0, whatever else is set"""
    tuning.set("CTTS_F32_WINOGRAD_MIN", "0")
    lean = m.infer_from_noise(mel, z)
    tuning.set("CTTS_F32_WINOGRAD_PLAIN")
    plain = m.infer_from_noise(mel, z)
    tuning.clear("CTTS_F32_WINOGRAD_PLAIN")
    return lean, plain


@pytest.mark.parametrize("knob", [None, "CTTS_F32_NO_SMALL", "CTTS_F32_NO_WN_FOLD"])
def test_utterance_edges_both_kernel_shapes(hip_lib_path, tuning, knob):
    """d up to 128, B = 2.  F = 37: L = 1184, a multiple of neither 128 nor 256.  F = 5: L = 160 < 2 d at d = 128 - one pair
    block whose odd half hangs past the end, and mapped cond reads beyond L; it runs second on the same model, so the halo and
    the columns behind L hold the longer utterance's data.  CTTS_F32_NO_SMALL: the 256 x 128 shape (two parts in one launch) at
    these sizes, otherwise the small one.  CTTS_F32_NO_WN_FOLD: layer 0 reads x, d = 1 keeps the cond copy."""
    m, cfg = _model("full", 9)
    if knob:
        tuning.set(knob)
    for F in (37, 5):
        mel, z = _inputs(cfg, 2, F, seed=F)
        lean, plain = _lean_and_plain(m, tuning, mel, z)
        assert torch.isfinite(lean).all()
        assert torch.equal(lean, plain), (knob, F)


# the peel shapes of test_waveglow_winograd_gpu.py.  ("full", 7, 292): 259 pair-space tiles x 4 = 1036 workgroups per part: the small
# shape whole, part by part.  2 x 8 x 512 at 5 x 823: 515 tiles x 4 = 2060 per part, the 256 x 128 shape; two parts = 4120
# workgroups = 8 rounds + 24 on 256 CUs, so the merged launch still peels (6 tiles at the end of the last part's last item).
_PEEL_CFG = synthetic.waveglow_config(n_flows=2, n_channels=512, n_layers=8, n_early_every=4)


@pytest.mark.parametrize("key,B,F", [("full", 7, 292), (_PEEL_CFG, 5, 823)], ids=["full-7x292", "2x8x512-5x823"])
def test_round_peel_of_the_merged_launches(hip_lib_path, tuning, key, B, F):
    """The peel of a two-part launch is taken from the merged workgroup count and lies in the last part; its mapped cond segment
    keeps its row origin.  Bit-equal to the plain form, to the unpeeled launch (CTTS_F32_NO_ROUND_SPLIT) and run to run."""
    m, cfg = _model(key, 77)
    mel, z = _inputs(cfg, B, F, seed=7)
    lean, plain = _lean_and_plain(m, tuning, mel, z)
    again = m.infer_from_noise(mel, z)
    tuning.set("CTTS_F32_NO_ROUND_SPLIT")
    one = m.infer_from_noise(mel, z)
    assert torch.isfinite(lean).all()
    assert torch.equal(lean, plain)
    assert torch.equal(lean, again)
    assert torch.equal(lean, one)


def test_merged_parts_do_not_mix_batch_items(hip_lib_path, tuning):
    """Items 0 and B - 1 of a batch of three equal the same utterances run alone (and the plain form of the batch)."""
    m, cfg = _model("full", 5)
    B, F = 3, 292
    mel, z = _inputs(cfg, B, F, seed=3)
    full, plain = _lean_and_plain(m, tuning, mel, z)
    assert torch.isfinite(full).all() and torch.equal(full, plain)
    for b in (0, B - 1):
        assert torch.equal(m.infer_from_noise(mel[b:b + 1], z[b:b + 1])[0], full[b])
