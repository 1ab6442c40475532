"""fp32 WaveGlow with the Winograd F(2,3) in-layer form against the direct 3-tap form (CTTS_F32_NO_WINOGRAD) and the goldens.

The layers that read x compute their dilated 3-tap conv on output pairs (t, t + d): a transform kernel, T2 = G2 V2, T3 = G3 V3
and an even / odd GATE launch with two addends and a pair-column -> natural-column store (waveglow_api.hip,
run_in_layer_winograd).  Same algebra with 2 C instead of 3 C products per output: a re-ordered sum.  CTTS_F32_WINOGRAD_MIN=0
takes the form at every size (by default short utterances keep the direct form).
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rms_rel_err
from cookietts_amd import WaveGlow, synthetic

pytestmark = pytest.mark.gpu

REORDERED_SUM = 1e-5       # the project's bound for a re-ordered sum; the fp32 path is held to it against the goldens too


def _model(key, seed):
    cfg = synthetic.WAVEGLOW_CONFIGS[key] if isinstance(key, str) else key
    sd = synthetic.waveglow_state_dict(cfg, seed=seed)
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(sd))
    return m.cuda().eval(), cfg


def _golden_args(g):
    ids = torch.from_numpy(g["speaker_ids"]).cuda() if "speaker_ids" in g.files else None
    return torch.from_numpy(g["mel"]).cuda(), torch.from_numpy(g["z_scaled"]).cuda(), ids


def _inputs(cfg, B, F, seed):
    G = cfg["n_group"]
    mel = torch.from_numpy(synthetic.synthetic_mel(B, F, seed=seed)).cuda()
    z = torch.from_numpy(synthetic.synthetic_noise(B, G, F * cfg["hop_length"] // G, seed=seed) * np.float32(0.7)).cuda()
    return mel, z


def _both(m, tuning, *args, **kw):
    """(Winograd at every size, direct) of one call, whatever else is set"""
    tuning.set("CTTS_F32_WINOGRAD_MIN", "0")
    wino = m.infer_from_noise(*args, **kw)
    tuning.set("CTTS_F32_NO_WINOGRAD")
    direct = m.infer_from_noise(*args, **kw)
    tuning.clear("CTTS_F32_NO_WINOGRAD")
    return wino, direct


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("name", ["full_short", "toy_early", "toy_spk_rezero", "toy_hop512_g16", "toy_hop384_g12", "small"])
def test_winograd_matches_the_golden_and_the_direct_form(hip_lib_path, tuning, name, fold):
    g = np.load(os.path.join(GOLDEN, f"waveglow_{name}.npz"))
    m, _ = _model(str(g["config_key"]), int(g["seed"]))
    mel, z, ids = _golden_args(g)
    if not fold:
        tuning.set("CTTS_F32_NO_WN_FOLD")       # layer 0 reads x too
    wino, direct = _both(m, tuning, mel, z, speaker_id=ids)
    wino, direct = wino.cpu().numpy(), direct.cpu().numpy()
    e = (rms_rel_err(wino, g["wave"]), rms_rel_err(direct, g["wave"]), rms_rel_err(wino, direct))
    print(f"{name} fold={fold}: winograd vs reference {e[0]:.3e}, direct vs reference {e[1]:.3e}, winograd vs direct {e[2]:.3e}")
    assert np.isfinite(wino).all()
    assert e[0] < REORDERED_SUM and e[2] < REORDERED_SUM


@pytest.mark.parametrize("no_small", [False, True])
@pytest.mark.parametrize("F", [5, 37])
def test_utterance_edges_match_the_direct_form(hip_lib_path, tuning, F, no_small):
    """d up to 128.  F = 5: L = 160 < 2 d, a single pair block whose odd half hangs over the end; F = 37: L = 1184, no multiple
    of 256 or 128.  A wrong zero padding or pair mapping shows in the first and last samples of every utterance first.
    CTTS_F32_NO_SMALL: the 256 x 128 kernel's epilogue at this size."""
    m, cfg = _model("full", 9)
    B, G = 2, cfg["n_group"]
    mel, z = _inputs(cfg, B, F, seed=F)
    if no_small:
        tuning.set("CTTS_F32_NO_SMALL")
    wino, direct = _both(m, tuning, mel, z)
    wino, direct = wino.cpu().numpy().astype(np.float64), direct.cpu().numpy().astype(np.float64)
    n = 2 * G
    for b in range(B):
        rms = np.sqrt(np.mean(direct[b] ** 2))
        head = np.max(np.abs(wino[b, :n] - direct[b, :n])) / rms
        tail = np.max(np.abs(wino[b, -n:] - direct[b, -n:])) / rms
        print(f"F={F} no_small={no_small} item {b}: head {head:.3e} tail {tail:.3e}")
        assert head < 1e-4 and tail < 1e-4, (b, head, tail)
    assert rms_rel_err(wino, direct) < REORDERED_SUM


# 512 channels = 4 m-blocks.  ("full", 7, 292): 259 pair-space column tiles x 4 = 1036 workgroups = 2 rounds + 12 on 256 CUs.  A launch
# below 2048 large blocks takes the small shape whole (gemm_f32_small_applies), so the second case is the one that runs the
# 256 x 128 shape with a peeled remainder: 2 flows x 8 layers x 512 channels, 5 x 103 = 515 pair-space tiles x 4 = 2060
# workgroups = 4 rounds + 12 (the peel: 3 tiles of the last batch item through the small shape).
_PEEL_CFG = synthetic.waveglow_config(n_flows=2, n_channels=512, n_layers=8, n_early_every=4)


@pytest.mark.parametrize("key,B,F", [("full", 7, 292), (_PEEL_CFG, 5, 823)], ids=["full-7x292", "2x8x512-5x823"])
def test_round_peel_in_pair_space(hip_lib_path, tuning, key, B, F):
    """The peeled tiles of a mapped-store launch advance a pair-column origin, not the destination, and both addends:
    bit-equal to the single launch (CTTS_F32_NO_ROUND_SPLIT) and run to run, and the direct form within a re-ordered sum."""
    m, cfg = _model(key, 77)
    mel, z = _inputs(cfg, B, F, seed=7)
    wino, direct = _both(m, tuning, mel, z)
    again = m.infer_from_noise(mel, z)
    tuning.set("CTTS_F32_NO_ROUND_SPLIT")
    one = m.infer_from_noise(mel, z)
    e = rms_rel_err(wino.cpu().numpy(), direct.cpu().numpy())
    print(f"B={B} F={F}: winograd vs direct {e:.3e}")
    assert torch.isfinite(wino).all() and e < REORDERED_SUM
    assert torch.equal(wino, again)
    assert torch.equal(wino, one)


def test_split_bf16_loops_keep_the_direct_form(hip_lib_path, tuning):
    g = np.load(os.path.join(GOLDEN, "waveglow_full_short.npz"))
    m, _ = _model(str(g["config_key"]), int(g["seed"]))
    m.set_f32_gemm_mode("bf16x6")
    mel, z, _ = _golden_args(g)
    wino, direct = _both(m, tuning, mel, z)
    assert torch.isfinite(wino).all() and torch.equal(wino, direct)


def test_winograd_rows_are_independent_of_batch_mates(hip_lib_path, tuning):
    """An utterance alone takes the small kernel shape, in a batch of five the 256 x 128 one (565 pair-space tiles x 4 = 2260 blocks): same bits in both."""
    m, cfg = _model("full", 5)
    B, F = 5, 900
    mel, z = _inputs(cfg, B, F, seed=3)
    tuning.set("CTTS_F32_WINOGRAD_MIN", "0")
    full = m.infer_from_noise(mel, z)
    assert torch.isfinite(full).all()
    for b in (0, B - 1):
        assert torch.equal(m.infer_from_noise(mel[b:b + 1], z[b:b + 1])[0], full[b])


def test_default_threshold_keeps_short_utterances_on_the_direct_form(hip_lib_path, tuning):
    """Without CTTS_F32_WINOGRAD_MIN a short utterance is below the threshold: bit-equal to CTTS_F32_NO_WINOGRAD."""
    m, cfg = _model("toy", 3)
    mel, z = _inputs(cfg, 1, 11, seed=4)
    default = m.infer_from_noise(mel, z)
    tuning.set("CTTS_F32_NO_WINOGRAD")
    direct = m.infer_from_noise(mel, z)
    assert torch.equal(default, direct)
