"""fp32 WaveGlow with the WN start / end folds (the default) against the unfolded form (CTTS_F32_NO_WN_FOLD) and the goldens.

Layer 0 reads [audio_0; 1; 0] through W_in,0 . [W_start | b_start], and the skip sum is never formed: a skip/end pass
accumulates its 2 n_half-row image W_end . W_skip,i act_i and ends in the flow tail.  Same algebra, another summation order.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rms_rel_err
from cookietts_amd import WaveGlow, synthetic

pytestmark = pytest.mark.gpu

WAVE_TOL = 1e-3            # BASELINE.json: waveform RMS relative error
FOLD_VS_UNFOLDED = 1e-5    # a reordered sum, like the deferred-skip form's


def _model(key, seed):
    cfg = synthetic.WAVEGLOW_CONFIGS[key]
    sd = synthetic.waveglow_state_dict(cfg, seed=seed)
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(sd))
    return m.cuda().eval(), cfg


def _golden_args(g):
    ids = torch.from_numpy(g["speaker_ids"]).cuda() if "speaker_ids" in g.files else None
    return torch.from_numpy(g["mel"]).cuda(), torch.from_numpy(g["z_scaled"]).cuda(), ids


@pytest.mark.parametrize("name", ["full_short", "toy_early", "toy_spk_rezero", "toy_hop512_g16", "toy_hop384_g12"])
def test_folded_and_unfolded_match_the_golden_and_each_other(hip_lib_path, tuning, name):
    g = np.load(os.path.join(GOLDEN, f"waveglow_{name}.npz"))
    m, _ = _model(str(g["config_key"]), int(g["seed"]))
    mel, z, ids = _golden_args(g)
    folded = m.infer_from_noise(mel, z, speaker_id=ids).cpu().numpy()
    tuning.set("CTTS_F32_NO_WN_FOLD")
    unfolded = m.infer_from_noise(mel, z, speaker_id=ids).cpu().numpy()
    e = (rms_rel_err(folded, g["wave"]), rms_rel_err(unfolded, g["wave"]), rms_rel_err(folded, unfolded))
    print(f"{name}: folded vs reference {e[0]:.3e}, unfolded vs reference {e[1]:.3e}, folded vs unfolded {e[2]:.3e}")
    assert np.isfinite(folded).all()
    assert e[0] < WAVE_TOL and e[1] < WAVE_TOL and e[2] < FOLD_VS_UNFOLDED


@pytest.mark.parametrize("key,B,F", [("toy_early", 2, 37), ("full", 2, 37), ("toy_hop512_g16", 8, 131)])
def test_utterance_edges_match_the_unfolded_form(hip_lib_path, tuning, key, B, F):
    """The folded b_start rides on a ones row that is zero where the conv zero-pads: a wrong fold shows in the first and
    last samples of every utterance first.  Ragged widths (L not a multiple of the 128-column tile)."""
    m, cfg = _model(key, 9)
    G = cfg["n_group"]
    L = F * cfg["hop_length"] // G
    mel = torch.from_numpy(synthetic.synthetic_mel(B, F, seed=F)).cuda()
    z = torch.from_numpy(synthetic.synthetic_noise(B, G, L, seed=F) * np.float32(0.7)).cuda()
    folded = m.infer_from_noise(mel, z).cpu().numpy().astype(np.float64)
    tuning.set("CTTS_F32_NO_WN_FOLD")
    unfolded = m.infer_from_noise(mel, z).cpu().numpy().astype(np.float64)
    n = 2 * G
    for b in range(B):
        rms = np.sqrt(np.mean(unfolded[b] ** 2))
        head = np.max(np.abs(folded[b, :n] - unfolded[b, :n])) / rms
        tail = np.max(np.abs(folded[b, -n:] - unfolded[b, -n:])) / rms
        assert head < 1e-4 and tail < 1e-4, (b, head, tail)
    assert rms_rel_err(folded, unfolded) < FOLD_VS_UNFOLDED


def test_folded_rows_are_independent_of_batch_mates_and_run_to_run(hip_lib_path):
    m, cfg = _model("full", 5)
    B, F = 4, 37
    mel = torch.from_numpy(synthetic.synthetic_mel(B, F, seed=3)).cuda()
    z = torch.from_numpy(synthetic.synthetic_noise(B, 8, F * 32, seed=3) * np.float32(0.6)).cuda()
    full = m.infer_from_noise(mel, z)
    again = m.infer_from_noise(mel, z)
    assert torch.isfinite(full).all() and torch.equal(full, again)        # every workgroup owns its columns
    for b in range(B):
        one = m.infer_from_noise(mel[b:b + 1], z[b:b + 1])
        assert rms_rel_err(one.cpu().numpy(), full[b:b + 1].cpu().numpy()) < 1e-6


@pytest.mark.parametrize("mode", ["bf16x3", "bf16x6"])
def test_split_gemm_modes_with_the_fold(hip_lib_path, tuning, mode):
    """The split-bf16 main loops run the folded layer 0 too: inside their existing bounds (test_gemm_mode.py), and within the
    same bound of their own unfolded form."""
    g = np.load(os.path.join(GOLDEN, "waveglow_full_short.npz"))
    m, _ = _model(str(g["config_key"]), int(g["seed"]))
    m.set_f32_gemm_mode(mode)
    mel, z, _ = _golden_args(g)
    folded = m.infer_from_noise(mel, z).cpu().numpy()
    tuning.set("CTTS_F32_NO_WN_FOLD")
    unfolded = m.infer_from_noise(mel, z).cpu().numpy()
    e = (rms_rel_err(folded, g["wave"]), rms_rel_err(unfolded, g["wave"]))
    print(f"{mode}: folded vs reference {e[0]:.3e}, unfolded vs reference {e[1]:.3e}")
    assert e[0] < 1e-4 and e[1] < 1e-4
