"""The retry loop's restatement (tests/retry_restatement.py) against hand-computed cases, and the host-side surface of the
device path (exports, size query, refusal of CPU tensors).  No GPU: the device side is tests/test_retry_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from retry_restatement import RetryLoop, pcm16, score_candidate

#         diagonalitys avg_prob max_focus min_focus avg_focus p_missing: no punishment applies, the score is avg_prob
CLEAN = [1.0, 0.75, 10.0, 0.5, 4.0, 0.0]


def _pass(rows, T, avg_probs, n_mel=2, enc=3, seed=0):
    rng = np.random.default_rng(seed)
    mel = rng.standard_normal((rows, n_mel, T)).astype(np.float32)
    gate = rng.random((rows, T)).astype(np.float32)
    al = rng.random((rows, T, enc)).astype(np.float32)
    metrics = np.array([CLEAN] * rows, dtype=np.float64)
    metrics[:, 1] = avg_probs
    return mel, gate, al, metrics, np.arange(rows) % (T - 1) + 1


def test_score_by_hand():
    assert score_candidate(CLEAN, 20, False)[0] == 0.75
    s, d = score_candidate([1.6, 0.75, 80.0, -0.25, 3.1, 0.58], 13, False)
    # (1.6 - 1.1) * .5 * .5 = .125;  (80 - 60) * .005 = .1;  .25 * .5 = .125;  3.6 - 3.1 = .5;  .58 - .08 = .5   (float32 inputs)
    assert np.allclose(d[1:], [0.125, 0.1, 0.125, 0.5, 0.5], atol=1e-6, rtol=0)
    assert abs(s - (0.75 - 1.35)) < 1e-6 and d[0] == s
    assert score_candidate([1.6, 0.75, 80.0, -0.25, 3.1, 0.58], 13, True)[0] == 1e-7            # :615, detail keeps :605's value


def test_short_text_drops_the_missing_encoder_punishment():
    row = [1.0, 0.75, 10.0, 0.5, 4.0, 0.58]
    assert score_candidate(row, 12, False)[0] == 0.75 and score_candidate(row, 12, False)[1][5] == 0.0      # :603: > 12 only
    assert abs(score_candidate(row, 13, False)[0] - 0.25) < 1e-6


def test_a_tie_keeps_the_first_candidate():
    loop = RetryLoop(1, 3, max_attempts=64, target_score=0.9)
    st, scores, _ = loop.update(*_pass(3, 5, [0.5, 0.75, 0.75]), text_lengths=[20])
    assert list(scores) == [0.5, 0.75, 0.75] and loop.best_where[0] == (0, 1) and loop.best_score[0] == 0.75   # :616 is strict
    assert st.done == 0 and st.min_tries == 3 and st.n_passes == 1


def test_nan_metric_never_wins_and_nan_mel_scores_1e_minus_7():
    loop = RetryLoop(2, 2, max_attempts=64, target_score=0.9)
    mel, gate, al, metrics, ol = _pass(4, 5, [0.75, 0.5, 0.25, 0.25])
    metrics[0, 1] = np.nan            # text 0, candidate 0: NaN score - `nan > best` is False, it never wins (:616)
    metrics[2:, 4] = 1.0              # text 1: avg_focus punishment 2.6 -> both candidates score 0.25 - 2.6 < 0
    mel[3, -1, -1] = np.nan           # ... but candidate 1 holds a NaN: 1e-7 (:615) beats the negative score
    st, scores, _ = loop.update(mel, gate, al, metrics, ol, [20, 20])
    assert np.isnan(scores[0]) and scores[1] == 0.5 and abs(scores[2] + 2.35) < 1e-6 and scores[3] == 1e-7
    assert loop.best_where == [(0, 1), (0, 3)] and list(loop.best_score) == [0.5, 1e-7]
    assert st.min_best_score == 1e-7 and st.n_without_winner == 0


def test_max_attempts_rule_stops_the_pass_mid_text():
    """:621-622 raise out of both loops: the last text's candidates behind the one that completed max_attempts are never
    looked at, however good."""
    loop = RetryLoop(2, 3, max_attempts=4, target_score=0.9)
    loop.update(*_pass(6, 5, [0.25] * 6), text_lengths=[20, 20])
    assert loop.done == 0 and list(loop.tries) == [3, 3]
    st, _, _ = loop.update(*_pass(6, 5, [0.25, 0.25, 0.25, 0.25, 0.25, 0.75], seed=1), text_lengths=[20, 20])
    assert st.done == 2 and list(loop.tries) == [6, 4] and st.min_tries == 4        # stopped behind text 1's first candidate
    assert loop.best_score[1] == 0.25 and loop.best_where[1] == (0, 3)               # the 0.75 of row 5 was not considered
    before = (loop.best_score.copy(), loop.tries.copy(), st)
    st2, _, _ = loop.update(*_pass(6, 5, [0.8] * 6, seed=2), text_lengths=[20, 20])  # the loop has been left
    assert st2 == before[2] and (loop.best_score == before[0]).all() and (loop.tries == before[1]).all()


def test_absolute_maximum_and_target_rules():
    loop = RetryLoop(1, 2, max_attempts=64, target_score=0.9, absolute_maximum_tries=3)
    assert loop.update(*_pass(2, 5, [0.25, 0.25]), text_lengths=[20])[0].done == 0
    st = loop.update(*_pass(2, 5, [0.25, 0.95]), text_lengths=[20])[0]
    assert st.done == 3 and st.min_tries == 3 and loop.best_score[0] == 0.25          # :623; the 0.95 came too late
    loop = RetryLoop(1, 2, max_attempts=64, target_score=0.5)
    assert loop.update(*_pass(2, 5, [0.25, 0.5]), text_lengths=[20])[0].done == 1     # :552: not (min < target)


def test_a_pass_one_winner_keeps_its_length_and_is_padded_from_its_own_T():
    """:645-651 pad the winners' whole pass-length mels: a winner of a T = 37 pass keeps columns [output_length, 37) as the
    decoder wrote them, and -11.52 starts at column 37 - when another text's winner is longer."""
    loop = RetryLoop(2, 1, max_attempts=64, target_score=0.9)
    p1 = _pass(2, 37, [0.75, 0.25])
    p1[4][:] = [30, 20]
    loop.update(*p1, text_lengths=[20, 20])
    p2 = _pass(2, 21, [0.5, 0.5], seed=1)
    p2[4][:] = [15, 18]
    st, _, _ = loop.update(*p2, text_lengths=[20, 20])
    assert loop.best_where == [(0, 0), (1, 1)] and st.max_best_length == 30 and st.max_best_T == 37
    mel, lengths = loop.vocoder_batch()
    assert mel.shape == (2, 2, 30) and list(lengths) == [30, 18]
    assert (mel[0] == p1[0][0][:, :30]).all()
    assert (mel[1, :, :21] == p2[0][1]).all() and (mel[1, :, 21:] == np.float32(-11.52)).all()   # from ITS T, not from 18
    # and the longest winner decides where padding can start at all: cut at max_length = 45 > 37
    loop = RetryLoop(2, 1, max_attempts=64, target_score=0.9)
    p1 = _pass(2, 37, [0.75, 0.25])
    p1[4][:] = [30, 20]
    loop.update(*p1, text_lengths=[20, 20])
    p3 = _pass(2, 50, [0.5, 0.5], seed=3)
    p3[4][:] = [15, 45]
    loop.update(*p3, text_lengths=[20, 20])
    mel, lengths = loop.vocoder_batch()
    assert mel.shape == (2, 2, 45) and (mel[0, :, :37] == p1[0][0]).all() and (mel[0, :, 37:] == np.float32(-11.52)).all()


def test_pcm_restatement_by_hand():
    audio = np.zeros((2, 12), dtype=np.float32)
    audio[0, :8] = [1.0, -1.0, 0.99997, -0.00002, 1.5, -np.inf, np.nan, 0.5]
    audio[1, :4] = [0.25, -0.25, 3.0517578125e-05, -3.0517578125e-05]
    pcm, offsets = pcm16(audio, [2, 1], 4, 3)
    assert list(offsets) == [0, 11, 18]
    assert list(pcm[:11]) == [32767, -32768, 32767, 0, 32767, -32768, 0, 16384, 0, 0, 0]
    assert list(pcm[11:]) == [8192, -8192, 1, -1, 0, 0, 0]
    assert list(pcm16(audio.astype(np.float16), [0, 3], 4, 0)[1]) == [0, 0, 12]


# ---- host side of the device path -------------------------------------------------------------------------------------
NEW_SYMBOLS = ("ctts_retry_state_bytes", "ctts_retry_state_layout", "ctts_retry_reset", "ctts_retry_update_f32",
               "ctts_retry_vocoder_batch_f32", "ctts_pcm16_concat")


def _config(n_texts, per_text, n_mel=160, t_cap=1000, enc_cap=0):
    from cookietts_amd import _lib
    return _lib.RetryConfig(0.5, 1.0, 0.5, 1.0, 0.75, -1e3, 64, 2048, n_texts, per_text, n_mel, t_cap, enc_cap)


def test_library_exports_the_retry_symbols_and_sizes_the_state(hip_lib_path):
    import os
    from conftest import REPO
    from cookietts_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(REPO, "include", "cookietts_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert (name + "(") in header and name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    assert lib.ctts_abi_version() == 7
    assert C.sizeof(_lib.RetryStatus) == 32
    cfg = _config(4, 64)                                          # the shipped t2s_config.json: 256 rows per pass
    n = lib.ctts_retry_state_bytes(C.byref(cfg))
    assert n >= 32 + 4 * 160 * 1000 * 4
    offsets = (C.c_size_t * 14)()
    assert lib.ctts_retry_state_layout(C.byref(cfg), offsets) == 0
    offs = list(offsets)
    assert offs[0] == 0 and offs[1] == 32 and offs == sorted(offs) and all(o % 16 == 0 for o in offs) and offs[-1] < n
    assert lib.ctts_retry_state_bytes(C.byref(_config(4, 64, enc_cap=200))) == n + 4 * 1000 * 200 * 4
    assert lib.ctts_retry_state_bytes(C.byref(_config(64, 64))) > 0                       # 4096 rows: the limit
    for bad in (_config(64, 65), _config(4097, 1), _config(0, 4), _config(4, 64, n_mel=0)):
        assert lib.ctts_retry_state_bytes(C.byref(bad)) == 0 and "retry" in _lib.last_error()
    assert lib.ctts_retry_state_bytes(C.byref(_config(64, 65))) == 0 and "4096" in _lib.last_error()
    assert lib.ctts_retry_update_f32(C.byref(_config(64, 65)), *([None] * 6), 8, 8, None, None, None) != 0   # refused, no launch


def test_best_of_n_and_pcm16_concat_refuse_cpu_tensors(hip_lib_path):
    import cookietts_amd
    from cookietts_amd import BestOfN, _lib, pcm16_concat
    assert {"BestOfN", "pcm16_concat"} <= set(cookietts_amd.__all__)
    loop = BestOfN(2, 3, 8, 40, max_attempts=4, target_score=0.75)
    assert not loop.done and loop.status.n_without_winner == 2
    out = {"pred_mel_postnet": torch.zeros(6, 8, 5), "pred_gate": torch.zeros(6, 5), "alignments": torch.zeros(6, 5, 4)}
    with pytest.raises(_lib.HipLibraryError):
        loop.update(out, torch.tensor([20, 20]))
    with pytest.raises(_lib.HipLibraryError):
        pcm16_concat(torch.zeros(2, 1, 64), torch.tensor([3, 4]), 16)
    with pytest.raises(_lib.HipLibraryError):
        BestOfN(2, 3, 8, 40, max_attempts=4, target_score=0.75, device="cpu")
