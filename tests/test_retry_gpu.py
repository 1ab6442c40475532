"""The retry loop on the device (csrc/retry.hip, cookietts_amd/retry.py) against tests/retry_restatement.py fed the same
arrays, bit for bit: the arithmetic is double add, multiply and compare, copies and a truncation, so there are no tolerances.
The one exception is stated where it is made: the payload of a NaN score is not compared, only that it is a NaN."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from retry_restatement import RetryLoop, pcm16

pytestmark = pytest.mark.gpu

SECTIONS = ("status", "best_score", "detail", "tries", "best_length", "best_T", "best_pass", "best_row", "changed", "best_mel",
            "best_alignments", "row_score", "row_detail", "row_flags")
PAD = np.float32(-11.52)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


class DeviceLoop:
    """The C entry points as they are, on caller-owned torch memory."""

    def __init__(self, n_texts, per_text, n_mel, t_cap, enc_cap, *, max_attempts, target_score, absolute_maximum_tries=2048,
                 absolutely_required_score=-1e3, weights=(0.5, 1.0, 0.5, 1.0)):
        from cookietts_amd import _lib
        self._lib, self.lib = _lib, _lib.lib()
        self.N, self.P, self.n_mel, self.t_cap, self.enc_cap = n_texts, per_text, n_mel, t_cap, enc_cap
        self.cfg = _lib.RetryConfig(*weights, target_score, absolutely_required_score, max_attempts, absolute_maximum_tries,
                                    n_texts, per_text, n_mel, t_cap, enc_cap)
        nbytes = self.lib.ctts_retry_state_bytes(C.byref(self.cfg))
        assert nbytes > 0, _lib.last_error()
        offsets = (C.c_size_t * len(SECTIONS))()
        assert self.lib.ctts_retry_state_layout(C.byref(self.cfg), offsets) == 0
        self.off = dict(zip(SECTIONS, offsets))
        self.state = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")           # reset must not rely on zeros
        self.stream = _lib.stream(self.state.device)
        _lib.check(self.lib.ctts_retry_reset(C.byref(self.cfg), _lib.ptr(self.state), self.stream), "ctts_retry_reset")

    def section(self, name, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return self.state[self.off[name]:self.off[name] + n].cpu().numpy().view(dtype).reshape(shape)

    def status(self):
        s = self._lib.RetryStatus.from_buffer_copy(self.state[:32].cpu().numpy().tobytes())
        return tuple(getattr(s, f) for f, _ in self._lib.RetryStatus._fields_)

    def update(self, mel, gate, al, metrics, ol, tl):
        dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in
               (mel, gate, al, metrics, np.asarray(ol, dtype=np.int32), np.asarray(tl, dtype=np.int32))]
        rows, T, enc = al.shape
        detail = torch.full((rows, 6), -7.0, dtype=torch.float64, device="cuda")
        p = self._lib.ptr
        self._lib.check(self.lib.ctts_retry_update_f32(C.byref(self.cfg), *(p(d) for d in dev), T, enc, p(detail), p(self.state),
                                                       self.stream), "ctts_retry_update_f32")
        torch.cuda.synchronize()
        return self.status(), self.section("row_score", (rows,), np.float64), detail.cpu().numpy()

    def vocoder_batch(self, t_out, pad=-11.52):
        out = torch.empty(self.N, self.n_mel, t_out, dtype=torch.float32, device="cuda")
        self._lib.check(self.lib.ctts_retry_vocoder_batch_f32(C.byref(self.cfg), self._lib.ptr(self.state), self._lib.ptr(out),
                                                              t_out, pad, self.stream), "ctts_retry_vocoder_batch_f32")
        return out.cpu().numpy()

    def kept(self):
        """The persistent per-text sections (everything but `changed` and the scratch of the last update)."""
        N = self.N
        d = {k: self.section(k, (N,), np.int32) for k in ("tries", "best_length", "best_T", "best_pass", "best_row")}
        d["best_score"] = self.section("best_score", (N,), np.uint64)
        d["detail"] = self.section("detail", (N, 6), np.uint64)
        d["best_mel"] = self.section("best_mel", (N, self.n_mel, self.t_cap), np.uint32)
        return d


def compare_with(loop, dev, st_ref, st_dev):
    """Status and per-text state of the device against the restatement's."""
    assert st_dev[:2] == tuple(st_ref[:2]) and st_dev[3:] == tuple(st_ref[3:]), (st_dev, st_ref)
    assert bits(st_dev[2]) == bits(st_ref.min_best_score)
    k = dev.kept()
    assert (k["best_score"] == bits(loop.best_score)).all()
    assert (k["tries"] == loop.tries.astype(np.int32)).all()
    al = dev.section("best_alignments", (dev.N, dev.t_cap, dev.enc_cap), np.uint32) if dev.enc_cap else None
    for j, g in enumerate(loop.best_generations):
        if g == 0:
            assert k["best_pass"][j] == -1 and k["best_row"][j] == -1 and k["best_T"][j] == 0
            continue
        T = g[0].shape[1]
        assert (k["best_pass"][j], k["best_row"][j]) == loop.best_where[j]
        assert k["best_length"][j] == g[1] and k["best_T"][j] == T
        assert (k["detail"][j] == bits(loop.best_detail[j])).all()
        assert (k["best_mel"][j][:, :T] == g[0].view(np.uint32)).all()
        if al is not None:
            assert (al[j][:T, :g[2].shape[1]] == g[2].view(np.uint32)).all()


def straddling_metrics(rng, rows):
    """Six columns drawn on, just below and just above every threshold of :599-603 (1.10, 60, 0, 3.6, 0.08); columns 1-5 as
    doubles that are NOT float32 values in half of the rows, so the rounding the library documents is exercised."""
    pick = lambda vals: rng.choice(np.array(vals, dtype=np.float64), size=rows)
    m = np.stack([pick([0.9, 1.10, 1.1000000000000003, 1.0999999999999999, 1.7, 2.4]),
                  rng.random(rows),
                  pick([10.0, 59.5, 60.0, 60.00001, 90.0, 200.0]),
                  pick([-0.3, -1e-9, 0.0, 0.2, 0.9]),
                  pick([2.0, 3.5, 3.6, 3.6000001, 3.7, 5.0]),
                  pick([0.0, 0.07, 0.08, 0.0800001, 0.09, 0.3])], axis=1)
    f32 = rng.random(rows) < 0.5
    m[f32, 1:] = m[f32, 1:].astype(np.float32)
    return m


def synthetic_pass(rng, rows, n_mel, T, enc, lo=1):
    mel = rng.standard_normal((rows, n_mel, T)).astype(np.float32)
    gate = rng.random((rows, T)).astype(np.float32)
    al = rng.random((rows, T, enc)).astype(np.float32)
    return mel, gate, al, straddling_metrics(rng, rows), rng.integers(lo, T, size=rows).astype(np.int32)


def test_synthetic_passes_match_the_restatement_bit_for_bit(hip_lib_path):
    """Three passes of T = 37, 21, 40 at enc = 13: rows of gate and alignments start off 16-byte boundaries and T * enc is odd
    (scalar head and tail of the NaN scan); one NaN in the LAST element of one row of mel, gate and alignments in turn."""
    N, P, n_mel, enc = 3, 2, 8, 13
    rng = np.random.default_rng(7)
    tl = [12, 13, 30]                                            # :603: 12 drops the punishment, 13 keeps it
    kw = dict(max_attempts=64, target_score=500.0)
    loop, dev = RetryLoop(N, P, **kw), DeviceLoop(N, P, n_mel, 40, enc, **kw)
    # avg_prob steers who wins (the punishments sum to less than 4): text 0 in pass 0 for good, text 2 in the longest pass;
    # text 1 improves every pass
    boost = [[30.0, 0.0, 0.0], [0.0, 10.0, 10.0], [0.0, 20.0, 40.0]]
    for n, T in enumerate((37, 21, 40)):
        mel, gate, al, metrics, ol = synthetic_pass(rng, N * P, n_mel, T, enc)
        metrics[:, 1] += np.repeat(boost[n], P)
        if n == 2:
            ol[2 * P:] = 39                                      # text 2's winner is longer than text 0's whole pass
        planted = (mel, gate, al)[n]
        planted[(1, 4, 3)[n]].reshape(-1)[-1] = np.nan
        st_ref, sc_ref, det_ref = loop.update(mel, gate, al, metrics, ol, tl)
        st_dev, sc_dev, det_dev = dev.update(mel, gate, al, metrics, ol, tl)
        assert sc_ref[(1, 4, 3)[n]] == 1e-7 and np.isfinite(sc_ref).all()
        assert (bits(sc_dev) == bits(sc_ref)).all(), (sc_dev, sc_ref)
        assert (bits(det_dev) == bits(det_ref)).all()
        compare_with(loop, dev, st_ref, st_dev)
        assert st_dev[0] == 0 and st_dev[1] == n + 1
    assert [w[0] for w in loop.best_where] == [0, 2, 2] and st_ref.max_best_length == 39 and st_ref.max_best_T == 40
    want, _ = loop.vocoder_batch()
    got = dev.vocoder_batch(st_dev[5])
    assert got.shape == want.shape == (N, n_mel, 39) and (got.view(np.uint32) == want.view(np.uint32)).all()
    assert (got[0][:, 37:] == PAD).all() and (got[0][:, :37] == loop.best_generations[0][0]).all()   # padded from ITS T on
    # a pass longer than the capacity, or wider than the kept alignments, is refused before anything is launched
    before = dev.state.clone()
    big = synthetic_pass(rng, N * P, n_mel, 41, enc)
    with pytest.raises(dev._lib.HipLibraryError, match="t_cap"):
        dev.update(*big, tl)
    wide = synthetic_pass(rng, N * P, n_mel, 30, enc + 1)
    with pytest.raises(dev._lib.HipLibraryError, match="enc_cap"):
        dev.update(*wide, tl)
    torch.cuda.synchronize()
    assert torch.equal(before, dev.state)


def test_a_nan_metric_never_wins(hip_lib_path):
    """A NaN metric makes the score NaN (Python's max keeps a NaN first argument) and `nan > best` is False.  Which NaN the
    arithmetic produces (sign, payload) is not specified by IEEE 754 and differs between hosts and the GPU, so for these rows
    the test asks for a NaN, not for its bits; every other row and all state is compared bit for bit."""
    N, P, n_mel, enc, T = 2, 3, 4, 5, 9
    rng = np.random.default_rng(11)
    kw = dict(max_attempts=64, target_score=5.0)
    loop, dev = RetryLoop(N, P, **kw), DeviceLoop(N, P, n_mel, T, 0, **kw)
    mel, gate, al, metrics, ol = synthetic_pass(rng, N * P, n_mel, T, enc)
    metrics[0, 0] = np.nan                                       # through max(diagonality, 1.10)
    metrics[2, 3] = np.nan                                       # through max(0.0 - min_focus, 0)
    metrics[3:, 1] = np.nan                                      # text 1: no candidate can win this pass
    st_ref, sc_ref, _ = loop.update(mel, gate, al, metrics, ol, [20, 20])
    st_dev, sc_dev, _ = dev.update(mel, gate, al, metrics, ol, [20, 20])
    nan = np.isnan(sc_ref)
    assert list(nan) == [True, False, True, True, True, True] and (np.isnan(sc_dev) == nan).all()
    assert (bits(sc_dev)[~nan] == bits(sc_ref)[~nan]).all()
    compare_with(loop, dev, st_ref, st_dev)
    assert st_dev[4] == 1 and loop.best_where == [(0, 1), None]


@pytest.mark.parametrize("case", ["max_attempts", "absolute_maximum_tries", "target"])
def test_stop_rules_and_the_sticky_verdict(hip_lib_path, case):
    N, P, n_mel, enc, T = 2, 3, 4, 5, 9
    kw = {"max_attempts": dict(max_attempts=4, target_score=50.0),                    # fires mid-pass in pass 2 (:621)
          "absolute_maximum_tries": dict(max_attempts=64, target_score=50.0, absolute_maximum_tries=5),           # (:623)
          "target": dict(max_attempts=64, target_score=-40.0)}[case]                  # reached in pass 1 (:552)
    rng = np.random.default_rng(3)
    loop, dev = RetryLoop(N, P, **kw), DeviceLoop(N, P, n_mel, T, enc, **kw)
    tl = [30, 9]
    for n in range(3):                                           # the third update comes after the verdict in every case
        p = synthetic_pass(rng, N * P, n_mel, T, enc)
        p[3][:, 1] += n                                          # later passes score higher: they WOULD win
        kept = dev.kept()
        st_ref, _, _ = loop.update(*p, tl)
        st_dev, _, _ = dev.update(*p, tl)
        compare_with(loop, dev, st_ref, st_dev)
        if n == 2 or (case == "target" and n == 1):              # done on entry: nothing may change
            now = dev.kept()
            assert all((kept[k] == now[k]).all() for k in kept)
            assert (dev.section("changed", (N,), np.int32) == -1).all()
    want = {"max_attempts": (2, 2, 4), "absolute_maximum_tries": (3, 2, 5), "target": (1, 1, 3)}[case]
    assert (st_dev[0], st_dev[1], st_dev[3]) == want             # done, n_passes, min_tries
    if case == "max_attempts":
        assert list(loop.tries) == [6, 4]                        # text 1's candidates 1 and 2 of pass 2 were not considered


def test_widest_replay_4096_rows(hip_lib_path):
    """64 texts x 64 candidates: every thread of the replay workgroup owns texts, the running minima cross all 16 waves, and
    max_attempts = 60 fires at the last text's 60th candidate."""
    N, P, n_mel, enc, T = 64, 64, 4, 8, 8
    rng = np.random.default_rng(5)
    kw = dict(max_attempts=60, target_score=50.0)
    loop, dev = RetryLoop(N, P, **kw), DeviceLoop(N, P, n_mel, T, 0, **kw)
    p = synthetic_pass(rng, N * P, n_mel, T, enc)
    p[0][77, 0, 0] = np.nan
    tl = rng.integers(5, 40, size=N)
    st_ref, sc_ref, det_ref = loop.update(*p, tl)
    st_dev, sc_dev, det_dev = dev.update(*p, tl)
    assert (bits(sc_dev) == bits(sc_ref)).all() and (bits(det_dev) == bits(det_ref)).all()
    compare_with(loop, dev, st_ref, st_dev)
    assert st_dev[0] == 2 and st_dev[3] == 60 and loop.tries[-1] == 60 and loop.tries[0] == 64
    want, _ = loop.vocoder_batch()
    assert (dev.vocoder_batch(st_dev[5]).view(np.uint32) == want.view(np.uint32)).all()
    # a second state whose rule fires in the MIDDLE of the pass: texts behind it keep their entry state
    kw = dict(max_attempts=64, target_score=50.0, absolute_maximum_tries=0)
    loop, dev = RetryLoop(N, P, **kw), DeviceLoop(N, P, n_mel, T, 0, **kw)
    st_ref, _, _ = loop.update(*p, tl)
    st_dev, _, _ = dev.update(*p, tl)
    compare_with(loop, dev, st_ref, st_dev)
    assert st_dev[0] == 3 and st_dev[4] == N - 1 and loop.tries.sum() == 1        # stopped behind the very first candidate


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("frames", [[0, 7, 12], [0, 7, 13]], ids=["issue", "clamped_to_ld"])
def test_pcm16_concat(hip_lib_path, dtype, frames):
    from cookietts_amd import _lib, pcm16_concat
    B, ld, hop, silence = 3, 50, 4, 5
    rng = np.random.default_rng(2)
    audio = (rng.random((B, ld)) * 2 - 1).astype(np.float32)
    audio[1, :8] = [1.0, -1.0, 0.99997, -0.00002, 1.5, -np.inf, np.nan, np.inf]
    audio[2, 40:48] = [-1.5, 2.0 ** -15, -(2.0 ** -15), 0.0, -0.0, 0.5, -0.99997, np.nan]
    audio = audio.astype(dtype)
    want, want_off = pcm16(audio, frames, hop, silence)
    assert want[5 + 3] == 0 and want[5] == 32767 and want[6] == -32768                 # -0.00002 truncates to 0, not to -1
    for shape in ((B, 1, ld), (B, ld)):
        got, off = pcm16_concat(torch.from_numpy(audio).cuda().reshape(shape), torch.tensor(frames).cuda(), hop, silence)
        assert got.dtype == torch.int16 and off.dtype == torch.int64
        assert (off.cpu().numpy() == want_off).all() and (got.cpu().numpy() == want).all()
    got0, off0 = pcm16_concat(torch.from_numpy(audio).cuda(), frames, hop)              # no silence
    assert (got0.cpu().numpy() == pcm16(audio, frames, hop, 0)[0]).all()
    # capacity one short of the total: nothing behind it is written, the total comes back negative
    total = int(want_off[-1])
    pcm = torch.full((total + 8,), 0x5A5A, dtype=torch.int16, device="cuda")
    off = torch.zeros(B + 1, dtype=torch.int64, device="cuda")
    a, f = torch.from_numpy(audio).cuda(), torch.tensor(frames, dtype=torch.int32).cuda()
    _lib.check(_lib.lib().ctts_pcm16_concat(_lib.ptr(a), int(dtype == np.float16), _lib.ptr(f), B, ld, hop, silence,
                                            _lib.ptr(pcm), total - 1, _lib.ptr(off), _lib.stream(a.device)), "ctts_pcm16_concat")
    pcm, off = pcm.cpu().numpy(), off.cpu().numpy()
    assert off[-1] == -total and (off[:-1] == want_off[:-1]).all()
    assert (pcm[:total - 1] == want[:-1]).all() and (pcm[total - 1:] == 0x5A5A).all()


def test_best_of_n_through_the_model(hip_lib_path):
    """Three Tacotron2.inference passes of the non-default golden model, 2 texts (40 and 12 symbols) x 3 candidates that differ
    in their prenet dropout, through BestOfN; the restatement is fed the DEVICE's outputs, lengths and metrics copied to the
    host, so the test does not depend on the decoder's bits."""
    import json
    from cookietts_amd import BestOfN, get_first_over_thresh, synthetic
    from cookietts_amd.alignment import metric_table
    from cookietts_amd.tacotron2 import Tacotron2
    g = np.load(os.path.join(GOLDEN, "tacotron_small.npz"))
    hp = synthetic.tacotron_hparams(**synthetic.TACOTRON_SMALL_OVERRIDES)
    shapes = json.load(open(os.path.join(GOLDEN, "tacotron_small_state_shapes.json")))
    m = Tacotron2(hp)
    m.load_state_dict(synthetic.to_torch(synthetic.tacotron_state_dict(hp, seed=int(g["seed"]), shapes=shapes)))
    m = m.cuda().eval()
    N, P, pick = 2, 3, [0, 2]
    rep = lambda k: torch.from_numpy(g[k][pick]).cuda().repeat_interleave(P, dim=0)
    tl = torch.from_numpy(g["lengths"][pick]).cuda()
    kw = dict(max_attempts=64, target_score=50.0)
    best = BestOfN(N, P, hp.n_mel_channels, 24, keep_alignments=True, **kw)
    loop = RetryLoop(N, P, **kw)
    for n, (steps, mode) in enumerate(((24, 'thresh'), (20, 'thresh'), (22, 'max'))):
        masks = synthetic.prenet_dropout_masks(steps, N * P, hp.prenet_dim, seed=100 + n)
        out = m.inference(rep("text"), rep("lengths"), rep("speakers"), rep("torchmoji"), keep_masks=masks, fixed_steps=steps)
        assert out["pred_mel_postnet"].shape == (N * P, hp.n_mel_channels, steps)
        # passes 0, 1: no gate reaches 2.0, every length is T - 1 (utils.py:51); pass 2: wherever the gate peaks (:567)
        st, scores, detail = best.update(out, tl, gate_threshold=2.0, end_mode=mode, return_detail=True)
        ol = get_first_over_thresh(out["pred_gate"], 2.0) if mode == 'thresh' else out["pred_gate"].argmax(dim=1).to(torch.int32)
        metrics = metric_table(out["alignments"], input_lengths=tl.repeat_interleave(P), output_lengths=ol)
        host = [out[k].cpu().numpy() for k in ("pred_mel_postnet", "pred_gate", "alignments")]
        st_ref, sc_ref, det_ref = loop.update(*host, metrics.cpu().numpy(), ol.cpu().numpy(), g["lengths"][pick])
        print("pass", n, "lengths", ol.tolist(), "scores", sc_ref.tolist())
        assert n > 1 or np.isfinite(sc_ref).all()                # (a length of 0 in pass 2 makes the metrics, and the score, NaN)
        for got, ref in ((scores.cpu().numpy(), sc_ref), (detail.cpu().numpy(), det_ref)):
            nan = np.isnan(ref)                                  # a NaN's payload is not compared (test_a_nan_metric_never_wins)
            assert (np.isnan(got) == nan).all() and (bits(got)[~nan] == bits(ref)[~nan]).all()
        assert tuple(st)[:2] == tuple(st_ref)[:2] and tuple(st)[3:] == tuple(st_ref)[3:]
        assert bits(st.min_best_score) == bits(st_ref.min_best_score) and best.done == bool(st_ref.done)
    assert (bits(best.best_scores().cpu().numpy()) == bits(loop.best_score)).all()
    info = best.best_detail()
    assert [(d["pass"], d["row"]) for d in info] == loop.best_where
    assert all(bits(d["weighted_score"]) == bits(loop.best_detail[j][0]) for j, d in enumerate(info))
    mel, lengths = best.vocoder_batch()
    want, want_len = loop.vocoder_batch()
    assert mel.shape == want.shape and (mel.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all()
    assert (lengths.cpu().numpy() == want_len).all()
    al = best.best_alignments().cpu().numpy()
    for j, gen in enumerate(loop.best_generations):
        assert (al[j, :gen[2].shape[0]] == gen[2]).all()
    best.reset()
    assert not best.done and best.status.n_without_winner == N and (best.best_scores() == -1e5).all()
