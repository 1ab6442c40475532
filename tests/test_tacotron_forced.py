"""Teacher-forced Tacotron2 (``Tacotron2.forward`` / ``Decoder.forward``, model.py:769-849, 976-1028 in eval mode: what GTA.py
runs) on the batched decoder: ``ctts_taco_prenet_frames_f32`` -> ``ctts_taco_decoder_steps_forced_f32`` ->
``ctts_taco_project_frames_f32``.

References: the reference's own ``Tacotron2.forward`` outputs (tests/golden/tacotron_forced_*.npz, make_golden_taco_forced.py) at
the project's mel bound; the free-running ``inference`` of the same build fed back as ground truth (frame / mask alignment);
float64 evaluations for the two one-shot operators alone."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from cookietts_amd import synthetic
import tacotron_forced_restatement as fr

MEL_TOL = 1e-4            # BASELINE.json: mel L_inf <= 1e-4 (as in test_tacotron.py)
CASES = ["default", "small", "init"]
E_ARG = -1
SENTINEL = -12345.5
# the keys MEL_TOL is asserted on (the gate through its sigmoid; the raw logits' L_inf is printed)
TOL_KEYS = ("pred_mel", "pred_mel_postnet", "alignments", "encoder_outputs")


def _hp_sd(case, g):
    small = case == "small"
    hp = synthetic.tacotron_hparams(**(synthetic.TACOTRON_SMALL_OVERRIDES if small else {}))
    shapes = json.load(open(os.path.join(GOLDEN, "tacotron_small_state_shapes.json" if small else "tacotron_state_shapes.json")))
    return hp, synthetic.tacotron_state_dict(hp, seed=int(g["seed"]), shapes=shapes)


_REF = {}


def _case(case):
    """(golden, hparams, state dict), loaded once and shared (never modified)."""
    if case not in _REF:
        g = fr.load_golden(case)
        _REF[case] = (g,) + _hp_sd(case, g)
    return _REF[case]


def _sig(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def _compare(out, g, what, keys=TOL_KEYS + ("pred_sylps", "pred_sylps_mu", "pred_sylps_logvar", "hidden_att_contexts")):
    for k in keys:
        a, b = np.asarray(out[k]), g[k]
        assert a.shape == b.shape, (k, a.shape, b.shape)
        err = float(np.abs(a - b).max())
        print(f"{what} {k}: L_inf {err:.3e}")
        assert err < MEL_TOL, (what, k, err)
    print(f"{what} pred_gate_logits: L_inf {np.abs(out['pred_gate_logits'] - g['pred_gate_logits']).max():.3e} (not asserted)")
    assert np.abs(_sig(out["pred_gate_logits"]) - _sig(g["pred_gate_logits"])).max() < MEL_TOL


# ------------------------------------------------------------------------------------------------ CPU ----
@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_reference_golden(case):
    """The teacher-forced loop restated with the oracle's stage functions against the reference's own Tacotron2.forward: all
    nine dict keys (and the bottlenecked memory the decoder returns).  Pins the goldens and the restatement."""
    g, hp, sd = _case(case)
    assert g["gt_mel"].shape[2] == (9 if case == "init" else 37) and ("init_mel" in g) == (case == "init")
    for b, n in enumerate(g["mel_lengths"]):
        assert not g["gt_mel"][b, :, n:].any() and g["gt_mel"][b, :, :n].any()
    out = fr.tacotron_forward(sd, hp, g["gt_mel"], g["text"], g["lengths"], g["speakers"], g["gt_sylps"], g["torchmoji"],
                              g["masks"], g.get("init_mel"))
    assert set(fr.DICT_KEYS) <= set(out) and set(fr.DICT_KEYS) <= set(g)
    _compare(out, g, f"restatement {case}")
    assert np.abs(out["memory"] - g["memory"]).max() < MEL_TOL
    R = hp.windowed_attention_range
    assert ((g["alignments"] > 0).sum(axis=2) <= 2 * R + 1).all() and np.allclose(g["alignments"].sum(axis=2), 1.0, atol=1e-5)
    if case != "init":
        assert g["lengths"][2] < 2 * R + 1 or case == "small"       # default: a text shorter than the 33-token window


def _cfg(**over):
    from cookietts_amd import _lib
    kw = dict(n_mel_channels=80, memory_in_dim=1313, memory_dim=512, attention_dim=128, attention_rnn_dim=1280,
              decoder_rnn_dim=1024, second_decoder_rnn_dim=1024, prenet_dim=256, location_n_filters=32,
              location_kernel_size=31, window_range=16)
    kw.update(over)
    return _lib.TacoDecoderConfig(**kw)


def test_symbols_are_exported_declared_and_typed(hip_lib_path):
    from cookietts_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "cookietts_hip.h")).read()
    for name in ("ctts_taco_prenet_frames_f32", "ctts_taco_decoder_steps_forced_f32", "ctts_taco_project_frames_f32",
                 "ctts_taco_prenet_frames_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and (name + "(") in header, name
    assert lib.ctts_abi_version() == 7


def test_argument_refusals_come_before_any_launch(hip_lib_path):
    """Made-up, aligned, never dereferenced addresses: every refusal is CTTS_E_ARG with its message, without a GPU."""
    from cookietts_amd import _lib
    lib = _lib.lib()
    cfg = _cfg()
    assert lib.ctts_taco_decoder_max_batch(C.byref(cfg)) == 256
    pk, fr_, km, out, al, hid, ws, mel, gate = (C.c_void_p(4096 * i) for i in range(1, 10))
    B, T, TXT = 5, 7, 40
    P = 256
    assert lib.ctts_taco_prenet_frames_bytes(C.byref(cfg), B, T) == T * 16 * P * 4           # 5 rows -> one 16-row tile
    assert lib.ctts_taco_prenet_frames_bytes(C.byref(cfg), 18, T) == T * 32 * P * 4
    assert lib.ctts_taco_prenet_frames_bytes(C.byref(cfg), 70, T) == T * 128 * P * 4
    assert lib.ctts_taco_prenet_frames_bytes(C.byref(cfg), 257, T) == 0 and b"batch=257" in lib.ctts_last_error()
    nbytes = T * 16 * P * 4
    # --- prenet frames
    good = [pk, fr_, None, km, out, nbytes, B, T, None]
    for i in (0, 1, 3, 4):
        a = list(good); a[i] = None
        assert lib.ctts_taco_prenet_frames_f32(C.byref(cfg), *a) == E_ARG and b"NULL pointer" in lib.ctts_last_error()
    for a, msg in (([pk, fr_, None, km, out, nbytes, 0, T, None], b"batch=0"), ([pk, fr_, None, km, out, nbytes, 257, T, None], b"batch=257"),
                   ([pk, fr_, None, km, out, nbytes, B, 0, None], b"n_frames=0"),
                   ([pk, fr_, None, km, out, nbytes - 4, B, T, None], b"bytes < required")):
        assert lib.ctts_taco_prenet_frames_f32(C.byref(cfg), *a) == E_ARG and msg in lib.ctts_last_error(), msg
    # --- forced steps
    need = lib.ctts_taco_decoder_workspace_bytes(C.byref(cfg), B, TXT)
    assert need > 0
    good = [pk, out, al, hid, B, TXT, 0, T, T, ws, need, None]
    for i in (0, 1, 2, 3, 9):
        a = list(good); a[i] = None
        assert lib.ctts_taco_decoder_steps_forced_f32(C.byref(cfg), *a) == E_ARG and b"NULL pointer" in lib.ctts_last_error()
    for edit, msg in (({4: 0}, b"batch=0"), ({4: 257}, b"batch=257"), ({6: 3, 7: 5}, b"step0=3 n_steps=5 max_steps=7"),
                      ({6: -1}, b"step0=-1"), ({7: -1}, b"n_steps=-1"), ({5: 0}, b"text_len=0"),
                      ({10: need - 4}, b"bytes < required")):
        a = list(good)
        for i, v in edit.items():
            a[i] = v
        assert lib.ctts_taco_decoder_steps_forced_f32(C.byref(cfg), *a) == E_ARG and msg in lib.ctts_last_error(), msg
    # --- project frames
    good = [pk, hid, mel, gate, B, T, None]
    for i in range(4):
        a = list(good); a[i] = None
        assert lib.ctts_taco_project_frames_f32(C.byref(cfg), *a) == E_ARG and b"NULL pointer" in lib.ctts_last_error()
    for edit, msg in (({4: 0}, b"batch=0"), ({5: 0}, b"n_frames=0")):
        a = list(good)
        for i, v in edit.items():
            a[i] = v
        assert lib.ctts_taco_project_frames_f32(C.byref(cfg), *a) == E_ARG and msg in lib.ctts_last_error(), msg
    assert lib.ctts_taco_project_frames_f32(None, *good) == E_ARG


def test_shapes_without_the_batched_form_are_refused(hip_lib_path):
    from cookietts_amd import _lib
    lib = _lib.lib()
    cfg = _cfg(prenet_dim=252)                      # not a multiple of 16: VALU / persistent forms only
    assert lib.ctts_taco_decoder_max_batch(C.byref(cfg)) == 4
    pk, a1, a2, a3, ws = (C.c_void_p(4096 * i) for i in range(1, 6))
    need = lib.ctts_taco_decoder_workspace_bytes(C.byref(cfg), 2, 40)
    assert need > 0
    assert lib.ctts_taco_decoder_steps_forced_f32(C.byref(cfg), pk, a1, a2, a3, 2, 40, 0, 3, 3, ws, need, None) == E_ARG
    assert b"no batched form" in lib.ctts_last_error()
    assert lib.ctts_taco_prenet_frames_bytes(C.byref(cfg), 2, 3) == 0 and b"no batched form" in lib.ctts_last_error()
    assert lib.ctts_taco_prenet_frames_f32(C.byref(cfg), pk, a1, None, a2, a3, 1 << 20, 2, 3, None) == E_ARG
    assert b"no batched form" in lib.ctts_last_error()


def test_host_refusals_name_the_option_and_the_defaulting_quirk():
    """On a CPU-constructed model: every refusal is raised before anything touches a device."""
    from cookietts_amd.tacotron2 import Tacotron2
    hp = synthetic.tacotron_hparams(**synthetic.TACOTRON_SMALL_OVERRIDES)
    m = Tacotron2(hp).eval()
    B, T = 2, 6
    gt = torch.zeros(B, hp.n_mel_channels, T)
    args = (gt, torch.tensor([T, T]), torch.zeros(B, 5, dtype=torch.long), torch.tensor([5, 5]), torch.zeros(B, dtype=torch.long),
            torch.ones(B), torch.zeros(B, hp.torchMoji_attDim))
    gta = dict(teacher_force_till=0, p_teacher_forcing=1.0, drop_frame_rate=0.0)
    m.train()
    with pytest.raises(NotImplementedError, match="self.training"):
        m(*args, **gta)
    with pytest.raises(NotImplementedError, match="self.training"):
        m.decoder(torch.zeros(B, 5, m.decoder._memory_in_dim), gt, torch.tensor([5, 5]))
    m.eval()
    with pytest.raises(NotImplementedError, match="pres_prev_state"):
        m(*args, torch.tensor([[0.0], [1.0]]), **gta)
    with pytest.raises(NotImplementedError, match="p_teacher_forcing=0.5"):
        m(*args, **dict(gta, p_teacher_forcing=0.5))
    with pytest.raises(NotImplementedError, match="p_teacher_forcing=0.9"):
        m(*args, teacher_force_till=T - 2, p_teacher_forcing=0.9)
    m.decoder.dump_attention_weights = True
    with pytest.raises(NotImplementedError, match="dump_attention_weights"):
        m(*args, **gta)
    m.decoder.dump_attention_weights = False
    # teacher_force_till >= T - 1 forces every step whatever p_teacher_forcing is (model.py:830): passes the checks
    m.decoder.check_forced(T, None, T - 1, 0.0)
    m.decoder.check_forced(T, torch.zeros(B, 1), 0, 1.0)
    # the options the constructor refuses
    for over, what in ((dict(hide_startstop_tokens=True), "hide_startstop_tokens"), (dict(context_frames=2), "context_frames")):
        with pytest.raises(NotImplementedError, match=what):
            Tacotron2(synthetic.tacotron_hparams(**over))
    # model.py:980-981, as written: the second line tests the value the first one has just assigned
    own_p, own_t = 0.7, 20
    res = Tacotron2.resolve_teacher_forcing
    for tft, ptf in ((None, None), (None, 0.3), (0, None), (0, 1.0), (5, 0.25)):
        p = own_p if tft is None else ptf                  # the reference's two lines
        t = own_t if p is None else tft
        assert res(own_p, own_t, tft, ptf) == (p, t)
    assert res(own_p, own_t, None, 0.3) == (0.7, None) and res(own_p, own_t, 0, None) == (None, 20)
    assert (m.p_teacher_forcing, m.teacher_force_till, m.drop_frame_rate) == (hp.p_teacher_forcing, hp.teacher_force_till,
                                                                              hp.drop_frame_rate)
    with pytest.raises(TypeError, match="teacher_force_till is None"):        # both left to their defaults: as in the reference
        m(*args)


# ------------------------------------------------------------------------------------------------ GPU ----
_MODELS = {}


def _model(case):
    from cookietts_amd.tacotron2 import Tacotron2
    if case not in _MODELS:
        g, hp, sd = _case(case)
        m = Tacotron2(hp)
        m.load_state_dict(synthetic.to_torch(sd))
        _MODELS[case] = m.cuda().eval()
    return _MODELS[case]


def _forward(m, g, **kw):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = m(t(g["gt_mel"]), t(g["mel_lengths"]), t(g["text"]), t(g["lengths"]), t(g["speakers"]), t(g["gt_sylps"]), t(g["torchmoji"]),
            None, None, t(g["init_mel"]) if "init_mel" in g else None, teacher_force_till=0, p_teacher_forcing=1.0,
            drop_frame_rate=0.0, keep_masks=g["masks"], **kw)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_hip_forward_matches_reference_golden(hip_lib_path, case):
    """Tacotron2.forward against the reference's own, and return_hidden_state=True against its hidden_att_contexts."""
    g, hp, sd = _case(case)
    m = _model(case)
    out = _forward(m, g, return_hidden_state=True)
    assert sorted(out) == sorted(fr.DICT_KEYS)
    _compare(out, g, f"hip {case}")
    if case == "default":                                # return_hidden_state=False: the key is there, None, as in the reference
        assert _forward(m, g)["hidden_att_contexts"] is None


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 70])
def test_forward_on_its_own_free_running_frames_reproduces_them(hip_lib_path, B):
    """Frame and mask alignment: inference(fixed_steps=T, keep_masks=m) free-running, then forward with that pred_mel as gt_mel
    and the same masks - step t of either reads frame t - 1 and mask t, so mel, alignments and sigmoid(gate) agree within
    MEL_TOL.  B = 3: one 16-row tile, pipelined schedule; B = 70: 128 padded rows, plain schedule.
    (The free-running frames of the synthetic weights are small, |mel| < 0.1, so the prenet moves little here: masks shifted by
    one step move the mel by 2e-4 - outside the bound, which is all that is asserted about it; the figure is printed.  On the
    goldens, whose ground-truth frames are log-mel sized, the same slip is off by orders of magnitude.)"""
    g, hp, sd = _case("default")
    m = _model("default")
    T, TXT = 24, 40
    rng = np.random.default_rng(B)
    lengths = np.sort(rng.integers(12, TXT + 1, B))[::-1].copy()
    lengths[0] = TXT
    text = rng.integers(1, hp.n_symbols, (B, TXT))
    for b in range(B):
        text[b, lengths[b]:] = 0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    spk, tm = t(rng.integers(0, 500, B)), t(rng.standard_normal((B, hp.torchMoji_attDim)).astype(np.float32))
    syl = t(rng.uniform(2.5, 6.5, B).astype(np.float32))
    masks = synthetic.prenet_dropout_masks(T, B, hp.prenet_dim, seed=B)
    free = m.inference(t(text), t(lengths), spk, tm, gt_sylps=syl, keep_masks=masks, fixed_steps=T)
    out = m(free["pred_mel"], t(np.full(B, T)), t(text), t(lengths), spk, syl, tm, teacher_force_till=0, p_teacher_forcing=1.0,
            keep_masks=masks)
    for k_forced, a, b in (("pred_mel", out["pred_mel"], free["pred_mel"]), ("alignments", out["alignments"], free["alignments"]),
                           ("sigmoid(gate)", torch.sigmoid(out["pred_gate_logits"]), free["pred_gate"]),
                           ("pred_mel_postnet", out["pred_mel_postnet"], free["pred_mel_postnet"])):
        err = float((a - b).abs().max())
        print(f"B={B} forced vs free-running {k_forced}: L_inf {err:.3e}")
        assert a.shape == b.shape and err < MEL_TOL, (k_forced, err)
    # the comparison above can fail: masks shifted by one step leave the bound
    shifted = np.roll(masks, 1, axis=0)
    off = m(free["pred_mel"], t(np.full(B, T)), t(text), t(lengths), spk, syl, tm, teacher_force_till=0, p_teacher_forcing=1.0,
            keep_masks=shifted)
    moved = float((off["pred_mel"] - free["pred_mel"]).abs().max())
    print(f"B={B} masks shifted by one step: L_inf {moved:.3e}")
    assert moved > MEL_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["pipelined", "plain"])
def test_blocks_rows_and_repeats(hip_lib_path, tuning, schedule):
    """B = 18 (two 16-row tiles, ragged), T = 21, Decoder.forward.  Blocks of 8 / 8 / 5 steps (step0 > 0) equal one block of 21
    bit for bit; a repeated call is bit-equal (workspace reuse; padded rows of prenet_all stay zero); the first 17 rows of the
    18-row call equal a 17-row call bit for bit (same column-tile shape).  Against the same utterances decoded in a batch of
    their own the bound is the one test_tacotron_batched.py uses for that comparison, 2e-5; whether it is met bit for bit is
    printed.  That comparison also holds the loop's two forms to each other: 2 rows -> a 16-row tile and five launches per
    step; 18 rows -> 32 padded rows and four (the second decoder RNN and the next step's attention RNN as roles of one launch),
    with other launch shapes, whose summation order may differ.  Both schedules of the step: the pipelined one the library picks at
    these sizes and the plain one (CTTS_TACO_BG_NO_PIPE)."""
    if schedule == "plain":
        tuning.set("CTTS_TACO_BG_NO_PIPE")
    g, hp, sd = _case("default")
    dec = _model("default").decoder
    B, T, TXT = 18, 21, 45
    rng = np.random.default_rng(18)
    mem = torch.from_numpy((rng.standard_normal((B, TXT, synthetic.tacotron_memory_in_dim(hp))) * 0.5).astype(np.float32)).cuda()
    lens = torch.from_numpy(np.sort(rng.integers(10, TXT + 1, B))[::-1].copy()).cuda()
    gt = torch.from_numpy(synthetic.synthetic_mel(B, T, hp.n_mel_channels, seed=18)).cuda()
    masks = synthetic.prenet_dropout_masks(T, B, hp.prenet_dim, seed=18)
    run = lambda sl=slice(None): dec(mem[sl], gt[sl], lens[sl], keep_masks=masks[:, :, sl], return_hidden_state=True)
    one = run()
    assert one[0].shape == (B, hp.n_mel_channels, T) and one[3].shape == (B, hp.second_decoder_rnn_dim + hp.memory_bottleneck_dim, T)
    assert all(bool(torch.isfinite(x).all()) for x in one)
    again = run()
    assert all(torch.equal(a, b) for a, b in zip(one, again))
    dec.forced_chunk = 8
    try:
        blocks = run()
    finally:
        dec.forced_chunk = None
    assert all(torch.equal(a, b) for a, b in zip(one, blocks))
    first17 = run(slice(0, 17))
    assert all(torch.equal(a[:17], b) for a, b in zip(one, first17))
    alone = run(slice(3, 5))
    d = max(float((a[3:5] - b).abs().max()) for a, b in zip(one[:3], alone[:3]))
    print(f"rows 3-4 of 18 vs a batch of their own: L_inf {d:.2e}, bit-equal: {all(torch.equal(a[3:5], b) for a, b in zip(one, alone))}")
    assert d < 2e-5


@pytest.mark.gpu
def test_prenet_frames_against_float64(hip_lib_path):
    """B = 5, T = 7, n_mel = 80, P = 256.  |y - y64| <= (n_mel + P) * 2^-23 * (sum of the absolute products through both layers):
    one rounding (2^-24 relative) per step of a chain of n_mel, then P, products, with a factor 2 for the growth of the partial
    sums' bound (as test_depthwise_operator_against_float64 derives its bound).  Nothing outside [T][NB][P] is written; rows
    [B, NB) are zeros; all-zero masks give exactly zero."""
    from cookietts_amd import _lib
    lib = _lib.lib()
    g, hp, sd = _case("default")
    dec = _model("default").decoder
    blob, cfg = dec._ensure_packed(torch.device("cuda", torch.cuda.current_device())), dec.c_config()
    B, T, n_mel, P = 5, 7, hp.n_mel_channels, hp.prenet_dim
    assert (n_mel, P) == (80, 256)
    nbytes = lib.ctts_taco_prenet_frames_bytes(C.byref(cfg), B, T)
    NB = nbytes // (4 * T * P)
    assert NB == 16
    frames = synthetic.synthetic_mel(B, T, n_mel, seed=9)
    init = (np.random.default_rng(9).standard_normal((B, n_mel)) * 2 - 5).astype(np.float32)
    masks = synthetic.prenet_dropout_masks(T, B, P, seed=9)
    w1 = sd["decoder.prenet.layers.0.linear_layer.weight"].astype(np.float64)
    w2 = sd["decoder.prenet.layers.1.linear_layer.weight"].astype(np.float64)
    GUARD = 1024
    stream = _lib.stream(blob.device)
    for go in (None, init):
        buf = torch.full((GUARD + nbytes // 4 + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        out = buf[GUARD:GUARD + nbytes // 4]
        tf, tk = torch.from_numpy(frames).cuda(), torch.from_numpy(masks).cuda()
        ti = None if go is None else torch.from_numpy(go).cuda()
        _lib.check(lib.ctts_taco_prenet_frames_f32(C.byref(cfg), _lib.ptr(blob), _lib.ptr(tf), _lib.ptr(ti), _lib.ptr(tk), _lib.ptr(out),
                                                  nbytes, B, T, stream), "ctts_taco_prenet_frames_f32")
        got = buf.cpu().numpy()
        assert np.all(got[:GUARD] == np.float32(SENTINEL)) and np.all(got[-GUARD:] == np.float32(SENTINEL))
        got = got[GUARD:-GUARD].reshape(T, NB, P)
        assert not got[:, B:].any()
        x = np.concatenate([(np.zeros((B, n_mel)) if go is None else go.astype(np.float64))[None],
                            frames.astype(np.float64).transpose(2, 0, 1)[:-1]], axis=0)               # [T, B, n_mel]: step t reads frame t - 1
        k1, k2 = masks[:, 0].astype(np.float64) * 2.0, masks[:, 1].astype(np.float64) * 2.0
        a1 = np.maximum(x @ w1.T, 0) * k1
        y64 = np.maximum(a1 @ w2.T, 0) * k2
        mag1 = (np.abs(x) @ np.abs(w1).T) * k1
        mag = (mag1 @ np.abs(w2).T) * k2
        diff = np.abs(got[:, :B].astype(np.float64) - y64)
        bound = (n_mel + P) * 2.0 ** -23 * mag
        ratio = float((diff[bound > 0] / bound[bound > 0]).max())
        print(f"prenet frames (go frame {'zeros' if go is None else 'given'}): max |y - y64| / bound = {ratio:.3e}, |y| max {np.abs(y64).max():.3f}")
        assert ratio <= 1.0 and not diff[bound == 0].any() and np.abs(y64).max() > 0.1
    zero = torch.zeros_like(tk)
    _lib.check(lib.ctts_taco_prenet_frames_f32(C.byref(cfg), _lib.ptr(blob), _lib.ptr(tf), None, _lib.ptr(zero), _lib.ptr(out), nbytes,
                                              B, T, stream), "ctts_taco_prenet_frames_f32")
    assert not bool(out.any())


@pytest.mark.gpu
def test_project_frames_against_float64(hip_lib_path):
    """B = 5, T = 7: |y - y64| <= (Rd2 + Dm) * 2^-23 * (|b| + sum |w| |x|) per element, mel rows and the gate row; nothing
    outside the two outputs is written."""
    from cookietts_amd import _lib
    lib = _lib.lib()
    g, hp, sd = _case("default")
    dec = _model("default").decoder
    blob, cfg = dec._ensure_packed(torch.device("cuda", torch.cuda.current_device())), dec.c_config()
    B, T, n_mel, D = 5, 7, hp.n_mel_channels, hp.second_decoder_rnn_dim + hp.memory_bottleneck_dim
    hidden = np.random.default_rng(10).standard_normal((B, D, T)).astype(np.float32)
    w = np.concatenate([sd["decoder.linear_projection.linear_layer.weight"], sd["decoder.gate_layer.linear_layer.weight"]]).astype(np.float64)
    b = np.concatenate([sd["decoder.linear_projection.linear_layer.bias"], sd["decoder.gate_layer.linear_layer.bias"]]).astype(np.float64)
    GUARD = 256
    bm = torch.full((GUARD + B * n_mel * T + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    bg = torch.full((GUARD + B * T + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    th = torch.from_numpy(hidden).cuda()
    _lib.check(lib.ctts_taco_project_frames_f32(C.byref(cfg), _lib.ptr(blob), _lib.ptr(th), _lib.ptr(bm[GUARD:]), _lib.ptr(bg[GUARD:]), B, T,
                                               _lib.stream(blob.device)), "ctts_taco_project_frames_f32")
    gm, gg = bm.cpu().numpy(), bg.cpu().numpy()
    for a in (gm, gg):
        assert np.all(a[:GUARD] == np.float32(SENTINEL)) and np.all(a[-GUARD:] == np.float32(SENTINEL))
    got = np.concatenate([gm[GUARD:-GUARD].reshape(B, n_mel, T), gg[GUARD:-GUARD].reshape(B, 1, T)], axis=1).astype(np.float64)
    y64 = np.einsum("rk,bkt->brt", w, hidden.astype(np.float64)) + b[None, :, None]
    mag = np.einsum("rk,bkt->brt", np.abs(w), np.abs(hidden).astype(np.float64)) + np.abs(b)[None, :, None]
    ratio = float((np.abs(got - y64) / (D * 2.0 ** -23 * mag)).max())
    print(f"project frames: max |y - y64| / bound = {ratio:.3e}")
    assert ratio <= 1.0


@pytest.mark.gpu
def test_inference_is_bit_equal_before_and_after_a_forward_call(hip_lib_path):
    """The decoder workspaces are shared between the two entry points of a model."""
    g, hp, sd = _case("default")
    m = _model("default")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n = 12
    masks = synthetic.prenet_dropout_masks(n, 3, hp.prenet_dim, seed=77)
    args = (t(g["text"]), t(g["lengths"]), t(g["speakers"]), t(g["torchmoji"]))
    before = m.inference(*args, keep_masks=masks, fixed_steps=n)
    fwd = _forward(m, g)
    after = m.inference(*args, keep_masks=masks, fixed_steps=n)
    assert sorted(before) == sorted(after)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert np.abs(fwd["pred_mel"] - g["pred_mel"]).max() < MEL_TOL
