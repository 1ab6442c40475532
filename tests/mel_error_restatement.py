"""numpy restatement of the vocoder validation score (cookietts_amd/mel_error.py, csrc/mel_error.hip): the per-file, per-window log-mel
MSE / MAE of ``_4_mtw/waveglow/train.py:258-278`` with ``TacotronSTFT.mel_spectrogram`` (``utils/audio/stft.py:79-111, 180-207``), and
the framing of ``hifigan/nvSTFT.py:92-101`` under ``framing="nv"``.  Not a test module.

Two arms: ``np.float32`` follows the reference's arithmetic (the windowed DFT as a float32 matrix product with the float32 basis, float32
mel projection, log, float32 means; the totals of :276-278 as Python floats) and is pinned to the reference's own outputs
(tests/golden/mel_error_*.npz) by tests/test_mel_error.py; ``np.float64`` (rfft of the windowed frames, everything in double) is the
truth of the GPU tests, with ``e32 = |float32 arm - float64 arm|`` as the reference's own error in the project's bound.
"""
import os

import numpy as np

from oracle import stft_oracle as so

F32, F64 = np.float32, np.float64
FACTOR = 8                      # the project's factor on e32 (tests/ax_cond_f64_restatement.py:50)
EPS32 = 2.0 ** -23
COLUMNS = ("n_frames", "SAE", "SSE", "MAE", "MSE")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> the constructor arguments, the ground-truth and generated lengths (samples)
CASES = {
    # 131 frames (crosses a 128-frame tile; length no multiple of hop), 128 frames (exactly one tile), 9 frames; no crop, a crop by
    # under one frame, a crop by many frames; 33 / 49 bins are no multiple of 16, 12 mels no multiple of the MFMA tile
    "small": dict(windows=(64, 96), hop_length=16, sampling_rate=8000, n_mel_channels=12, mel_fmin=0.0, mel_fmax=4000.0,
                  framing="tacotron", gt_lengths=(2085, 2032, 130), pred_lengths=(2085, 2100, 400)),
    "real": dict(windows=(1200, 2400), hop_length=600, sampling_rate=48000, n_mel_channels=160, mel_fmin=0.0, mel_fmax=16000.0,
                 framing="tacotron", gt_lengths=(4800, 7300), pred_lengths=(4800, 7300)),
    "nv_small": dict(windows=(64,), win_lengths=(48,), hop_length=16, sampling_rate=8000, n_mel_channels=12, mel_fmin=0.0,
                     mel_fmax=4000.0, framing="nv", gt_lengths=(2048, 2048), pred_lengths=(2048, 2048)),
    "nv_real": dict(windows=(1024,), win_lengths=(1024,), hop_length=256, sampling_rate=22050, n_mel_channels=80, mel_fmin=0.0,
                    mel_fmax=8000.0, framing="nv", gt_lengths=(8192, 8192), pred_lengths=(8192, 8192)),
}
CTOR_KEYS = ("windows", "hop_length", "sampling_rate", "n_mel_channels", "mel_fmin", "mel_fmax", "win_lengths", "framing")


def ctor_args(case):
    return {k: CASES[case][k] for k in CTOR_KEYS if k in CASES[case]}


def bound(e32, y64):
    """The project's parity bound: FACTOR * max(|fp32 reference - fp64 reference|, 4 ulp of the fp64 value)."""
    return FACTOR * np.maximum(np.asarray(e32, F64), 4 * EPS32 * np.abs(np.asarray(y64, F64)))


def signals(case, seed=0):
    """Seeded tones plus noise of amplitude >= 1e-2, below 1 in magnitude: no near-silent bins, so the reference's own float32
    error stays well-behaved.  -> (gt [B, Tg_max], pred [B, Tp_max]) float32, zero beyond each length."""
    c = CASES[case]
    rng = np.random.RandomState(1234 + seed)
    gl, pl = c["gt_lengths"], c["pred_lengths"]
    gt = np.zeros((len(gl), max(gl)), F32)
    pred = np.zeros((len(pl), max(pl)), F32)
    for b in range(len(gl)):
        n = max(gl[b], pl[b])
        t = np.arange(n) / c["sampling_rate"]
        tone = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip((0.3, 0.2, 0.1), rng.uniform(0.02, 0.4, 3) * c["sampling_rate"],
                                                                        rng.uniform(0, 6.28, 3)))
        g = tone + 0.05 * rng.randn(n)
        p = 0.9 * tone + 0.08 * rng.randn(n)
        gt[b, :gl[b]] = np.clip(g[:gl[b]], -0.95, 0.95)
        pred[b, :pl[b]] = np.clip(p[:pl[b]], -0.95, 0.95)
    return gt, pred


def sanitize(x):
    """train.py:259-260: clamp to +-0.999 (NaN stays, +-inf are clamped), then NaN -> 0."""
    x = np.clip(np.asarray(x), -0.999, 0.999)
    return np.where(np.isnan(x), np.zeros_like(x), x)


def reflect_pad(framing, n_fft, hop):
    return int((n_fft - hop) / 2) if framing == "nv" else n_fft // 2


def n_frames(T, n_fft, hop, framing):
    if framing == "nv":
        return (T + 2 * reflect_pad(framing, n_fft, hop) - n_fft) // hop + 1
    return T // hop + 1


def log_mel(x, n_fft, win_length, hop, fb, dtype, framing="tacotron", clamp=1e-5):
    """x [T] -> log-mel [n_mel, frames] in ``dtype``."""
    x = np.asarray(x, dtype)
    pad = reflect_pad(framing, n_fft, hop)
    xp = np.pad(x, pad, mode="reflect")
    frames = n_frames(len(x), n_fft, hop, framing)
    idx = np.arange(frames)[:, None] * hop + np.arange(n_fft)[None, :]
    eps = 1e-9 if framing == "nv" else 0.0
    if dtype == F32:
        basis = so.forward_basis(n_fft, win_length)                           # float32 [2 cutoff, n_fft], window folded in
        ri = basis @ xp[idx].T                                                # float32 [2 cutoff, frames]
        c = n_fft // 2 + 1
        mag = np.sqrt(ri[:c] ** 2 + ri[c:] ** 2 + F32(eps))
    else:
        win = so.pad_center(so.hann_periodic(win_length), n_fft)
        spec = np.fft.rfft(xp[idx].astype(F64) * win[None, :], axis=1).T
        mag = np.sqrt(spec.real ** 2 + spec.imag ** 2 + eps)
    mel = np.asarray(fb, dtype) @ mag.astype(dtype)
    return np.log(np.maximum(mel, dtype(clamp))).astype(dtype)


def score(pred, gt, pred_lengths, gt_lengths, dtype, windows, hop_length, sampling_rate, n_mel_channels=160, mel_fmin=0.0,
          mel_fmax=16000.0, clamp_val=1e-5, win_lengths=None, framing="tacotron", do_sanitize=True, gt_mel=None):
    """The loop of train.py:258-278 over the items of a padded batch -> dict: ``table`` [B, W, 5] float64 (the values of ``dtype``
    widened), ``average_MSE`` / ``average_MAE`` (Python-float totals, :276-278, 294-295), ``l1`` [W], and the lists ``pred_mel``,
    ``gt_mel``, ``mae_spec`` [b][w] of [n_mel, n_frames] arrays.  ``gt_mel`` [B][n_mel, frames]: the ground-truth log-mel itself
    (one window), as hifigan/train.py:208 takes it from its loader."""
    win_lengths = windows if win_lengths is None else win_lengths
    B, W = len(pred_lengths), len(windows)
    table = np.zeros((B, W, 5), F64)
    maps = {"pred_mel": [], "gt_mel": [], "mae_spec": []}
    total_mse = total_mae = total = 0
    fbs = [so.slaney_mel_filterbank(sampling_rate, n, n_mel_channels, mel_fmin, mel_fmax) for n in windows]
    for b in range(B):
        p = np.asarray(pred[b][:pred_lengths[b]], F32)
        p = sanitize(p) if do_sanitize else p
        rows = {k: [] for k in maps}
        for w, (n, wl) in enumerate(zip(windows, win_lengths)):
            if gt_mel is None:
                mg = log_mel(np.asarray(gt[b][:gt_lengths[b]], F32), n, wl, hop_length, fbs[w], dtype, framing, clamp_val)
            else:
                mg = np.asarray(gt_mel[b], dtype)
            mp = log_mel(p, n, wl, hop_length, fbs[w], dtype, framing, clamp_val)[:, :mg.shape[1]]          # :268
            assert mp.shape == mg.shape, (mp.shape, mg.shape)
            d = mp - mg
            mse, mae = float(np.mean(d * d, dtype=dtype)), float(np.mean(np.abs(d), dtype=dtype))
            table[b, w] = (mg.shape[1], float(np.sum(np.abs(d), dtype=dtype)), float(np.sum(d * d, dtype=dtype)), mae, mse)
            total_mae += mae
            total_mse += mse
            total += 1
            rows["pred_mel"].append(mp); rows["gt_mel"].append(mg); rows["mae_spec"].append(np.abs(d))
        for k in maps:
            maps[k].append(rows[k])
    count = table[:, :, 0] * n_mel_channels
    out = {"table": table, "average_MSE": total_mse / total, "average_MAE": total_mae / total,
           "l1": table[:, :, 1].sum(axis=0) / count.sum(axis=0)}
    out.update(maps)
    return out


_CACHE = {}


def load_golden(case):
    """tests/golden/mel_error_<case>.npz, loaded once and shared (never modified)."""
    if case not in _CACHE:
        z = np.load(os.path.join(GOLDEN, f"mel_error_{case}.npz"))
        _CACHE[case] = {k: z[k] for k in z.files}
    return _CACHE[case]


_LIVE = {}


def live(case):
    """(gt, pred, float64 score, float32 score) of a case's seeded signals, computed once and shared (never modified)."""
    if case not in _LIVE:
        c = CASES[case]
        gt, pred = signals(case)
        r = [score(pred, gt, c["pred_lengths"], c["gt_lengths"], dt, **ctor_args(case)) for dt in (F64, F32)]
        _LIVE[case] = (gt, pred, r[0], r[1])
    return _LIVE[case]
