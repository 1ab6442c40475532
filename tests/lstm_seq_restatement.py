"""Packed-sequence LSTM vectorised over the batch, and the Tacotron2 text side built on it.

TEST INFRASTRUCTURE ONLY (numpy; see oracle/waveglow_oracle.py header for the import rule).  ``oracle.tacotron_oracle.encoder``
walks the BiLSTM item by item in Python, which is too slow for 256 utterances; that is the only reason for this second
statement.  It is pinned to the first one and to the reference's own outputs by tests/test_tacotron_text_side.py (CPU):
float32 ``text_side`` reproduces ``encoder_outputs`` / ``pred_sylps`` of tests/golden/tacotron_full.npz within 1e-6 and agrees
with ``oracle.tacotron_oracle.encoder`` on a ragged, unsorted batch.

Semantics (nn.LSTM over a packed sequence, one direction; layers.py:308-372 for the cell): gate order i, f, g, o; item b is
active while ``step < lengths[b]``; it reads and writes time index ``step`` (forward) or ``lengths[b] - 1 - step`` (reverse);
``hn`` is the state after the item's last active step; ``out`` is zero beyond each length (pad_packed_sequence).
Every intermediate is held in ``dtype`` and the weights are cast to ``dtype`` first, so float64 really is float64.
"""
from __future__ import annotations

import numpy as np

from oracle import tacotron_oracle as to

# Deliberately WRONG variants, for the test that proves the parity tests can fail (never used as a reference):
#   "reverse_from_T"  the reverse direction reads / writes time index T - 1 - step instead of len - 1 - step
#   "hn_at_T"         hn is what the output holds at time index T - 1 (the state of step T - 1 of an unpacked run)
MUTATIONS = ("reverse_from_T", "hn_at_T")


def _sigmoid(x, dtype):
    return (dtype(1.0) / (dtype(1.0) + np.exp(-x))).astype(dtype)


def packed_lstm(x, lengths, w_ih, w_hh, b_ih, b_hh, reverse, dtype, *, mutation=None):
    """x [B, T, I], lengths [B] (1 <= len <= T), w_ih [4H, I], w_hh [4H, H], b_ih / b_hh [4H].
    Returns (out [B, T, H] zero beyond each length, hn [B, H])."""
    assert mutation is None or mutation in MUTATIONS, mutation
    x = np.asarray(x).astype(dtype)
    w_ih, w_hh = np.asarray(w_ih).astype(dtype), np.asarray(w_hh).astype(dtype)
    b_ih, b_hh = np.asarray(b_ih).astype(dtype), np.asarray(b_hh).astype(dtype)
    lengths = np.asarray(lengths).astype(np.int64)
    B, T, _ = x.shape
    H = w_hh.shape[1]
    assert w_ih.shape[0] == w_hh.shape[0] == 4 * H and lengths.shape == (B,) and lengths.min() >= 1 and lengths.max() <= T
    xp = (x @ w_ih.T + b_ih + b_hh).astype(dtype)                               # input projection of every step [B, T, 4H]
    w_hh_t = np.ascontiguousarray(w_hh.T)
    h = np.zeros((B, H), dtype)
    c = np.zeros((B, H), dtype)
    out = np.zeros((B, T, H), dtype)
    rows = np.arange(B)
    for step in range(T):
        active = step < lengths
        if not active.any():
            break
        last = (T if mutation == "reverse_from_T" else lengths) - 1
        tb = np.where(active, last - step if reverse else step, 0)
        g = (xp[rows, tb] + h @ w_hh_t).astype(dtype)
        i, f, gg, o = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
        c2 = (_sigmoid(f, dtype) * c + _sigmoid(i, dtype) * np.tanh(gg)).astype(dtype)
        h2 = (_sigmoid(o, dtype) * np.tanh(c2)).astype(dtype)
        act = active[:, None]
        c = np.where(act, c2, c)
        h = np.where(act, h2, h)                                                # inactive items keep their state: hn = h at the end
        out[rows[active], tb[active]] = h2[active]
    hn = out[:, T - 1].copy() if mutation == "hn_at_T" else h
    assert out.dtype == dtype and hn.dtype == dtype
    return out, hn


def bilstm(x, lengths, fwd, bwd, dtype, *, mutation=None):
    """Both directions: ``fwd`` / ``bwd`` = (w_ih, w_hh, b_ih, b_hh).  Returns (out [B, T, 2H], hn [B, 2H]), [forward | backward]."""
    of, hf = packed_lstm(x, lengths, *fwd, False, dtype, mutation=mutation)
    ob, hb = packed_lstm(x, lengths, *bwd, True, dtype, mutation=mutation)
    return np.concatenate([of, ob], axis=2), np.concatenate([hf, hb], axis=1)


def cast_state_dict(sd, dtype):
    return {k: (np.asarray(v).astype(dtype) if np.issubdtype(np.asarray(v).dtype, np.floating) else np.asarray(v))
            for k, v in sd.items()}


def encoder_side(sd, hp, text, lengths, speakers, dtype):
    """model.py:283-316 in eval mode: embedding gather, conv + BatchNorm + LeakyReLU layers (the oracle's own ``_conv1d_same`` /
    ``_bn_eval``), packed BiLSTM, sylps head.  Returns (encoder_outputs [B, T, enc], hn [B, enc], pred_sylps [B, 1]) in ``dtype``."""
    sd = cast_state_dict(sd, dtype)
    text, speakers = np.asarray(text), np.asarray(speakers)
    with to.precision(dtype):
        emb = sd["embedding.weight"][text].transpose(0, 2, 1)
        spk = sd["encoder.encoder_speaker_embedding.weight"][speakers][:, :, None]
        x = np.concatenate([emb, np.repeat(spk, emb.shape[2], axis=2)], axis=1).astype(dtype)
        for i in range(hp.encoder_n_convolutions):
            p = f"encoder.convolutions.{i}"
            x = to._bn_eval(to._conv1d_same(x, sd[p + ".0.conv.weight"], sd[p + ".0.conv.bias"]), sd, p + ".1")
            x = np.where(x > 0, x, dtype(0.01) * x).astype(dtype)
        params = [tuple(sd[f"encoder.lstm.{n}_l0{sfx}"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                  for sfx in ("", "_reverse")]
        out, hn = bilstm(x.transpose(0, 2, 1), lengths, params[0], params[1], dtype)
        sylps = (hn @ sd["encoder.sylps_layer.linear_layer.weight"].T + sd["encoder.sylps_layer.linear_layer.bias"]).astype(dtype)
    return out, hn, sylps


def assemble(sd, hp, encoder_outputs, pred_sylps, speakers, torchmoji, gt_sylps, dtype):
    """model.py:1051-1068: the decoder's memory from the encoder outputs and the per-utterance columns (the oracle's own
    ``memory_assemble``); ``gt_sylps`` [B] feeds the SylpsNet instead of the predicted value where given (model.py:1058)."""
    sd = cast_state_dict(sd, dtype)
    syl_in = pred_sylps if gt_sylps is None else np.asarray(gt_sylps).astype(dtype).reshape(pred_sylps.shape)
    with to.precision(dtype):
        return to.memory_assemble(sd, hp, encoder_outputs.astype(dtype), syl_in.astype(dtype), np.asarray(speakers),
                                  np.asarray(torchmoji).astype(dtype))


def text_side(sd, hp, text, lengths, speakers, torchmoji, gt_sylps, dtype):
    """Text -> the decoder's memory, every intermediate in ``dtype``.
    Returns dict(encoder_outputs [B, T, enc], hn [B, enc], pred_sylps [B, 1], memory_in [B, T, enc + spk + 1 + tm])."""
    out, hn, sylps = encoder_side(sd, hp, text, lengths, speakers, dtype)
    memory_in = assemble(sd, hp, out, sylps, speakers, torchmoji, gt_sylps, dtype)
    assert memory_in.dtype == dtype
    return dict(encoder_outputs=out, hn=hn, pred_sylps=sylps, memory_in=memory_in)
