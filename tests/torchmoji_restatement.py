"""torchMoji feature encoder (utils/torchmoji/model_def.py:169-253, feature_output=True) restated in numpy.

TEST INFRASTRUCTURE ONLY (numpy, generic in ``dtype``; see oracle/waveglow_oracle.py header for the import rule).  Built on
``lstm_seq_restatement.packed_lstm`` with the gate function as a parameter: that module reads its gate through the module-level
name ``_sigmoid``, which ``_gate`` swaps for the duration of a call (the file itself is not edited).

It follows the reference point by point:
  lengths     index of the last non-zero token plus one (model_def.py:193); zeros inside a sentence are tokens
  trimming    the batch is cut to max(len) columns (:195)
  embedding   tanh(embed.weight[tok]) (:209-210), row 0 a normal row
  LSTMs       packed bidirectional, zero initial states, gate order i, f, g, o, i / f / o through
              hard_sigmoid(v) = clamp(0.2 v + 0.5, 0, 1) (lstm.py:330-357), lstm_1 fed with lstm_0's [fwd | bwd]
  features    [lstm_1 | lstm_0 | tanh-embedding], zero beyond len[b] (:224-229)
  pooling     attlayer.py:48-66 with M = the maximum logit of the WHOLE padded batch (padded positions have logit 0)
Outputs are in INPUT order (the reference un-sorts its features; its attention weights stay sorted by length - the golden
generator un-sorts them).

Deliberately WRONG variants, for the test that proves the parity tests can fail (never used as a reference):
  "sigmoid"    logistic gates
  "order"      features as [lstm_0 | lstm_1 | embed]
  "len_count"  length = number of non-zero tokens
"""
from __future__ import annotations

import contextlib

import numpy as np

import lstm_seq_restatement as tsr

MUTATIONS = ("sigmoid", "order", "len_count")


def hard_sigmoid(x, dtype):
    return np.clip(dtype(0.2) * x + dtype(0.5), dtype(0.0), dtype(1.0)).astype(dtype)


@contextlib.contextmanager
def _gate(fn):
    """``lstm_seq_restatement.packed_lstm`` with ``fn(x, dtype)`` as the gate of i, f and o."""
    old = tsr._sigmoid
    tsr._sigmoid = fn
    try:
        yield
    finally:
        tsr._sigmoid = old


def packed_lstm(x, lengths, w_ih, w_hh, b_ih, b_hh, reverse, dtype, gate=hard_sigmoid):
    with _gate(gate):
        return tsr.packed_lstm(x, lengths, w_ih, w_hh, b_ih, b_hh, reverse, dtype)


def bilstm(x, lengths, fwd, bwd, dtype, gate=hard_sigmoid):
    with _gate(gate):
        return tsr.bilstm(x, lengths, fwd, bwd, dtype)


def lengths_of(tokens, *, mutation=None):
    tokens = np.asarray(tokens)
    nz = tokens != 0
    if mutation == "len_count":
        return nz.sum(axis=1).astype(np.int64)
    T = tokens.shape[1]
    return np.where(nz.any(axis=1), T - np.argmax(nz[:, ::-1], axis=1), 0).astype(np.int64)


def _lstm_params(sd, layer):
    return [tuple(sd[f"lstm_{layer}.{n}_l0{sfx}"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for sfx in ("", "_reverse")]


def attention_pool(feat, vector, lengths, dtype, *, batch_max=True):
    """attlayer.py:48-66.  ``batch_max``: M over the whole padded batch (the reference); else each row's own maximum over its
    valid steps.  Returns (out [B, D], att [B, T])."""
    feat, vector = np.asarray(feat).astype(dtype), np.asarray(vector).astype(dtype)
    lengths = np.asarray(lengths)
    T = feat.shape[1]
    logits = (feat @ vector).astype(dtype)
    mask = np.arange(T)[None, :] < lengths[:, None]
    if batch_max:
        m = logits.max()
    else:
        m = np.where(mask, logits, -np.inf).max(axis=1, keepdims=True)
    w = (np.exp((logits - m).astype(dtype)) * mask.astype(dtype)).astype(dtype)
    att = (w / w.sum(axis=1, keepdims=True)).astype(dtype)
    out = (feat * att[:, :, None]).sum(axis=1).astype(dtype)
    return out, att


def lstm0_preactivations(sd, tokens, dtype=np.float64):
    """The i / f / o pre-activations of lstm_0's forward direction at every valid step, one flat array (what the saturation
    test counts: the share below -2.5 and above +2.5, the two clamps of the hard sigmoid)."""
    sd = tsr.cast_state_dict(sd, dtype)
    tokens = np.asarray(tokens).astype(np.int64)
    lengths = lengths_of(tokens)
    x = np.tanh(sd["embed.weight"][tokens]).astype(dtype)
    w_ih, w_hh, b_ih, b_hh = _lstm_params(sd, 0)[0]
    out, _ = packed_lstm(x, lengths, w_ih, w_hh, b_ih, b_hh, False, dtype)
    H = w_hh.shape[1]
    h_prev = np.concatenate([np.zeros_like(out[:, :1]), out[:, :-1]], axis=1)
    pre = x @ w_ih.T + b_ih + b_hh + h_prev @ w_hh.T
    valid = np.arange(tokens.shape[1])[None, :] < lengths[:, None]
    return np.concatenate([pre[valid][:, :2 * H].ravel(), pre[valid][:, 3 * H:].ravel()])


def features(sd, tokens, dtype, *, mutation=None):
    """tokens [B, T] (any integer dtype) -> dict(features [B, 4H + E], attention [B, max(len)], lengths [B], feat [B, max(len), 4H + E]),
    input order, every intermediate in ``dtype``."""
    assert mutation is None or mutation in MUTATIONS, mutation
    sd = tsr.cast_state_dict(sd, dtype)
    tokens = np.asarray(tokens).astype(np.int64)
    lengths = lengths_of(tokens, mutation=mutation)
    assert lengths.min() >= 1, "an all-zero row: the reference fails there with an empty max"
    tokens = tokens[:, :lengths.max()]
    T = tokens.shape[1]
    gate = tsr._sigmoid if mutation == "sigmoid" else hard_sigmoid
    x = np.tanh(sd["embed.weight"][tokens]).astype(dtype)
    valid = (np.arange(T)[None, :] < lengths[:, None])[:, :, None]
    x = np.where(valid, x, dtype(0.0)).astype(dtype)
    p0, p1 = _lstm_params(sd, 0), _lstm_params(sd, 1)
    o0, _ = bilstm(x, lengths, p0[0], p0[1], dtype, gate)
    o1, _ = bilstm(o0, lengths, p1[0], p1[1], dtype, gate)
    parts = [o0, o1, x] if mutation == "order" else [o1, o0, x]
    feat = np.concatenate(parts, axis=2).astype(dtype)
    out, att = attention_pool(feat, sd["attention_layer.attention_vector"], lengths, dtype)
    assert out.dtype == dtype and att.dtype == dtype
    return dict(features=out, attention=att, lengths=lengths, feat=feat)
