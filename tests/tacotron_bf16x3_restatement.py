"""Restatement of the Tacotron2 decoder's SPLIT-BF16 cell arithmetic (helper of test_tacotron_bf16x3.py; TEST INFRASTRUCTURE ONLY -
the product path is ``cookietts_amd.tacotron2`` with ``set_f32_gemm_mode("bf16x3")`` over csrc/tacotron_batched_bf16x3.h).

Written from the contract at ``ctts_taco_decoder_steps_bf16x3``, not from the kernel: it is ``oracle.tacotron_oracle.
decoder_inference_steps`` with the products of the three ``lstm_cell`` calls replaced by split products summed in float64 and
rounded to fp32; every other stage is the oracle's fp32 arithmetic.

    split(v) = (hi, lo),  hi = bf16_rne(v),  lo = bf16_rne(v - hi)                  (v fp32; hi, lo held as float64 values)
    X = [x | h], W = [w_ih | w_hh]                                                   (the cell's GEMM over the whole K)
    sum = fp32(X_hi W_hi^T + X_hi W_lo^T + X_lo W_hi^T)                              (float64 sums; no lo * lo term)
    gates = sum + (b_ih + b_hh) in fp32, then the oracle's cell update

``terms`` names the products that are summed - ``"hh"`` = W_hi x_hi, ``"lh"`` = W_lo x_hi, ``"hl"`` = W_hi x_lo - so that a test
can plant the faults it must tell apart (a dropped cross term, hi * hi only).
"""
import numpy as np
import torch

from oracle import tacotron_oracle as to

TERMS = ("hh", "lh", "hl")


def split(v):
    """fp32 array -> (hi, lo) as float64 arrays holding bf16 values."""
    v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    hi = v.to(torch.bfloat16).to(torch.float32)
    lo = (v - hi).to(torch.bfloat16).to(torch.float32)
    return hi.double().numpy(), lo.double().numpy()


def make_lstm_cell(terms=TERMS):
    """``oracle.tacotron_oracle.lstm_cell`` with the split products; the weights of a cell are split once (keyed by the array)."""
    assert set(terms) <= set(TERMS) and terms
    cache = {}

    def lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh):
        key = (id(w_ih), id(w_hh))
        if key not in cache:
            cache[key] = (w_ih, w_hh) + split(np.concatenate([w_ih, w_hh], axis=1))      # (the arrays are kept: ids stay unique)
        wh, wl = cache[key][2:]
        xh, xl = split(np.concatenate([x, h], axis=1))
        s = 0.0
        for t, (a, b) in (("hh", (xh, wh)), ("lh", (xh, wl)), ("hl", (xl, wh))):
            if t in terms:
                s = s + a @ b.T
        g = (s.astype(np.float32) + (b_ih + b_hh).astype(np.float32)).astype(np.float32)
        H = h.shape[1]
        i, f, gg, o = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
        sig = lambda v: (np.float32(1.0) / (np.float32(1.0) + np.exp(-v))).astype(np.float32)      # noqa: E731
        c2 = (sig(f) * c + sig(i) * np.tanh(gg)).astype(np.float32)
        h2 = (sig(o) * np.tanh(c2)).astype(np.float32)
        return h2, c2
    return lstm_cell


def decoder_inference_steps(sd, hp, memory_in, lengths, keep_masks, n_steps, terms=TERMS):
    """The oracle's ``decoder_inference_steps`` (same arguments, same returns) with the three cells' products split."""
    saved = to.lstm_cell
    to.lstm_cell = make_lstm_cell(terms)
    try:
        return to.decoder_inference_steps(sd, hp, memory_in, lengths, keep_masks, n_steps)
    finally:
        to.lstm_cell = saved
