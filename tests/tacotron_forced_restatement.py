"""CPU restatement of the teacher-forced Tacotron2 pass (model.py:769-849, 976-1028 in eval mode with p_teacher_forcing = 1),
written with the stage functions of ``oracle.tacotron_oracle`` (prenet, decoder_init, attention_step, lstm_cell, encoder,
memory_assemble, postnet).  TEST INFRASTRUCTURE ONLY.

Pinned by tests/golden/tacotron_forced_*.npz (the reference's own ``Tacotron2.forward``, make_golden_taco_forced.py): the CPU test
that compares the two pins both the goldens and this file.
"""
from __future__ import annotations

import os

import numpy as np

from conftest import GOLDEN
from oracle import tacotron_oracle as to

DICT_KEYS = ("pred_mel", "pred_mel_postnet", "pred_gate_logits", "pred_sylps", "pred_sylps_mu", "pred_sylps_logvar",
             "alignments", "hidden_att_contexts", "encoder_outputs")


def load_golden(case):
    """One case as a dict: the inputs, the reference's nine outputs, the bottlenecked memory."""
    g = dict(np.load(os.path.join(GOLDEN, f"tacotron_forced_{case}.npz")))
    g.update(np.load(os.path.join(GOLDEN, f"tacotron_forced_{case}_hidden.npz")))
    return g


def decoder_forward(sd, hp, memory_in, gt_mel, lengths, keep_masks, init_mel=None):
    """Decoder.forward: step t's prenet input is frame t - 1 of ``gt_mel`` [B, n_mel, T] (the go frame for t = 0: zeros, or
    ``init_mel`` [B, n_mel, 1]); ``keep_masks`` [T, 2, B, P], mask t for step t.
    Returns (mel [B, n_mel, T], gate logits [B, T], alignments [B, T, txt_T], hidden [B, Rd2 + Dm, T], memory [B, txt_T, Dm])."""
    FT = to.FT
    sd = {k: np.asarray(v) for k, v in sd.items()}
    memory_in = np.asarray(memory_in, dtype=FT)
    lengths = np.asarray(lengths).astype(np.int64)
    B, T, _ = memory_in.shape
    n_frames = gt_mel.shape[2]
    memory, pm = to.decoder_init(sd, memory_in)
    Ra, Rd, Rd2 = hp.attention_rnn_dim, hp.decoder_rnn_dim, hp.second_decoder_rnn_dim
    att_h = np.zeros((B, Ra), FT); att_c = np.zeros((B, Ra), FT)
    dec_h = np.zeros((B, Rd), FT); dec_c = np.zeros((B, Rd), FT)
    d2_h = np.zeros((B, Rd2), FT); d2_c = np.zeros((B, Rd2), FT)
    w = np.zeros((B, T), FT); cum = np.zeros((B, T), FT)
    ctx = np.zeros((B, memory.shape[2]), FT); pos = np.zeros((B,), FT)
    go = np.zeros((B, hp.n_mel_channels), FT) if init_mel is None else np.asarray(init_mel, FT)[:, :, 0]
    sf = to._sig(sd["decoder.exp_smoothing_factor"].reshape(-1)[0].astype(FT))
    wp, bp = sd["decoder.linear_projection.linear_layer.weight"], sd["decoder.linear_projection.linear_layer.bias"]
    wg, bg = sd["decoder.gate_layer.linear_layer.weight"], sd["decoder.gate_layer.linear_layer.bias"]
    mels, gates, aligns, hiddens = [], [], [], []
    for i in range(n_frames):
        x = go if i == 0 else np.asarray(gt_mel[:, :, i - 1], FT)
        p = to.prenet(sd, x, keep_masks[i, 0], keep_masks[i, 1])
        att_h, att_c = to.lstm_cell(np.concatenate([p, ctx, dec_h], axis=1), att_h, att_c,
                                    *to._lstm_params(sd, "decoder.attention_rnn"))
        ctx, w, new_pos = to.attention_step(sd, hp, att_h, memory, pm, w, cum, pos, lengths)
        pos = (pos * sf + new_pos * (FT(1.0) - sf)).astype(FT)
        cum = (cum + w).astype(FT)
        dec_h, dec_c = to.lstm_cell(np.concatenate([att_h, ctx], axis=1), dec_h, dec_c,
                                    *to._lstm_params(sd, "decoder.decoder_rnn"))
        d2_h, d2_c = to.lstm_cell(dec_h, d2_h, d2_c, *to._lstm_params(sd, "decoder.second_decoder_rnn"))
        dc = np.concatenate([(dec_h + d2_h).astype(FT), ctx], axis=1)
        gates.append((dc @ wg.T + bg).astype(FT)[:, 0])
        mels.append((dc @ wp.T + bp).astype(FT))
        aligns.append(w); hiddens.append(dc)
    return (np.stack(mels, axis=2), np.stack(gates, axis=1), np.stack(aligns, axis=1), np.stack(hiddens, axis=2), memory)


def sylps_params(sd, gt_sylps):
    """SylpsNet.forward (tacotron2_ssvae/nets/SylpsNet.py:33-42): (mu [B], logvar [B])."""
    FT = to.FT
    s = np.asarray(gt_sylps, FT).reshape(-1)
    cat = np.stack([s, np.log(s)], axis=1).astype(FT)
    h = cat @ sd["sylps_net.seq_layers.0.linear_layer.weight"].T + sd["sylps_net.seq_layers.0.linear_layer.bias"]
    h = np.where(h > 0, h, FT(0.05) * h).astype(FT)
    res = h @ sd["sylps_net.seq_layers.2.linear_layer.weight"].T + sd["sylps_net.seq_layers.2.linear_layer.bias"]
    params = (cat + sd["sylps_net.res_weight"].reshape(()) * res).astype(FT)
    return params[:, 0], params[:, 1]


def tacotron_forward(sd, hp, gt_mel, text, lengths, speaker_ids, gt_sylps, torchmoji_hdn, keep_masks, init_mel=None):
    """Tacotron2.forward (model.py:976-1028), eval mode: the nine-key dict plus ``memory`` (the bottlenecked tensor)."""
    sd = {k: np.asarray(v) for k, v in sd.items()}
    enc_out, sylps = to.encoder(sd, hp, np.asarray(text), lengths, np.asarray(speaker_ids))
    mu, logvar = sylps_params(sd, gt_sylps)
    # eval-mode reparameterize: the memory's column is mu - which memory_assemble computes from the value it is given
    memory_in = to.memory_assemble(sd, hp, enc_out, np.asarray(gt_sylps, np.float32).reshape(sylps.shape),
                                   np.asarray(speaker_ids), torchmoji_hdn)
    mel, gate, align, hidden, memory = decoder_forward(sd, hp, memory_in, gt_mel, lengths, keep_masks, init_mel)
    return dict(pred_mel=mel, pred_mel_postnet=to.postnet(sd, hp, mel), pred_gate_logits=gate, pred_sylps=sylps,
                pred_sylps_mu=mu, pred_sylps_logvar=logvar, alignments=align, hidden_att_contexts=hidden,
                encoder_outputs=enc_out, memory=memory)
