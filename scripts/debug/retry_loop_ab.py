"""The T2S retry loop's body and tail, device calls against the reference's host loop, on ONE recorded Tacotron pass.

One `Tacotron2.inference` at 256 rows (4 texts x 64 candidates, 200 symbols, 400 forced steps) is recorded; then, alternating
in one process (warm-up first, `--reps` repetitions each, wall clock around a device synchronise):

  loop  device:  BestOfN.update           (lengths, metrics, ctts_retry_update_f32, one 32-byte read)
        host:    text2speech.py:563-625 as written there - the batch split into items, six .item() and three
                 isnan().any() per candidate, numpy minima per candidate
  tail  device:  BestOfN.vocoder_batch + pcm16_concat + the PCM copied to the host
        host:    :645-651 (pad_sequence of the winners) + :665's .cpu().split + :675-695 per utterance, no file I/O, the
                 clips concatenated in numpy where the server calls sox

Both arms take :564-568 (`get_first_over_thresh`, `alignment_metric`) from this package, so the difference is the loop
behind them.  The vocoder is in neither arm: the tail converts one random [4, 1, max_length * hop] batch.

usage: python scripts/debug/retry_loop_ab.py [--reps 5] [--steps 400] [--per-text 64] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from cookietts_amd import BestOfN, Tacotron2, alignment_metric, get_first_over_thresh, pcm16_concat, synthetic  # noqa: E402

HOP, SAMPLING_RATE, CAT_SILENCE_S = 256, 22050, 0.1
WEIGHTS = dict(diagonality_weighting=0.5, max_focus_weighting=1.0, min_focus_weighting=0.5, avg_focus_weighting=1.0)


def host_loop(outputs, text_lengths, simultaneous_texts, batch_size_per_text, gate_threshold, max_attempts, target_score,
              absolute_maximum_tries=2048, absolutely_required_score=-1e3):
    """text2speech.py:548-551 and one trip through :555-625."""
    diagonality_weighting, max_focus_weighting = WEIGHTS["diagonality_weighting"], WEIGHTS["max_focus_weighting"]
    min_focus_weighting, avg_focus_weighting = WEIGHTS["min_focus_weighting"], WEIGHTS["avg_focus_weighting"]
    best_score = np.ones(simultaneous_texts) * -1e5
    tries = np.zeros(simultaneous_texts)
    best_generations = [0] * simultaneous_texts
    mel_batch_outputs_postnet = outputs['pred_mel_postnet']
    gate_batch_outputs = outputs['pred_gate']
    alignments_batch = outputs['alignments']
    output_lengths = get_first_over_thresh(gate_batch_outputs, gate_threshold)
    atd = alignment_metric(alignments_batch, input_lengths=text_lengths.repeat_interleave(batch_size_per_text, dim=0),
                           output_lengths=output_lengths)
    batch = list(zip(
        output_lengths.split(1, dim=0),
        mel_batch_outputs_postnet.split(1, dim=0),
        gate_batch_outputs.split(1, dim=0),
        alignments_batch.split(1, dim=0),
        atd['diagonalitys'], atd['avg_prob'], atd['encoder_max_focus'], atd['encoder_min_focus'], atd['encoder_avg_focus'],
        atd['p_missing_enc'],))
    try:
        for j in range(simultaneous_texts):
            start, end = (j * batch_size_per_text), ((j + 1) * batch_size_per_text)
            sametext_batch = batch[start:end]
            for k, (output_length, mel_outputs_postnet, gate_outputs, alignments, diagonality, avg_prob, enc_max_focus,
                    enc_min_focus, enc_avg_focus, p_missing_enc) in enumerate(sametext_batch):
                weighted_score = avg_prob.item()
                diagonality_punishment = (max(diagonality.item(), 1.10) - 1.10) * 0.5 * diagonality_weighting
                max_dur_punishment = max((enc_max_focus.item() - 60), 0) * 0.005 * max_focus_weighting
                min_dur_punishment = max(0.00 - enc_min_focus.item(), 0) * min_focus_weighting
                avg_dur_punishment = max(3.6 - enc_avg_focus.item(), 0) * avg_focus_weighting
                mis_dur_punishment = max(p_missing_enc.item() - 0.08, 0) if text_lengths[j] > 12 else 0.0
                weighted_score -= (diagonality_punishment + max_dur_punishment + min_dur_punishment + avg_dur_punishment
                                   + mis_dur_punishment)
                if torch.isnan(mel_outputs_postnet).any() or torch.isnan(gate_outputs).any() or torch.isnan(alignments).any() \
                        or weighted_score == float('nan'):
                    weighted_score = 1e-7
                if weighted_score > best_score[j]:
                    best_score[j] = weighted_score
                    best_generations[j] = [mel_outputs_postnet, output_length, alignments]
                tries[j] += 1
                if np.amin(tries) >= max_attempts and np.amin(best_score) > (absolutely_required_score - 1):
                    raise StopIteration
                if np.amin(tries) >= absolute_maximum_tries:
                    raise StopIteration
    except StopIteration:
        pass
    return best_score, tries, best_generations


def host_tail(best_generations, audio_batch_device, cat_silence_samples):
    """:645-651, the .cpu().split of :665, :675-695 without the files."""
    mel_batch_outputs_postnet = [x[0][0].T for x in best_generations]
    output_lengths = torch.stack([x[1][0] for x in best_generations], dim=0)
    max_length = output_lengths.max()
    mel_batch_outputs_postnet = torch.nn.utils.rnn.pad_sequence(mel_batch_outputs_postnet, batch_first=True,
                                                                padding_value=-11.52).transpose(1, 2)[:, :, :max_length]
    audio_batch = audio_batch_device.squeeze(1).cpu().split(1, dim=0)
    clips = []
    for j, audio in enumerate(audio_batch):
        audio_end = output_lengths[j] * HOP
        audio = audio[:, :audio_end]
        if cat_silence_samples:
            audio = torch.nn.functional.pad(audio, (0, cat_silence_samples))
        clips.append((audio.float() * 2**15).squeeze().numpy().astype('int16'))
    return mel_batch_outputs_postnet, np.concatenate(clips)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--texts", type=int, default=4)
    ap.add_argument("--per-text", type=int, default=64)
    ap.add_argument("--symbols", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, P, rows = a.texts, a.per_text, a.texts * a.per_text
    hp = synthetic.tacotron_hparams()
    m = Tacotron2(hp)
    m.load_state_dict(synthetic.to_torch(synthetic.tacotron_state_dict(hp, seed=1234)))
    m = m.cuda().eval()
    rng = np.random.default_rng(rows)
    text = torch.from_numpy(rng.integers(1, hp.n_symbols, size=(N, a.symbols))).cuda()
    tl = torch.from_numpy(np.linspace(a.symbols, a.symbols * 0.6, N).astype(np.int64)).cuda()
    rep = lambda x: x.repeat_interleave(P, dim=0)
    spk = (torch.arange(N) % 64).cuda()
    tm = torch.from_numpy(rng.standard_normal((N, hp.torchMoji_attDim)).astype(np.float32)).cuda()
    outputs = m.inference(rep(text), rep(tl), rep(spk), rep(tm), fixed_steps=a.steps)           # the recorded pass
    outputs = {k: outputs[k] for k in ("pred_mel_postnet", "pred_gate", "alignments")}
    silence = int(CAT_SILENCE_S * SAMPLING_RATE)
    kw = dict(max_attempts=10 ** 6, target_score=1e3)                                          # one whole pass, no verdict
    # a first gate over the threshold at step 0 means output_length 0 and NaN metrics (the reference divides by it too): on
    # weights whose gate does that, cut at the last step instead (no gate reaches 2.0) so that every text has a winner
    thr = 0.7 if int(get_first_over_thresh(outputs["pred_gate"], 0.7).min()) > 0 else 2.0
    best = BestOfN(N, P, hp.n_mel_channels, a.steps, **kw)

    def device_loop():
        best.reset()
        return best.update(outputs, tl, gate_threshold=thr)

    def run_host_loop():
        return host_loop(outputs, tl, N, P, thr, **kw)

    st = device_loop()
    host_best, host_tries, host_gen = run_host_loop()
    same = bool((best.best_scores().cpu().numpy() == host_best).all()) and st.min_tries == int(host_tries.min())
    audio = torch.rand(N, 1, max(st.max_best_length, 1) * HOP, device="cuda") * 2 - 1

    def device_tail():
        mel, lengths = best.vocoder_batch()
        pcm, offsets = pcm16_concat(audio, lengths, HOP, silence)
        return mel, pcm.cpu().numpy()

    def run_host_tail():
        return host_tail(host_gen, audio, silence)

    d_mel, d_pcm = device_tail()
    h_mel, h_pcm = run_host_tail()
    same_tail = bool(torch.equal(d_mel, h_mel)) and bool((d_pcm == h_pcm).all())
    arms = {"loop_device": device_loop, "loop_host": run_host_loop, "tail_device": device_tail, "tail_host": run_host_tail}
    times = {k: [] for k in arms}
    for _ in range(a.reps):                                                                      # arms alternated
        for k, fn in arms.items():
            times[k].append(wall(fn)[0])
    lines = []
    for part in ("loop", "tail"):
        d, h = np.array(times[part + "_device"]), np.array(times[part + "_host"])
        spread = max(d.max() - d.min(), h.max() - h.min())
        diff = float(np.median(h) - np.median(d))
        lines.append(dict(row="retry_" + part + "_ab", texts=N, per_text=P, rows=rows, symbols=a.symbols, steps=a.steps,
                          reps=a.reps, gate_threshold=thr, device_ms=[round(x, 3) for x in d], host_ms=[round(x, 3) for x in h],
                          device_median_ms=round(float(np.median(d)), 3), host_median_ms=round(float(np.median(h)), 3),
                          larger_spread_ms=round(float(spread), 3), difference_ms=round(diff, 3),
                          difference_exceeds_10x_spread=bool(abs(diff) > 10 * spread),
                          same_result=same if part == "loop" else same_tail, timing="wall clock around a device synchronise"))
    for line in lines:
        print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
