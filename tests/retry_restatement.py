"""Plain Python / numpy restatement of the T2S server's retry loop and PCM tail, written from the cited lines of
``_5_infer/t2s_server/text2speech.py`` (:548-651 and :675-695).  It is the pin of tests/test_retry*.py: the reference
server itself cannot run in the test environment (Flask, torchMoji and its checkpoints are absent), so there is no
reference-produced golden for this loop; the reader checks this file against the reference by reading.

The score is Python floats and Python's ``max``; the arrays are numpy.  One :class:`RetryLoop` carries the loop's state
(``best_score``, ``tries``, ``best_generations``) across passes, as the ``while`` of :552 does.
"""
import collections

import numpy as np

Status = collections.namedtuple("Status", "done n_passes min_best_score min_tries n_without_winner max_best_length max_best_T")


def score_candidate(metrics_row, text_length, flagged, diagonality_weighting=0.5, max_focus_weighting=1.0,
                    min_focus_weighting=0.5, avg_focus_weighting=1.0):
    """:598-605 and :614-615 for one candidate.  ``metrics_row``: the six values of ``alignment_metric`` in the order
    diagonalitys (float64), avg_prob, encoder_max_focus, encoder_min_focus, encoder_avg_focus, p_missing_enc (float32 tensors in
    the reference: ``.item()`` yields the float32 value widened).  Returns (score, detail): detail = [weighted_score as
    score_str prints it, the five punishments]."""
    diagonality = float(metrics_row[0])
    avg_prob, enc_max_focus, enc_min_focus, enc_avg_focus, p_missing_enc = (float(np.float32(x)) for x in metrics_row[1:6])
    weighted_score = avg_prob                                                                           # :598
    diagonality_punishment = (max(diagonality, 1.10) - 1.10) * 0.5 * diagonality_weighting              # :599
    max_dur_punishment = max((enc_max_focus - 60), 0) * 0.005 * max_focus_weighting                     # :600
    min_dur_punishment = max(0.00 - enc_min_focus, 0) * min_focus_weighting                             # :601
    avg_dur_punishment = max(3.6 - enc_avg_focus, 0) * avg_focus_weighting                              # :602
    mis_dur_punishment = max(p_missing_enc - 0.08, 0) if text_length > 12 else 0.0                      # :603
    weighted_score -= (diagonality_punishment + max_dur_punishment + min_dur_punishment + avg_dur_punishment
                       + mis_dur_punishment)                                                            # :605
    detail = [float(weighted_score), float(diagonality_punishment), float(max_dur_punishment), float(min_dur_punishment),
              float(avg_dur_punishment), float(mis_dur_punishment)]
    if flagged or weighted_score == float('nan'):                                                       # :614 (2nd: never true)
        weighted_score = 1e-7                                                                           # :615
    return weighted_score, detail


class RetryLoop:
    def __init__(self, n_texts, per_text, *, max_attempts, target_score, absolute_maximum_tries=2048,
                 absolutely_required_score=-1e3, diagonality_weighting=0.5, max_focus_weighting=1.0, min_focus_weighting=0.5,
                 avg_focus_weighting=1.0):
        self.simultaneous_texts, self.batch_size_per_text = n_texts, per_text
        self.max_attempts, self.target_score = max_attempts, target_score
        self.absolute_maximum_tries, self.absolutely_required_score = absolute_maximum_tries, absolutely_required_score
        self.weights = dict(diagonality_weighting=diagonality_weighting, max_focus_weighting=max_focus_weighting,
                            min_focus_weighting=min_focus_weighting, avg_focus_weighting=avg_focus_weighting)
        self.best_score = np.ones(n_texts) * -1e5                                                       # :548
        self.tries = np.zeros(n_texts)                                                                  # :549
        self.best_generations = [0] * n_texts                                                           # :550
        self.best_detail = [None] * n_texts                                                             # :551 (best_score_str)
        self.best_where = [None] * n_texts                                                              # (pass, row), for the tests
        self.n_passes = 0
        self.done = 0

    def status(self):
        won = [g for g in self.best_generations if g != 0]
        return Status(self.done, self.n_passes, float(np.amin(self.best_score)), int(np.amin(self.tries)),
                      sum(1 for g in self.best_generations if g == 0),
                      max([int(g[1]) for g in won], default=0), max([g[0].shape[1] for g in won], default=0))

    def update(self, mel, gate, alignments, metrics, output_lengths, text_lengths):
        """One trip through the body of the ``while`` of :552 behind the model call: mel [rows, n_mel, T], gate [rows, T],
        alignments [rows, T, enc], metrics [rows, 6], output_lengths [rows], text_lengths [n_texts].  Returns
        (status, scores [rows], detail [rows, 6]) - the scores every row WOULD enter :616 with."""
        rows = self.simultaneous_texts * self.batch_size_per_text
        scores, detail = np.zeros(rows), np.zeros((rows, 6))
        for r in range(rows):
            flagged = bool(np.isnan(mel[r]).any() or np.isnan(gate[r]).any() or np.isnan(alignments[r]).any())   # :614
            scores[r], detail[r] = score_candidate(metrics[r], int(text_lengths[r // self.batch_size_per_text]), flagged,
                                                   **self.weights)
        if self.done:                                            # the while loop has been left: nothing runs any more
            return self.status(), scores, detail
        self.n_passes += 1                                                                              # :560
        try:
            for j in range(self.simultaneous_texts):                                                    # :590
                start, end = (j * self.batch_size_per_text), ((j + 1) * self.batch_size_per_text)       # :591
                for k, r in enumerate(range(start, end)):                                               # :596
                    weighted_score = scores[r]
                    if weighted_score > self.best_score[j]:                                             # :616
                        self.best_score[j] = weighted_score
                        self.best_detail[j] = detail[r].copy()
                        self.best_generations[j] = [mel[r].copy(), int(output_lengths[r]), alignments[r].copy()]   # :619
                        self.best_where[j] = (self.n_passes - 1, r)
                    self.tries[j] += 1                                                                  # :620
                    if np.amin(self.tries) >= self.max_attempts and np.amin(self.best_score) > (self.absolutely_required_score - 1):
                        self.done = 2
                        raise StopIteration                                                             # :621-622
                    if np.amin(self.tries) >= self.absolute_maximum_tries:
                        self.done = 3
                        raise StopIteration                                                             # :623-625
        except StopIteration:                                                                           # :631
            pass
        if not self.done and not (np.amin(self.best_score) < self.target_score):                        # :552
            self.done = 1
        return self.status(), scores, detail

    def vocoder_batch(self, padding_value=-11.52):
        """:636, :645-651 -> (mel [n_texts, n_mel, max_length], output_lengths [n_texts])."""
        assert not any([x == 0 for x in self.best_generations]), \
            'Tacotron Failed to generate one of the texts after multiple attempts.'                     # :636
        mels = [x[0].T for x in self.best_generations]                                                  # :645  [T, n_mel] each
        output_lengths = np.array([x[1] for x in self.best_generations], dtype=np.int64)                # :646
        max_length = int(output_lengths.max())                                                          # :650
        longest = max(m.shape[0] for m in mels)
        padded = np.stack([np.pad(m, ((0, longest - m.shape[0]), (0, 0)), constant_values=np.float32(padding_value))
                           for m in mels])                                                              # pad_sequence(batch_first)
        return padded.transpose(0, 2, 1)[:, :, :max_length], output_lengths                             # :651


def pcm16(audio, output_lengths, hop_length, cat_silence_samples=0):
    """:675-695 per row of audio [B, T] (float32 or float16), then the rows back to back (the sox merge): (int16 [total],
    offsets [B + 1]).  Where the reference's ``astype('int16')`` is platform-defined - a product outside the int16 range, NaN -
    this states the device's documented choice: saturation, and 0."""
    clips, offsets = [], [0]
    for j in range(audio.shape[0]):
        audio_end = int(output_lengths[j]) * hop_length                                                 # :677
        clip = audio[j:j + 1, :audio_end]                                                               # :678
        if cat_silence_samples:
            clip = np.pad(clip, ((0, 0), (0, cat_silence_samples)))                                     # :690-692
        scaled = (clip.astype(np.float32) * np.float32(2 ** 15)).squeeze(0)                             # :695
        whole = np.trunc(scaled)                                                                        # astype('int16'): toward zero
        whole = np.where(np.isnan(whole), np.float32(0), whole)
        clips.append(np.clip(whole, -32768, 32767).astype(np.int16))
        offsets.append(offsets[-1] + clips[-1].shape[0])
    return np.concatenate(clips), np.array(offsets, dtype=np.int64)
