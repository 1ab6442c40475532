"""Tacotron2Loss: this package's device path against the same arithmetic as plain PyTorch ops on the same GPU.

Shapes: the GTA batch (192 rows x 80 mel channels x 800 frames x 200 symbols) and a validation batch (32 rows), ragged lengths,
peaked monotonic attention maps.  Arms, alternated in one process (dropped warm-up rounds first, `--reps` repetitions each,
device events on the current stream, medians and spreads):

  a  device:     cookietts_amd.Tacotron2Loss(hp)(pred, gt, {}) - eight launches and ONE device-to-host copy (the per-item table)
  b  torch GPU:  `plain_loss` below: the arithmetic of tacotron2_tm/loss_function.py:167-290 written as plain PyTorch ops in the
                 shape a trainer would write it - a guided-attention mask built per item, masked selects of the mels, the
                 alignment metric twice as a dozen small ops, and one `.item()` per number that goes into `file_losses`

The reference tree is not imported and `plain_loss` is not its text; it does not write to its inputs (the second metric call
reads a cut copy).  Every line also records what leaves the device per call in either arm, COUNTED in one extra call of each
arm under `count_d2h` (every `.cpu()`, `.item()` and `.tolist()` of a device tensor: copies and bytes).  Arm b is the per-item,
one-read-per-number shape of the reference, not a vectorised rewrite: the ratio is against that shape of code.

usage: python scripts/debug/taco_loss_ab.py [--reps 5] [--warmup 2] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from cookietts_amd import Tacotron2Loss  # noqa: E402
from cookietts_amd.taco_loss import DEFAULTS, TERMS  # noqa: E402


def make_batch(B, n_mel, T, enc, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, device=dev)
    n = lambda *s: torch.randn(*s, generator=g, device=dev)
    ml = (T // 3 + (r(B) * (T - T // 3)).long()).clamp(1, T)
    tl = (enc // 3 + (r(B) * (enc - enc // 3)).long()).clamp(1, enc)
    ml[0], tl[0] = T, enc
    gt_mel = n(B, n_mel, T) * 2 - 5
    pos = torch.linspace(0, 1, T, device=dev)[None, :, None] * ((tl - 1) * (T / ml) * (0.7 + 0.3 * r(B)))[:, None, None]
    pos = torch.minimum(pos, (tl - 1)[:, None, None].float())
    logits = -0.5 * ((torch.arange(enc, device=dev)[None, None, :] - pos) / (0.6 + 0.9 * r(B, 1, 1))) ** 2 + 0.3 * n(B, T, enc)
    t_idx = torch.arange(T, device=dev)[None, :]
    cross = (ml - 1 + (r(B) * 9).long() - 4).clamp(0, T - 1)
    gate = torch.where(t_idx >= cross[:, None], 1.5 + 2.5 * r(B, T), -4 + 3.5 * r(B, T))
    pred = {"pred_mel": gt_mel + 0.4 * n(B, n_mel, T), "pred_mel_postnet": gt_mel + 0.25 * n(B, n_mel, T), "pred_gate_logits": gate,
            "pred_sylps": (2 + 6 * r(B)).unsqueeze(1), "pred_sylps_mu": 0.5 * n(B), "pred_sylps_logvar": 0.5 * n(B) - 1,
            "alignments": torch.softmax(logits, dim=2)}
    gt = {"gt_mel": gt_mel, "mel_lengths": ml.int(), "text_lengths": tl.int(), "gt_gate_logits": (t_idx >= (ml - 1)[:, None]).float(),
          "gt_sylps": 2 + 6 * r(B), "pres_prev_state": torch.zeros(B, device=dev), "audiopath": [f"clip_{i}.wav" for i in range(B)],
          "speaker_id_ext": list(range(B))}
    return pred, gt


def plain_metric(al, in_len, out_len, thresh=0.7):
    """The alignment metric on [B, dec, enc] as small PyTorch ops; returns six [B] tensors.  `al` is not modified."""
    B, dec, enc = al.shape
    omask = torch.arange(dec, device=al.device)[None, :] < out_len[:, None]
    imask = torch.arange(enc, device=al.device)[None, :] < in_len[:, None]
    values, idx = al.max(dim=2)
    idx = idx.float()
    prev = torch.cat((idx[:, :1], idx[:, :-1]), dim=1)
    dist = (((prev - idx) ** 2 + 1).sqrt() * omask).sum(dim=1)
    diag = (dist + 1.4142135).double() / (in_len.double() ** 2 + out_len.double() ** 2).sqrt()
    tot = (al * omask[:, :, None]).sum(dim=1)
    zeroed = tot * imask
    avg_focus = zeroed.mean(dim=1) * (enc / in_len.float())
    min_focus = torch.where(imask, tot, torch.ones_like(tot)).min(dim=1)[0]
    avg_prob = (values * omask).mean(dim=1) * (dec / out_len.float())
    missing = (torch.where(imask, tot, torch.full_like(tot, 1e3)) < thresh).sum(dim=1) / in_len.float()
    return diag, avg_prob, zeroed.max(dim=1)[0], min_focus, avg_focus, missing


class count_d2h:
    """Counts the device-to-host reads made through `Tensor.cpu`, `Tensor.item` and `Tensor.tolist` while it is entered."""

    def __enter__(self):
        self.copies, self.bytes, self._saved = 0, 0, {}
        for name in ("cpu", "item", "tolist"):
            self._saved[name] = orig = getattr(torch.Tensor, name)

            def counted(t, *args, _orig=orig, **kw):
                if t.is_cuda:
                    self.copies += 1
                    self.bytes += t.numel() * t.element_size()
                return _orig(t, *args, **kw)
            setattr(torch.Tensor, name, counted)
        return self

    def __exit__(self, *exc):
        for name, orig in self._saved.items():
            setattr(torch.Tensor, name, orig)
        return False


@torch.no_grad()
def plain_loss(pred, gt, hp):
    """-> (loss_dict, file_losses)."""
    item = lambda x: x.item()
    gt_mel, ml, tl = gt["gt_mel"], gt["mel_lengths"].long(), gt["text_lengths"].long()
    B, n_mel, T = gt_mel.shape
    ld, fl = {}, {p: {"speaker_id_ext": s, "time": time.time()} for p, s in zip(gt["audiopath"], gt["speaker_id_ext"])}
    fmask = torch.arange(T, device=gt_mel.device)[None, :] < ml[:, None]
    m3 = fmask[:, None, :].expand_as(gt_mel)
    g = gt_mel.masked_select(m3)
    se = (pred["pred_mel"].masked_select(m3) - g) ** 2
    ld["spec_MSE"] = se.mean()
    for p, part in zip(gt["audiopath"], se.split([int(n) * n_mel for n in ml.cpu()])):
        fl[p]["spec_MSE"] = item(part.mean())
    ld["postnet_MSE"] = F.mse_loss(pred["pred_mel_postnet"].masked_select(m3), g)
    for key, x in (("spec_MFSE", pred["pred_mel"]), ("postnet_MFSE", pred["pred_mel_postnet"])):
        ae = (x - gt_mel).abs().transpose(1, 2)[fmask]
        ld[key] = (ae * ae.mean(dim=1, keepdim=True)).mean()
    ld["gate_loss"] = F.binary_cross_entropy_with_logits(pred["pred_gate_logits"].reshape(-1, 1), gt["gt_gate_logits"].reshape(-1, 1),
                                                         pos_weight=torch.tensor(float(hp.gate_positive_weight), device=gt_mel.device))
    mu, lv = pred["pred_sylps_mu"], pred["pred_sylps_logvar"]
    ld["sylps_kld"] = -0.5 * (1 + lv - lv.exp() - mu ** 2).sum() / B
    ld["sylps_MAE"] = F.l1_loss(pred["pred_sylps"].squeeze(1), gt["gt_sylps"])
    ld["sylps_MSE"] = F.mse_loss(pred["pred_sylps"].squeeze(1), gt["gt_sylps"])
    # guided attention: one mask per item, built on the host side of the loop
    keep = gt["pres_prev_state"] == 0
    al = pred["alignments"]
    ml_h, tl_h, keep_h = ml.tolist(), tl.tolist(), keep.tolist()
    weights = torch.zeros_like(al)
    for b in range(B):
        if keep_h[b]:
            gx = torch.arange(ml_h[b], device=al.device).float()[:, None] / ml_h[b]
            gy = torch.arange(tl_h[b], device=al.device).float()[None, :] / tl_h[b]
            weights[b, :ml_h[b], :tl_h[b]] = 1.0 - torch.exp(-(gy - gx) ** 2 / (2 * hp.DiagonalGuidedAttention_sigma ** 2))
    ld["diag_att"] = (weights * al).sum() / ml[keep].sum()
    loss = None
    for k in TERMS[:9]:
        loss = ld[k] * getattr(hp, f"{k}_weight") if loss is None else loss + ld[k] * getattr(hp, f"{k}_weight")
    ld["loss"] = loss
    m1 = plain_metric(al, tl, ml)
    ld["diagonality"], ld["avg_max_attention"] = m1[0].mean(), m1[1].mean()
    for b, p in enumerate(gt["audiopath"]):
        for k, j in (("avg_max_attention", 1), ("att_diagonality", 0), ("p_missing_enc", 5), ("char_max_dur", 2),
                     ("char_min_dur", 3), ("char_avg_dur", 4)):
            fl[p][k] = item(m1[j][b])
    sig = pred["pred_gate_logits"].sigmoid()
    sig[:, :5] = 0
    sig[:, -1] = 0.7
    plen = (sig >= 0.7).int().argmax(dim=1)
    cut = al * fmask[:, :, None]
    m2 = [x.cpu() for x in plain_metric(cut, tl, plen)]
    mx = max(ml_h)
    scores = []
    for b in range(B):
        diag, avg_prob, emax, emin, eavg, miss = (float(x[b]) for x in m2)
        s = avg_prob - (max(diag - 1.10, 0) * 0.25 + max(emax - 60.0, 0) * 0.005 + max(0.00 - emin, 0) * 0.5 + max(3.60 - eavg, 0)
                        + (max(miss - 0.08, 0) if tl_h[b] > 12 and ml_h[b] < mx * 0.75 else 0.0))
        scores.append(s)
    fl[gt["audiopath"][-1]]["att_score"] = scores[-1]
    scores = torch.tensor(scores)
    scores[torch.isnan(scores)] = scores[~torch.isnan(scores)].mean()
    ld["weighted_score"] = scores.to(al.device).mean()
    return ld, fl


def timed(fn):
    """(device-event ms, wall ms around a synchronise, result)."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    hp = SimpleNamespace(**DEFAULTS)
    crit = Tacotron2Loss(hp)
    lines = []
    for name, B in (("gta", 192), ("validation", 32)):
        n_mel, T, enc = 80, 800, 200
        pred, gt = make_batch(B, n_mel, T, enc, 27 + B, dev)
        arms = {"a_device": lambda: crit(pred, gt, {}), "b_torch_gpu": lambda: plain_loss(pred, gt, hp)}
        for _ in range(a.warmup):                                                           # dropped
            res = {k: fn() for k, fn in arms.items()}
        torch.cuda.synchronize()
        rel = {k: abs(float(res["a_device"][0][k]) - float(res["b_torch_gpu"][0][k])) / max(abs(float(res["b_torch_gpu"][0][k])), 1e-30)
               for k in TERMS}
        d2h = {}
        for k, fn in arms.items():                                                          # counted, not timed
            with count_d2h() as c:
                fn()
            d2h[k] = {"copies": c.copies, "bytes": c.bytes}
        torch.cuda.synchronize()
        ev, wall = {k: [] for k in arms}, {k: [] for k in arms}
        for _ in range(a.reps):                                                             # arms alternated
            for k, fn in arms.items():
                e, w, _ = timed(fn)
                ev[k].append(e)
                wall[k].append(w)
        med = {k: float(np.median(v)) for k, v in ev.items()}
        spread = {k: float(max(v) - min(v)) for k, v in ev.items()}
        d = med["b_torch_gpu"] - med["a_device"]
        line = dict(row="taco_loss_ab", shape=name, batch=B, n_mel=n_mel, T=T, enc=enc, reps=a.reps, warmup=a.warmup,
                    a_device_event_ms=[round(x, 3) for x in ev["a_device"]], a_device_wall_ms=[round(x, 3) for x in wall["a_device"]],
                    b_torch_gpu_event_ms=[round(x, 3) for x in ev["b_torch_gpu"]],
                    b_torch_gpu_wall_ms=[round(x, 3) for x in wall["b_torch_gpu"]],
                    median_ms={k: round(v, 3) for k, v in med.items()}, spread_ms={k: round(v, 3) for k, v in spread.items()},
                    b_minus_a_ms=round(d, 3), difference_exceeds_10x_spread=bool(abs(d) > 10 * max(spread.values())),
                    b_over_a=round(med["b_torch_gpu"] / med["a_device"], 2),
                    d2h_counted_per_call=d2h, baseline_shape="per-item loop, one .item() per file_losses number (not vectorised)",
                    max_rel_diff_loss_dict=max(rel.values()), worst_key=max(rel, key=rel.get))
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
