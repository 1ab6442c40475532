#!/usr/bin/env python3
"""Secondary measurements for SURVEY.md 8 rows B (WaveFlow, config 4), C (Tacotron2 decoder, config 5)
and D (STFT/mel).  bench.py stays the headline (config 2): it imports the row functions of this file and attaches
short runs of configs 3 / 4 / 5 to its JSON line as ``rows`` (after, never inside, the headline's timed region);
run as a script this prints one JSON line per row."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cookietts_amd import synthetic  # noqa: E402


def _batches(args, default):
    return tuple(int(x) for x in args.batches.split(",")) if getattr(args, "batches", "") else default


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


FP32_MFMA_PEAK_TFLOPS = 157.3
HBM_PEAK_TBPS = 8.0                # MI355X_MICROARCH.md: HBM3E spec peak (6.29 TB/s measured with a float4 copy)
F16_MFMA_PEAK_TFLOPS = 2500.0      # MI355X_MICROARCH.md: dense bf16 / f16 MFMA (v_mfma_f32_32x32x16_f16 takes the bf16 form's cycles)


def gemm_loop_label():
    """What the calling thread's last conv-GEMM launch really ran (ctts_last_gemm_loop): the fused WaveFlow layer runs
    fp32 MFMA in its split-K shape (batch <= 2) whatever mode the model asked for."""
    from cookietts_amd import _lib
    code = _lib.lib().ctts_last_gemm_loop()
    loop = {0: "fp32 MFMA", 3: "split-bf16 x3", 6: "split-bf16 x6"}.get(code & 15, f"level {code & 15}")
    if code & 64:
        shape = ("row queue (one launch per flow), " if code & 128 else "row queue (one launch per row), ") + \
            ("split-K items of 128 x 64" if code & 32 else "items of 128 x 128")
    else:
        shape = "split-K shape" if code & 32 else "small shape" if code & 16 else "large shape"
    return f"{loop}, {shape}"


def _mode(m, args):
    """The rows' GEMM main loop travels in each model's config (``--gemm-mode``; there is no process-wide default)."""
    mode = getattr(args, "gemm_mode", "f32")
    if mode != "f32" and hasattr(m, "set_f32_gemm_mode"):
        m.set_f32_gemm_mode(mode)
    return m


def row_waveflow(args):
    from cookietts_amd.waveglow_ax import WaveGlow
    cfg = synthetic.WAVEFLOW_CONFIGS["full"]
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(synthetic.waveflow_state_dict(cfg, seed=1234)))
    m = m.cuda().eval()
    _mode(m, args)
    rows = []
    for B in _batches(args, (1, 8)):     # B = 1 too: the reference's own WaveFlow timing table is batch 1
        F = 900
        mel = torch.from_numpy(synthetic.synthetic_mel(B, F)).cuda()
        dt = timed(lambda: m.infer(mel, sigma=0.6, return_CPU=False), args.warmup, args.steps)
        loop = gemm_loop_label()
        samples = B * (F - 1) * 256
        wn = cfg["WN_config"]
        C, G = wn["n_channels"], cfg["n_group"]
        mac = 0.6515e6 * (G - 1) * cfg["n_flows"] / G          # per output sample
        rows.append({"row": "B/config4", "metric": "audio samples/sec (22.05kHz) WaveFlow infer (8 flows, 64 ch, h=16), 80x900 mel",
                     "value": samples / dt, "unit": "samples/s", "rtf": samples / dt / 22050, "ms_per_call": dt * 1e3,
                     "dtype": "f32", "batch": B, "frames": F,
                     # per row of the recurrence: start + tail + (row queue: ONE launch for the n_layers fused layers | one per layer)
                     "kernel_launches_per_utterance_batch": (2 * cfg["n_flows"] if "per flow" in loop else
                                                             ((1 if "row queue" in loop else wn["n_layers"]) + 2) * cfg["n_flows"] * (G - 1)),
                     # common schema (the headline's): the fused WaveFlow layer kernels against the fp32 MFMA peak on SURVEY 8d's
                     # algorithmic MACs per output sample; the survey's 138 KB-per-sample HBM denominator stays below as extra keys
                     "roofline": {"kernel": "fused WaveFlow layer (" + loop + ")", "bound": "mfma",
                                  "achieved": 2 * mac * samples / dt / 1e12, "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                                  "frac": 2 * mac * samples / dt / 1e12 / FP32_MFMA_PEAK_TFLOPS, "traffic": None},
                     "last_gemm_loop": loop,
                     # 138 KB of per-layer-kernel traffic per output sample (2304 B per row, step, layer)
                     "achieved_GBps_vs_138KB_per_sample": 138e3 * samples / dt / 1e9,
                     "hbm_frac_vs_138KB_per_sample": 138e3 * samples / dt / 8e12})
    return rows


# "WaveFlow Inference Times.png" (CookieTTS/_4_mtw/): the reference's only published numbers for this path.
# Columns: n_group, n_flows, n_channels, separable, published 22 kHz real-time factor (batch 1, 8 layers, hardware not named).
PUBLISHED_WAVEFLOW_TABLE = [
    (8, 6, 64, 0, 17.002), (8, 6, 64, 1, 16.432), (8, 8, 64, 0, 12.448), (8, 8, 64, 1, 12.251), (8, 8, 128, 1, 9.316),
    (20, 4, 128, 1, 8.807), (20, 6, 64, 0, 6.200), (20, 6, 64, 1, 6.011), (20, 6, 128, 1, 6.003), (8, 8, 128, 0, 5.376),
    (20, 6, 256, 1, 4.956), (20, 8, 64, 0, 4.911), (20, 8, 64, 1, 4.612), (8, 8, 256, 1, 4.488), (20, 8, 128, 1, 4.450),
    (12, 8, 256, 1, 4.218), (20, 8, 128, 0, 4.070), (20, 8, 256, 1, 3.778), (20, 10, 128, 1, 3.674), (20, 12, 128, 1, 3.076),
    (20, 6, 256, 0, 1.953), (50, 8, 128, 0, 1.929), (50, 8, 256, 1, 1.747), (20, 8, 512, 1, 1.630), (20, 8, 256, 0, 1.459),
    (50, 8, 256, 0, 1.131), (20, 8, 512, 0, 0.375), (50, 8, 512, 0, 0.336)]


def row_waveflow_table(args):
    """Every architecture of the reference's published WaveFlow sweep at batch 1 (the only batch it published), ~10 s of audio:
    3x3 kernels, 8 layers, permuteheight mixing (config 4's family), hop 256 for n_group 8 and 300 otherwise
    (hop % n_group == 0, efficient_model_ax.py:23); random-init weights.  The published factor is printed beside ours for
    context only: its hardware is not named."""
    import gc
    from cookietts_amd.waveglow_ax import WaveGlow
    rows = []
    for G, n_flows, C, sep, published in PUBLISHED_WAVEFLOW_TABLE:
        hop = 256 if G == 8 else 300
        cfg = synthetic.waveflow_config(n_flows=n_flows, n_group=G, n_channels=C, hop_length=hop, win_length=4 * hop,
                                        WN=dict(seperable_conv=bool(sep)))
        m = WaveGlow(**cfg)
        m.load_state_dict(synthetic.to_torch(synthetic.waveflow_state_dict(cfg, seed=1234)))
        m = m.cuda().eval()
        _mode(m, args)
        F = 220500 // hop
        mel = torch.from_numpy(synthetic.synthetic_mel(1, F)).cuda()
        dt = timed(lambda: m.infer(mel, sigma=0.6, return_CPU=False), args.warmup, args.steps)
        samples = (F - 1) * hop
        rows.append({"row": "B/waveflow_table", "metric": "real-time factor at 22.05 kHz, WaveFlow infer, batch 1",
                     "n_group": G, "n_flows": n_flows, "n_layers": 8, "n_channels": C, "seperable_conv": sep, "hop_length": hop,
                     "frames": F, "value": samples / dt / 22050, "unit": "x real time", "ms_per_call": dt * 1e3,
                     "published_rtf_22khz": published, "vs_published": samples / dt / 22050 / published,
                     "published_source": "CookieTTS/_4_mtw/WaveFlow Inference Times.png (hardware not named)",
                     "last_gemm_loop": gemm_loop_label(), "dtype": "f32"})
        del m
        gc.collect()
        torch.cuda.empty_cache()
    return rows


def row_waveflow_author(args):
    """the option set / sizes of the author's own WaveFlow checkpoints (48 kHz, hop 600, n_group 20,
    128 channels, separable 7x7 in-layers, speaker embeddings, 5 + 3 layer conditioning stacks, de-emphasis)."""
    from cookietts_amd.waveglow_ax import WaveGlow
    cfg = synthetic.WAVEFLOW_CONFIGS["author"]
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(synthetic.waveflow_state_dict(cfg, seed=1234)))
    m = m.cuda().eval()
    _mode(m, args)
    B, F = 8, 400
    mel = torch.from_numpy(synthetic.synthetic_mel(B, F, cfg["n_mel_channels"] * 2)).cuda()
    ids = torch.arange(B).cuda()
    dt = timed(lambda: m.infer(mel, speaker_ids=ids, sigma=0.6, return_CPU=False), args.warmup, args.steps)
    samples = B * (F - 1) * cfg["hop_length"]
    return {"row": "B/8f.4", "metric": "audio samples/sec (48kHz) WaveFlow infer, author's option set (8 flows, 128 ch, "
                                       "h=20, separable 7x7, speaker + cond stacks), 320x400 mel",
            "value": samples / dt, "unit": "samples/s", "rtf": samples / dt / cfg["sampling_rate"],
            "ms_per_call": dt * 1e3, "dtype": "f32", "batch": B, "frames": F}


def row_waveglow_ax_notebook(args):
    """the ONLY WaveGlow timing recorded in the reference tree - scripts/"WaveGlowFlow Inference
    Speed Testing.ipynb" cells 2-6: ax core, waveflow=False, 48 flows, n_group 24, 8 x 256 WN, 'permute' mixing,
    speaker embeddings, 3-layer cond stack, batch 1, one 5.8375 s clip at 48 kHz (hop 600 -> 468 mel frames):
    1.27 s = 4.60x real time (eager, fp16), 1.125 s = 5.19x (jit-traced), GPU not stated.  Same model shape, same
    clip length, batch 1 here; fp32, or with ``--dtype f16`` what the reference ran: ``.half()`` = IEEE-half WN activations
    on the f16 matrix pipe (``set_compute_dtype(torch.float16)``), priced against the nominal f16 MFMA peak."""
    m, cfg = _ax_notebook_model()
    _mode(m, args)
    f16 = getattr(args, "dtype", "f32") == "f16"
    if f16:
        m.set_compute_dtype(torch.float16)
    rows = []
    for B in _batches(args, (1, 8)):
        mel, ids = _ax_notebook_input(cfg, B)
        dt = timed(lambda: m.infer(mel, speaker_ids=ids, sigma=1.0, return_CPU=False), args.warmup, args.steps)
        rows.append(_ax_notebook_row(cfg, B, dt, "f16" if f16 else "f32"))
    return rows


def _ax_notebook_model():
    from cookietts_amd.waveglow_ax import WaveGlow
    cfg = synthetic.WAVEGLOW_AX_CONFIGS["notebook"]
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(synthetic.waveglow_ax_state_dict(cfg, seed=1234)))
    return m.cuda().eval(), cfg


AX_NOTEBOOK_FRAMES = 468                                          # -> (F - 1) * 600 = 280 200 samples = 5.8375 s


def _ax_notebook_input(cfg, B):
    mel = torch.from_numpy(synthetic.synthetic_mel(B, AX_NOTEBOOK_FRAMES, cfg["n_mel_channels"])).cuda()
    return mel, torch.zeros(B, dtype=torch.int64).cuda()


def _ax_notebook_row(cfg, B, dt, dtype):
    F = AX_NOTEBOOK_FRAMES
    peak = F16_MFMA_PEAK_TFLOPS if dtype == "f16" else FP32_MFMA_PEAK_TFLOPS
    samples = B * (F - 1) * cfg["hop_length"]                 # infer() pads one frame and trims one hop
    wn = cfg["WN_config"]
    C, nl = wn["n_channels"], wn["n_layers"]
    flop = 2.0 * cfg["n_flows"] * nl * (3 * C * 2 * C + 2 * C * C) * (samples / cfg["n_group"])   # in + res/skip GEMMs
    return {"row": "W5/notebook", "metric": "real-time factor (48 kHz), ax WaveGlow waveflow=False, 48 flows x 8 x 256, "
                                                "n_group 24, 160x468 mel (5.84 s clip)",
                "value": samples / dt / 48000.0, "unit": "x real time (48 kHz)", "batch": B, "ms_per_call": dt * 1e3,
                "samples_per_s": samples / dt, "rtf_22k_equiv": samples / dt / 48000.0 * 48 / 22, "dtype": dtype,
                "reference_published": {"eager_fp16_rtf_48k": 4.5977, "jit_fp16_rtf_48k": 5.1905, "batch": 1,
                                        "hardware": "not stated", "source": "BASELINE.md section 1"},
                "vs_reference_eager": (samples / dt / 48000.0) / 4.5977 if B == 1 else None,
                "roofline": {"kernel": "ax 1-D WN in-layer + res/skip conv-GEMMs", "bound": "mfma", "achieved": flop / dt / 1e12,
                             "peak": peak, "unit": "TFLOP/s", "frac": flop / dt / 1e12 / peak, "traffic": None}}


def row_waveglow_ax_notebook_ab(args):
    """The notebook row's three arms - fp32 MFMA, split bf16 (``bf16x3``), IEEE-half storage (``f16``) - in ONE process: one
    model per arm, the arms alternated ``--reps`` times after a warm-up of each, one line per (arm, batch) with every
    repetition's time, the median and the spread.  Compare arms of the same run only."""
    arms = []
    for name in ("f32", "bf16x3", "f16"):
        m, cfg = _ax_notebook_model()
        if name == "bf16x3":
            m.set_f32_gemm_mode("bf16x3")
        if name == "f16":
            m.set_compute_dtype(torch.float16)
        arms.append((name, m))
    rows = []
    for B in _batches(args, (1, 8)):
        mel, ids = _ax_notebook_input(cfg, B)
        times = {name: [] for name, _ in arms}
        for name, m in arms:
            timed(lambda: m.infer(mel, speaker_ids=ids, sigma=1.0, return_CPU=False), args.warmup, 1)
        for _ in range(getattr(args, "reps", 5)):
            for name, m in arms:
                times[name].append(timed(lambda: m.infer(mel, speaker_ids=ids, sigma=1.0, return_CPU=False), 0, args.steps))
        for name, _ in arms:
            t = sorted(times[name])
            row = _ax_notebook_row(cfg, B, t[len(t) // 2], "f16" if name == "f16" else "f32")
            row.update({"arm": name, "reps_ms": [x * 1e3 for x in times[name]], "ms_min": t[0] * 1e3, "ms_max": t[-1] * 1e3,
                        "spread_frac": (t[-1] - t[0]) / t[len(t) // 2]})
            rows.append(row)
    return rows


def row_waveglow_ax_sep_ab(args):
    """Separable in-layers on the 1-D ax core against the same network folded into dense in-layers: the notebook config
    (48 flows x 8 x 256, n_group 24) with ``seperable_conv`` at kernel size 3 and 7 (``--ks``), batch 1 and 8 on the notebook
    row's 5.84 s clip.  Arm ``sep`` = depthwise launch + K = C GEMM (ctts_wgax_sep_inverse_f32); arm ``fold`` = the same weights
    through ``synthetic.fold_separable`` on the dense path (K = ks * C).  Same latent for both arms, the arms alternated
    ``--reps`` times in one process after a warm-up of each, timed by device events; ``--arms sep`` for a profiler pass."""
    import copy
    import gc
    from cookietts_amd.waveglow_ax import WaveGlow
    arms_on = [a for a in getattr(args, "arms", "").split(",") if a in ("sep", "fold")] or ["sep", "fold"]
    rows = []
    for ks in (int(k) for k in getattr(args, "ks", "3,7").split(",")):
        cfg = copy.deepcopy(synthetic.WAVEGLOW_AX_CONFIGS["notebook"])
        cfg["WN_config"].update(seperable_conv=True, kernel_size_w=ks)
        sd = synthetic.waveglow_ax_state_dict(cfg, seed=1234)
        models = {}
        for name in arms_on:
            c, w = (cfg, sd) if name == "sep" else synthetic.fold_separable(sd, cfg)[::-1]
            m = WaveGlow(**c)
            m.load_state_dict(synthetic.to_torch(w))
            models[name] = _mode(m.cuda().eval(), args)
        wn = cfg["WN_config"]
        C, nl, G = wn["n_channels"], wn["n_layers"], cfg["n_group"]
        for B in _batches(args, (1, 8)):
            mel, ids = _ax_notebook_input(cfg, B)
            T = AX_NOTEBOOK_FRAMES * cfg["hop_length"]
            z = torch.randn(B, T - T % G, device="cuda")
            arms = [(n, (lambda m=m: m.infer_from_noise(mel, z, speaker_ids=ids, return_CPU=False))) for n, m in models.items()]
            times, outs = {n: [] for n, _ in arms}, {}
            for n, fn in arms:
                for _ in range(max(1, args.warmup)):
                    outs[n] = fn()
                torch.cuda.synchronize()
            for _ in range(getattr(args, "reps", 5)):
                for n, fn in arms:
                    times[n].append(_event_ms(fn, args.steps))
            med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
            L = z.shape[1] // G
            row = {"row": "W5/notebook_sep_ab", "metric": f"ax WaveGlow waveflow=False, 48 flows x 8 x 256, n_group 24, seperable_conv, "
                                                          f"kernel {ks}, 160x468 mel (5.84 s clip), ms per call (device events)",
                   "kernel_size": ks, "batch": B, "unit": "ms", "dtype": "f32",
                   "arms": {n: {"reps_ms": t, "median_ms": med[n], "min_ms": min(t), "max_ms": max(t),
                                "spread_frac": (max(t) - min(t)) / med[n]} for n, t in times.items()},
                   # counted from the layer shapes, per call: in-layer + res/skip GEMMs of each arm, and the depthwise stage's traffic
                   "gemm_flop": {"sep": 2.0 * cfg["n_flows"] * nl * (2 * C * C + 2 * C * C) * B * L,
                                 "fold": 2.0 * cfg["n_flows"] * nl * (ks * 2 * C * C + 2 * C * C) * B * L},
                   "depthwise_launches": cfg["n_flows"] * nl, "depthwise_bytes_per_launch": 2 * B * C * L * 4}
            if "sep" in med:
                row.update({"value": med["sep"], "rtf_48k": B * (AX_NOTEBOOK_FRAMES - 1) * cfg["hop_length"] / (med["sep"] * 1e-3) / 48000.0})
            if len(med) == 2:
                row["fold_over_sep"] = med["fold"] / med["sep"]
                d = outs["sep"].double() - outs["fold"].double()
                row["sep_vs_fold_rel_rms"] = float(d.pow(2).mean().sqrt() / outs["fold"].double().pow(2).mean().sqrt())
            rows.append(row)
            del outs, z, mel
        del models
        gc.collect()
        torch.cuda.empty_cache()
    return rows


def _hifigan_pair(key):
    """(HIP generator, baseline closure, cfg): the same synthetic weights behind ``cookietts_amd.HiFiGANGenerator`` and behind
    the plain ``torch.nn.functional`` restatement (tests/hifigan_restatement.py, folded weights, fp32 on the same GPU)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import hifigan_restatement as hr
    from cookietts_amd import HiFiGANGenerator
    from cookietts_amd.hifigan import AttrDict
    cfg = synthetic.HIFIGAN_CONFIGS[key]
    sd = synthetic.hifigan_state_dict(cfg, seed=1234)
    m = HiFiGANGenerator(AttrDict(cfg))
    m.load_state_dict(synthetic.to_torch(sd))
    m = m.cuda().eval()
    w = hr.folded_weights(cfg, sd, torch.float32, "cuda")
    return m, (lambda mel: hr.generator(cfg, w, mel)), cfg, hr


def _hifigan_f16_pair(key):
    """(HIP generator in the IEEE-half storage mode, baseline closure): a second instance on the same weights, so that the
    alternated loop never repacks, and the restatement's plain F.conv1d generator with ``.half()`` weights through
    PyTorch-ROCm - what a user of the reference gets today from ``vocoder.half()``."""
    import hifigan_restatement as hr
    from cookietts_amd import HiFiGANGenerator
    from cookietts_amd.hifigan import AttrDict
    cfg = synthetic.HIFIGAN_CONFIGS[key]
    sd = synthetic.hifigan_state_dict(cfg, seed=1234)
    m = HiFiGANGenerator(AttrDict(cfg))
    m.load_state_dict(synthetic.to_torch(sd))
    m = m.cuda().eval().set_compute_dtype(torch.float16)
    w = {k: (a.half(), b.half()) for k, (a, b) in hr.folded_weights(cfg, sd, torch.float32, "cuda").items()}
    return m, (lambda mel16: hr.generator(cfg, w, mel16))


def _hifigan_bf16x3(key):
    """A third HIP generator on the same weights with ``set_f32_gemm_mode("bf16x3")`` (its own instance: the alternated loop
    never repacks)."""
    from cookietts_amd import HiFiGANGenerator
    from cookietts_amd.hifigan import AttrDict
    cfg = synthetic.HIFIGAN_CONFIGS[key]
    m = HiFiGANGenerator(AttrDict(cfg))
    m.load_state_dict(synthetic.to_torch(synthetic.hifigan_state_dict(cfg, seed=1234)))
    return m.cuda().eval().set_f32_gemm_mode("bf16x3")


def _event_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def row_hifigan(args):
    """HiFi-GAN generator (the vocoder text2speech.py:258-263 loads): v1 at B = 1, 4, 16 x 80 x 900 (16 = the server's
    vocoder_batch_size) and v1-48 kHz at B = 1.  Two arms alternated ``--reps`` times in one process after a warm-up of each
    shape, timed by device events: ``hip`` = ctts_hifigan_forward_f32, ``torch`` = the same generator as plain
    F.conv1d / F.conv_transpose1d calls in fp32 through PyTorch-ROCm (what a user gets today).  FLOP from the shapes
    (hifigan_restatement.generator_macs); ``--batches`` restricts the v1 batch sizes; ``--arms hip`` for a profiler pass.

    Two more arms in the same alternated loop give a second row per shape, ``H/hifigan_f16``: ``hip_f16`` =
    ctts_hifigan_forward_f16 (``set_compute_dtype(torch.float16)``: IEEE-half storage, f16 MFMA) and ``torch_f16`` = the plain
    generator with ``.half()`` weights and mel through PyTorch-ROCm.  Its ``roofline`` carries both fractions - FLOP over the
    f16 MFMA peak, algorithmic bytes (hifigan_f16_restatement.generator_bytes) over the HBM peak - and ``bound`` names the larger.

    ``hip_bf16x3`` = ctts_hifigan_forward_bf16x3 (``set_f32_gemm_mode("bf16x3")``: fp32 tensors, split-bf16 products) in the same
    loop gives a third row, ``H/hifigan_bf16x3``, priced against one third of the bf16 MFMA peak (three products per operand pair)
    and against HBM by the algorithmic fp32 bytes."""
    rows = []
    frames = 900
    arms_on = getattr(args, "arms", "hip,torch,hip_f16,torch_f16,hip_bf16x3").split(",")
    for key, batches in (("v1", _batches(args, (1, 4, 16))), ("v1_48khz", (1,))):
        m, base, cfg, hr = _hifigan_pair(key)
        m16, base16 = _hifigan_f16_pair(key) if ("hip_f16" in arms_on or "torch_f16" in arms_on) else (None, None)
        m3 = _hifigan_bf16x3(key) if "hip_bf16x3" in arms_on else None
        import hifigan_f16_restatement as h16
        rate = cfg["sampling_rate"]
        for B in batches:
            mel = torch.from_numpy(synthetic.synthetic_mel(B, frames, cfg["num_mels"], seed=B)).cuda()
            mel16 = mel.half()
            arms = [a for a in (("hip", lambda: m(mel)), ("torch", lambda: base(mel)), ("hip_f16", lambda: m16(mel)),
                                ("torch_f16", lambda: base16(mel16)), ("hip_bf16x3", lambda: m3(mel))) if a[0] in arms_on]
            times = {n: [] for n, _ in arms}
            with torch.no_grad():
                outs = {}
                for n, fn in arms:
                    for _ in range(max(1, args.warmup)):
                        outs[n] = fn()
                    torch.cuda.synchronize()
                for _ in range(getattr(args, "reps", 5)):
                    for n, fn in arms:
                        times[n].append(_event_ms(fn, args.steps))
            flop = 2.0 * hr.generator_macs(cfg, frames) * B
            samples = B * frames * m.upsample_factor
            med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
            row = {"row": "H/hifigan", "metric": f"HiFi-GAN {key} generator, fp32, {B} x {cfg['num_mels']} x {frames} mel, ms per call (device events)",
                   "config": key, "batch": B, "frames": frames, "flop": flop,
                   "arms": {n: {"reps_ms": t, "median_ms": med[n], "min_ms": min(t), "max_ms": max(t),
                                "spread_frac": (max(t) - min(t)) / med[n]} for n, t in times.items() if n in ("hip", "torch")}}
            if "hip" in med:
                dt = med["hip"] * 1e-3
                row.update({"value": med["hip"], "unit": "ms", "samples_per_sec": samples / dt, "rtf": samples / dt / rate,
                            "roofline": {"kernel": "hg_conv_kernel (all launches of the call)", "bound": "mfma", "achieved": flop / dt / 1e12,
                                         "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": flop / dt / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                                         "traffic": None}})
            if "hip" in med and "torch" in med:
                row["torch_over_hip"] = med["torch"] / med["hip"]
                d = (outs["hip"].double() - outs["torch"].double())
                row["hip_vs_torch_rel_rms"] = float(d.pow(2).mean().sqrt() / outs["torch"].double().pow(2).mean().sqrt())
            if "hip" in med or "torch" in med:
                rows.append(row)
            if "hip_f16" in med or "torch_f16" in med:
                rows.append(_hifigan_f16_row(key, cfg, B, frames, flop, samples, rate, times, med, outs, h16))
            if "hip_bf16x3" in med:
                rows.append(_hifigan_bf16x3_row(key, cfg, B, frames, flop, samples, rate, times, med, outs, h16))
            del mel, mel16, outs
        del m, base, m16, base16, m3
        torch.cuda.empty_cache()
    return rows


def _hifigan_f16_row(key, cfg, B, frames, flop, samples, rate, times, med, outs, h16):
    """The half-storage row of one shape: the f16 arms, the fp32 ``hip`` arm of the same loop as the ratio's denominator."""
    nbytes = float(B * h16.generator_bytes(cfg, frames, 2))
    row = {"row": "H/hifigan_f16", "metric": f"HiFi-GAN {key} generator, IEEE-half storage, {B} x {cfg['num_mels']} x {frames} mel, ms per call (device events)",
           "config": key, "batch": B, "frames": frames, "flop": flop, "algorithmic_bytes": nbytes,
           "arms": {n: {"reps_ms": t, "median_ms": med[n], "min_ms": min(t), "max_ms": max(t),
                        "spread_frac": (max(t) - min(t)) / med[n]} for n, t in times.items() if n in ("hip_f16", "torch_f16")}}
    if "hip_f16" in med:
        dt = med["hip_f16"] * 1e-3
        mfma_frac = flop / dt / 1e12 / F16_MFMA_PEAK_TFLOPS
        hbm_frac = nbytes / dt / 1e12 / HBM_PEAK_TBPS
        row.update({"value": med["hip_f16"], "unit": "ms", "samples_per_sec": samples / dt, "rtf": samples / dt / rate,
                    "roofline": {"kernel": "hg_conv_f16_kernel (all launches of the call)", "bound": "hbm" if hbm_frac >= mfma_frac else "mfma",
                                 "mfma": {"achieved": flop / dt / 1e12, "peak": F16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": mfma_frac},
                                 "hbm": {"achieved": nbytes / dt / 1e12, "peak": HBM_PEAK_TBPS, "unit": "TB/s", "frac": hbm_frac},
                                 "frac": max(hbm_frac, mfma_frac), "traffic": "algorithmic bytes from the shapes, not counters"}})
        if "hip" in med:
            row["hip_f32_over_hip_f16"] = med["hip"] / med["hip_f16"]
        if "torch_f16" in med:
            row["torch_f16_over_hip_f16"] = med["torch_f16"] / med["hip_f16"]
            d = (outs["hip_f16"].double() - outs["torch_f16"].double())
            row["hip_f16_vs_torch_f16_rel_rms"] = float(d.pow(2).mean().sqrt() / outs["torch_f16"].double().pow(2).mean().sqrt())
        if "hip" in outs:
            d = (outs["hip_f16"].double() - outs["hip"].double())
            row["hip_f16_vs_hip_f32_rel_rms"] = float(d.pow(2).mean().sqrt() / outs["hip"].double().pow(2).mean().sqrt())
    return row


def _hifigan_bf16x3_row(key, cfg, B, frames, flop, samples, rate, times, med, outs, h16):
    """The split-bf16 row of one shape; the fp32 ``hip`` arm of the same loop is the ratio's denominator.  ``flop`` counts one
    product per operand pair, so the matrix-pipe peak it is priced against is a third of the bf16 MFMA peak."""
    nbytes = float(B * h16.generator_bytes(cfg, frames, 4))
    peak = F16_MFMA_PEAK_TFLOPS / 3.0
    t = times["hip_bf16x3"]
    dt = med["hip_bf16x3"] * 1e-3
    mfma_frac = flop / dt / 1e12 / peak
    hbm_frac = nbytes / dt / 1e12 / HBM_PEAK_TBPS
    row = {"row": "H/hifigan_bf16x3", "arm": "bf16x3", "metric": f"HiFi-GAN {key} generator, fp32 tensors, split-bf16 products, {B} x {cfg['num_mels']} x {frames} mel, ms per call (device events)",
           "config": key, "batch": B, "frames": frames, "flop": flop, "algorithmic_bytes": nbytes,
           "arms": {"hip_bf16x3": {"reps_ms": t, "median_ms": med["hip_bf16x3"], "min_ms": min(t), "max_ms": max(t),
                                   "spread_frac": (max(t) - min(t)) / med["hip_bf16x3"]}},
           "value": med["hip_bf16x3"], "unit": "ms", "samples_per_sec": samples / dt, "rtf": samples / dt / rate,
           "roofline": {"kernel": "hg_conv_bf16x3_kernel (all launches of the call)", "bound": "hbm" if hbm_frac >= mfma_frac else "mfma",
                        "mfma": {"achieved": flop / dt / 1e12, "peak": peak, "unit": "TFLOP/s", "frac": mfma_frac},
                        "hbm": {"achieved": nbytes / dt / 1e12, "peak": HBM_PEAK_TBPS, "unit": "TB/s", "frac": hbm_frac},
                        "frac": max(hbm_frac, mfma_frac), "traffic": "algorithmic bytes from the shapes, not counters"}}
    if "hip" in med:
        row["hip_f32_over_hip_bf16x3"] = med["hip"] / med["hip_bf16x3"]
        d = (outs["hip_bf16x3"].double() - outs["hip"].double())
        row["hip_bf16x3_vs_hip_f32_rel_rms"] = float(d.pow(2).mean().sqrt() / outs["hip"].double().pow(2).mean().sqrt())
    return row


def row_tacotron(args, vocoder=None):
    """``vocoder``: a WaveGlow (config 2 weights) already on the GPU, or None to build one."""
    from cookietts_amd.tacotron2 import Tacotron2
    hp = synthetic.tacotron_hparams()
    m = Tacotron2(hp)
    m.load_state_dict(synthetic.to_torch(synthetic.tacotron_state_dict(hp, seed=1234)))
    m = m.cuda().eval()
    B, T, steps = 4, 200, 900
    rng = np.random.default_rng(1234)
    text = torch.from_numpy(rng.integers(1, 179, size=(B, T))).cuda()
    lens = torch.tensor([200, 195, 150, 100]).cuda()
    spk = torch.arange(B).cuda()
    tm = torch.from_numpy(rng.standard_normal((B, 2304)).astype(np.float32)).cuda()
    dt = timed(lambda: m.inference(text, lens, spk, tm, fixed_steps=steps), args.warmup, args.steps)
    mem = torch.from_numpy((rng.standard_normal((B, T, 1313)) * 0.5).astype(np.float32)).cuda()
    dd = timed(lambda: m.decoder.inference(mem, lens, fixed_steps=steps), 1, args.steps)
    weights_mb = sum(p.numel() for n, p in m.decoder.named_parameters()
                     if "rnn" in n or "projection" in n or "gate" in n or "query" in n or "prenet" in n) * 4 / 1e6
    # chained vocoder: WaveGlow config 2 weights on the B=4 x 900-frame mel the model just produced
    wg = vocoder
    if wg is None:
        from cookietts_amd import WaveGlow
        wcfg = synthetic.WAVEGLOW_CONFIGS["full"]
        wg = WaveGlow(**wcfg)
        wg.load_state_dict(synthetic.to_torch(synthetic.waveglow_state_dict(wcfg, seed=1234)))
        wg = wg.cuda().eval()
    mel = m.inference(text, lens, spk, tm, fixed_steps=steps)["pred_mel_postnet"].clamp(-11.52, 2.0)
    dv = timed(lambda: wg.infer(mel, sigma=0.6), 1, max(1, args.steps - 1))
    # the same vocoder in the reference's half mode (WaveGlowVocoder.half(): IEEE-half storage + fp16 MFMA from the fp32 masters,
    # inside the 1e-3 waveform bound) - what the _5_infer slot runs after load_hifigan-style .half()
    dv16 = None
    try:
        wg.set_compute_dtype(torch.float16)
        dv16 = timed(lambda: wg.infer(mel, sigma=0.6), 1, max(1, args.steps - 1))
    finally:
        wg.set_compute_dtype(torch.float32)
    samples = B * steps * 256
    # the batch sizes the reference's server decodes per call (text2speech.py:418-424, 537, 554): one batched-form workspace
    server = []
    for Bs in (16, 64, 256):
        mem_s = torch.from_numpy((rng.standard_normal((Bs, T, 1313)) * 0.5).astype(np.float32)).cuda()
        lens_s = torch.full((Bs,), T, dtype=torch.int64).cuda()
        ds = timed(lambda: m.decoder.inference(mem_s, lens_s, fixed_steps=256), 1, max(1, args.steps))
        us = ds / 256 * 1e6
        server.append({"batch": Bs, "us_per_step": us, "mel_frames_per_s": Bs * 256 / ds, "workspaces": len(next(iter(m.decoder._ws.values()))),
                       # a step = one pass over the decoder's weights, whatever the batch; the batched form streams them
                       "roofline": {"kernel": "bg_kernel<CELL> x 3 + query / projection / prenet GEMMs + attention (7 launches per step)",
                                    "bound": "hbm", "achieved": weights_mb / 1e3 / (us * 1e-6), "peak": 8000.0, "unit": "GB/s",
                                    "frac": weights_mb / 1e3 / (us * 1e-6) / 8000.0, "traffic": None}})
        del mem_s
    m.decoder._ws, m.decoder._xchg = {}, {}
    return {"row": "C/config5", "metric": "Tacotron2-TM decoder step time, B=4, 200 symbols, 900 forced steps",
            "value": dd / steps * 1e6, "unit": "us/step", "higher_is_better": False,
            "server_batches": server,
            # common schema (the headline's): SURVEY 8d's algorithmic bytes per step = one pass over the weights.  The persistent
            # form keeps them on the CUs (0.78 MB fetched per step), so `achieved` is the rate a streaming step of this length would need
            "roofline": {"kernel": "taco_persistent_kernel", "bound": "hbm", "achieved": weights_mb / 1e3 / (dd / steps), "peak": 8000.0,
                         "unit": "GB/s", "frac": weights_mb / 1e3 / (dd / steps) / 8000.0, "traffic": 0.78e6},
            "mel_frames_per_s_batch": B * steps / dd, "end_to_end_ms_incl_encoder_postnet": dt * 1e3,
            "dtype": "f32", "decoder_form": m.decoder.persistent_state,
            # SURVEY 8d prices a step as one pass over the decoder's weights.  Since round 4 the persistent decoder keeps them in
            # registers / LDS for the whole launch (PMC: 0.78 MB fetched per step, profiles/r4_09_pmc_*): the figures below say what
            # a STREAMING step would cost, not what this kernel moves - the step is bound by its seven all-gathers
            "decoder_weights_MB": weights_mb,
            "streaming_floor_us_per_step_at_8TBps": weights_mb / 1e3 / 8000.0 * 1e6,
            "fetched_per_step_MB_pmc": 0.78 if m.decoder.persistent_state == "ok" else None,
            "fetched_per_step_source": "profiles/r4_09_pmc_config5_tacotron_resident.json (committed PMC pass, not re-measured in this run)",
            "chained_vocoder_samples_per_s": samples / dv, "chained_vocoder_ms": dv * 1e3,
            "text_to_wave_rtf": samples / (dt + dv) / 22050.0,
            "chained_vocoder_f16_ms": None if dv16 is None else dv16 * 1e3,
            "text_to_wave_rtf_f16_vocoder": None if dv16 is None else samples / (dt + dv16) / 22050.0}


def row_taco_forced(args):
    """Teacher-forced ``Tacotron2.forward`` (the GTA pass) against the free-running ``inference(fixed_steps=400)`` of the same build:
    200 symbols, 400 steps, 16 / 64 / 256 rows, the same prenet masks in both arms.  Per row count two pairs of arms, each pair
    alternated ``--reps`` times in one process after a warm-up of each and timed by device events:
      loop   the decoder loop alone, through the library: ``ctts_taco_decoder_steps_forced_f32`` (five launches per step at 16 rows,
             four above, on a prenet_all computed before) against ``ctts_taco_decoder_steps_f32`` (seven), both on an initialised
             workspace
      call   the whole call: ``forward`` (encoder + prenet-frames + loop + projection + postnet) against ``inference``
    The free-running arms are code this row's commit did not touch: they are the yardstick.  ``clears_10x_spread``: the per-step
    difference of the loop arms is more than ten times the larger of their spreads (max - min over the repetitions).
    ``--arms forced`` (or ``free``) runs one arm alone, for a profiler pass."""
    import ctypes as C
    from cookietts_amd import _lib
    from cookietts_amd.tacotron2 import Tacotron2
    hp = synthetic.tacotron_hparams()
    m = Tacotron2(hp)
    m.load_state_dict(synthetic.to_torch(synthetic.tacotron_state_dict(hp, seed=1234)))
    m = m.cuda().eval()
    dec, lib = m.decoder, _lib.lib()
    TXT, T = 200, 400
    reps = getattr(args, "reps", 5)
    arms_on = [a for a in getattr(args, "arms", "").split(",") if a in ("forced", "free")] or ["forced", "free"]
    rng = np.random.default_rng(1234)
    rows = []
    for B in _batches(args, (16, 64, 256)):
        text = torch.from_numpy(rng.integers(1, hp.n_symbols, size=(B, TXT))).cuda()
        lens = torch.full((B,), TXT, dtype=torch.int64).cuda()
        spk = (torch.arange(B) % hp.n_speakers).cuda()
        tm = torch.from_numpy(rng.standard_normal((B, hp.torchMoji_attDim)).astype(np.float32)).cuda()
        syl = torch.from_numpy(rng.uniform(2.5, 6.5, B).astype(np.float32)).cuda()
        gt = torch.from_numpy(synthetic.synthetic_mel(B, T, hp.n_mel_channels)).cuda()
        masks = torch.from_numpy(synthetic.prenet_dropout_masks(T, B, hp.prenet_dim)).cuda()
        # ---- the loop alone
        dev = text.device
        blob, cfg, st = dec._ensure_packed(dev), dec.c_config(), _lib.stream(dev)
        mem = torch.from_numpy((rng.standard_normal((B, TXT, dec._memory_in_dim)) * 0.5).astype(np.float32)).cuda()
        lens32 = lens.to(torch.int32)
        ws = torch.empty(lib.ctts_taco_decoder_workspace_bytes(C.byref(cfg), B, TXT) // 4, dtype=torch.float32, device=dev)
        pre_bytes = lib.ctts_taco_prenet_frames_bytes(C.byref(cfg), B, T)
        prenet_all = torch.empty(pre_bytes // 4, dtype=torch.float32, device=dev)
        mel = torch.empty(B, hp.n_mel_channels, T, device=dev)
        gate, align = torch.empty(B, T, device=dev), torch.empty(B, T, TXT, device=dev)
        hidden = torch.empty(B, hp.second_decoder_rnn_dim + hp.memory_bottleneck_dim, T, device=dev)
        _lib.check(lib.ctts_taco_prenet_frames_f32(C.byref(cfg), _lib.ptr(blob), _lib.ptr(gt), None, _lib.ptr(masks), _lib.ptr(prenet_all),
                                                  pre_bytes, B, T, st), "ctts_taco_prenet_frames_f32")

        def init():
            _lib.check(lib.ctts_taco_decoder_init_f32(C.byref(cfg), _lib.ptr(blob), _lib.ptr(mem), _lib.ptr(lens32), B, TXT, _lib.ptr(ws),
                                                     ws.numel() * 4, st), "ctts_taco_decoder_init_f32")

        def loop_forced():
            _lib.check(lib.ctts_taco_decoder_steps_forced_f32(C.byref(cfg), _lib.ptr(blob), _lib.ptr(prenet_all), _lib.ptr(align),
                                                              _lib.ptr(hidden), B, TXT, 0, T, T, _lib.ptr(ws), ws.numel() * 4, st),
                       "ctts_taco_decoder_steps_forced_f32")

        def loop_free():
            _lib.check(lib.ctts_taco_decoder_steps_f32(C.byref(cfg), _lib.ptr(blob), _lib.ptr(masks), _lib.ptr(mel), _lib.ptr(gate),
                                                       _lib.ptr(align), B, TXT, 0, T, T, _lib.ptr(ws), st), "ctts_taco_decoder_steps_f32")

        def one(fn):                                       # ms of fn() alone: the workspace is initialised outside the events
            init()
            return _event_ms(fn, 1)
        pairs = {"loop": (("forced", lambda: one(loop_forced)), ("free", lambda: one(loop_free))),
                 "call": (("forced", lambda: _event_ms(lambda: m(gt, lens, text, lens, spk, syl, tm, teacher_force_till=0,
                                                                  p_teacher_forcing=1.0, keep_masks=masks), 1)),
                          ("free", lambda: _event_ms(lambda: m.inference(text, lens, spk, tm, gt_sylps=syl, keep_masks=masks,
                                                                         fixed_steps=T), 1)))}
        row = {"row": "C/taco_forced", "metric": "teacher-forced Tacotron2.forward vs free-running inference(fixed_steps), 200 symbols, "
                                                 "400 steps (device events, arms alternated)", "batch": B, "steps": T, "dtype": "f32",
               "launches_per_step": {"forced": 5 if B <= 16 else 4, "free": 7}, "schedule": "pipelined" if B <= 64 else "plain"}
        for pname, arms in pairs.items():
            arms = [a for a in arms if a[0] in arms_on]
            times = {n: [] for n, _ in arms}
            for n, fn in arms:
                for _ in range(max(1, args.warmup)):
                    fn()
            for _ in range(reps):
                for n, fn in arms:
                    times[n].append(fn())
            stat = {}
            for n, t in times.items():
                med = sorted(t)[len(t) // 2]
                stat[n] = {"reps_ms": t, "median_ms": med, "min_ms": min(t), "max_ms": max(t), "spread_ms": max(t) - min(t),
                           "spread_frac": (max(t) - min(t)) / med}
                if pname == "loop":
                    stat[n]["us_per_step"] = med / T * 1e3
            row[pname] = stat
            if len(stat) == 2:
                diff = stat["free"]["median_ms"] - stat["forced"]["median_ms"]
                spread = max(stat["free"]["spread_ms"], stat["forced"]["spread_ms"])
                row[pname] = dict(stat, free_minus_forced_ms=diff, free_over_forced=stat["free"]["median_ms"] / stat["forced"]["median_ms"],
                                  max_spread_ms=spread, clears_10x_spread=bool(diff > 10 * spread))
        row.update({"value": row["loop"][arms_on[0]]["us_per_step"], "unit": "us/step", "higher_is_better": False})
        rows.append(row)
        del ws, prenet_all, hidden, align, mem, gt, masks
        dec._ws, dec._xchg = {}, {}
        torch.cuda.empty_cache()
    return rows


def row_taco_bf16x3(args):
    """``Decoder.inference(fixed_steps=256)`` above 64 rows with ``set_f32_gemm_mode("bf16x3")`` off / on on the same model: 65, 128
    and 256 rows of 200 symbols, arms alternated ``--reps`` times in one process (device events around the whole call; a change of
    mode repacks the blob, so every timed call follows an untimed one in the same mode).  The fp32 arm is the parent's code path:
    it is the yardstick.  ``clears_10x_spread``: the per-step difference exceeds ten times the larger arm's spread (max - min over
    the repetitions).  ``roofline`` per arm: the cells' FLOPs of a step (three products per operand pair in the split mode) against
    the peak of the MFMA they run on, and the cells' weight bytes of a step against HBM; ``bound`` names the larger fraction."""
    from cookietts_amd.tacotron2 import Tacotron2
    hp = synthetic.tacotron_hparams()
    m = Tacotron2(hp)
    m.load_state_dict(synthetic.to_torch(synthetic.tacotron_state_dict(hp, seed=1234)))
    m = m.cuda().eval()
    dec = m.decoder
    TXT, steps = 200, 256
    reps = getattr(args, "reps", 5)
    rng = np.random.default_rng(1234)
    cell_weights = sum(p.numel() for n, p in dec.named_parameters() if "rnn" in n and "weight" in n)
    peaks = {"f32": ("v_mfma_f32_16x16x4_f32", FP32_MFMA_PEAK_TFLOPS, 1), "bf16x3": ("v_mfma_f32_16x16x32_bf16", F16_MFMA_PEAK_TFLOPS, 3)}
    rows = []
    for B in _batches(args, (65, 128, 256)):
        mem = torch.from_numpy((rng.standard_normal((B, TXT, dec._memory_in_dim)) * 0.5).astype(np.float32)).cuda()
        lens = torch.full((B,), TXT, dtype=torch.int64).cuda()
        masks = torch.from_numpy(synthetic.prenet_dropout_masks(steps, B, hp.prenet_dim)).cuda()

        def call(mode):
            dec.set_f32_gemm_mode(mode)
            dec.inference(mem, lens, keep_masks=masks, fixed_steps=steps)            # (re)packs where the mode changed; untimed
            return _event_ms(lambda: dec.inference(mem, lens, keep_masks=masks, fixed_steps=steps), 1)
        times = {"f32": [], "bf16x3": []}
        for mode in times:
            for _ in range(max(1, args.warmup)):
                call(mode)
        for _ in range(reps):
            for mode in times:
                times[mode].append(call(mode))
        stat = {}
        for mode, t in times.items():
            med = sorted(t)[len(t) // 2]
            us = med / steps * 1e3
            kernel, peak, products = peaks[mode]
            tflops = 2.0 * products * B * cell_weights / (us * 1e-6) / 1e12
            gbs = cell_weights * 4 / 1e9 / (us * 1e-6)
            mfma_frac, hbm_frac = tflops / peak, gbs / 8000.0
            stat[mode] = {"reps_ms": t, "median_ms": med, "us_per_step": us, "spread_us_per_step": (max(t) - min(t)) / steps * 1e3,
                          "roofline": {"kernel": "three cell launches of the step (" + kernel + ")", "bound": "mfma" if mfma_frac >= hbm_frac else "hbm",
                                       "mfma": {"achieved": tflops, "peak": peak, "unit": "TFLOP/s", "frac": mfma_frac},
                                       "hbm": {"achieved": gbs, "peak": 8000.0, "unit": "GB/s", "frac": hbm_frac}}}
        diff = stat["f32"]["us_per_step"] - stat["bf16x3"]["us_per_step"]
        spread = max(stat["f32"]["spread_us_per_step"], stat["bf16x3"]["spread_us_per_step"])
        rows.append({"row": "C/taco_bf16x3", "metric": "Decoder.inference(fixed_steps=256), 200 symbols, f32 GEMM mode off / on (device events, "
                                                       "arms alternated)", "batch": B, "steps": steps, "dtype": "f32", "schedule": "plain",
                     "value": stat["bf16x3"]["us_per_step"], "unit": "us/step", "higher_is_better": False, "f32": stat["f32"],
                     "bf16x3": stat["bf16x3"], "f32_minus_bf16x3_us_per_step": diff, "f32_over_bf16x3": stat["f32"]["us_per_step"] / stat["bf16x3"]["us_per_step"],
                     "max_spread_us_per_step": spread, "clears_10x_spread": bool(diff > 10 * spread), "f32_gemm_mode": "f32 | bf16x3 (the two arms)"})
        del mem, masks
        dec._ws, dec._xchg = {}, {}
        torch.cuda.empty_cache()
    dec.set_f32_gemm_mode(None)
    return rows


def row_taco_forced_bf16x3(args):
    """The teacher-forced loop above 64 rows with ``set_f32_gemm_mode("bf16x3")`` off / on on the same model: 65, 128, 192 and 256
    rows (192 = what GTA.py runs: batch_size 32 x 6), 200 symbols, 400 steps.  Per row count two pairs of arms, each pair alternated
    ``--reps`` times in one process after a warm-up of each and timed by device events:
      loop   the decoder loop alone, through the library, on an initialised workspace and a prenet_all computed before:
             ``ctts_taco_decoder_steps_forced_f32`` on the fp32 blob against ``ctts_taco_decoder_steps_forced_bf16x3`` on the bf16x3
             blob (four launches per step in both)
      call   the whole ``Tacotron2.forward`` (encoder + prenet frames + loop + projection + postnet) in either mode; a change of
             mode repacks the blob, so every timed call follows an untimed one in the same mode
    The fp32 arms are the parent's code path: they are the yardstick.  ``clears_10x_spread``: the difference of the two arms exceeds
    ten times the larger arm's spread (max - min over the repetitions); where it does not, the difference is not claimed."""
    import ctypes as C
    from cookietts_amd import _lib
    from cookietts_amd.tacotron2 import Tacotron2
    hp = synthetic.tacotron_hparams()
    m = Tacotron2(hp)
    m.load_state_dict(synthetic.to_torch(synthetic.tacotron_state_dict(hp, seed=1234)))
    m = m.cuda().eval()
    dec, lib = m.decoder, _lib.lib()
    TXT, T = 200, 400
    reps = getattr(args, "reps", 5)
    rng = np.random.default_rng(1234)
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg, st = dec.c_config(), _lib.stream(dev)
    blobs = {}
    for mode in ("f32", "bf16x3"):                           # both blobs of the one model, kept for the loop arms
        dec.set_f32_gemm_mode(mode)
        blobs[mode] = dec._ensure_packed(dev)
    entry = {"f32": ("ctts_taco_decoder_steps_forced_f32", lib.ctts_taco_decoder_steps_forced_f32),
             "bf16x3": ("ctts_taco_decoder_steps_forced_bf16x3", lib.ctts_taco_decoder_steps_forced_bf16x3)}
    rows = []
    for B in _batches(args, (65, 128, 192, 256)):
        text = torch.from_numpy(rng.integers(1, hp.n_symbols, size=(B, TXT))).cuda()
        lens = torch.full((B,), TXT, dtype=torch.int64).cuda()
        spk = (torch.arange(B) % hp.n_speakers).cuda()
        tm = torch.from_numpy(rng.standard_normal((B, hp.torchMoji_attDim)).astype(np.float32)).cuda()
        syl = torch.from_numpy(rng.uniform(2.5, 6.5, B).astype(np.float32)).cuda()
        gt = torch.from_numpy(synthetic.synthetic_mel(B, T, hp.n_mel_channels)).cuda()
        masks = torch.from_numpy(synthetic.prenet_dropout_masks(T, B, hp.prenet_dim)).cuda()
        mem = torch.from_numpy((rng.standard_normal((B, TXT, dec._memory_in_dim)) * 0.5).astype(np.float32)).cuda()
        lens32 = lens.to(torch.int32)
        ws = torch.empty(lib.ctts_taco_decoder_workspace_bytes(C.byref(cfg), B, TXT) // 4, dtype=torch.float32, device=dev)
        pre_bytes = lib.ctts_taco_prenet_frames_bytes(C.byref(cfg), B, T)
        prenet_all = torch.empty(pre_bytes // 4, dtype=torch.float32, device=dev)
        align = torch.empty(B, T, TXT, device=dev)
        hidden = torch.empty(B, hp.second_decoder_rnn_dim + hp.memory_bottleneck_dim, T, device=dev)
        _lib.check(lib.ctts_taco_prenet_frames_f32(C.byref(cfg), _lib.ptr(blobs["f32"]), _lib.ptr(gt), None, _lib.ptr(masks),
                                                  _lib.ptr(prenet_all), pre_bytes, B, T, st), "ctts_taco_prenet_frames_f32")

        def loop(mode):                                    # ms of the loop alone: the workspace is initialised outside the events
            blob, (name, fn) = blobs[mode], entry[mode]
            _lib.check(lib.ctts_taco_decoder_init_f32(C.byref(cfg), _lib.ptr(blob), _lib.ptr(mem), _lib.ptr(lens32), B, TXT, _lib.ptr(ws),
                                                     ws.numel() * 4, st), "ctts_taco_decoder_init_f32")
            return _event_ms(lambda: _lib.check(fn(C.byref(cfg), _lib.ptr(blob), _lib.ptr(prenet_all), _lib.ptr(align), _lib.ptr(hidden),
                                                   B, TXT, 0, T, T, _lib.ptr(ws), ws.numel() * 4, st), name), 1)

        def call(mode):
            fwd = lambda: m(gt, lens, text, lens, spk, syl, tm, teacher_force_till=0, p_teacher_forcing=1.0, keep_masks=masks)   # noqa: E731
            m.set_f32_gemm_mode(mode)
            fwd()                                              # (re)packs where the mode changed; untimed
            return _event_ms(fwd, 1)
        row = {"row": "C/taco_forced_bf16x3", "metric": "teacher-forced decoder loop and Tacotron2.forward, 200 symbols, 400 steps, f32 GEMM "
                                                        "mode off / on (device events, arms alternated)", "batch": B, "steps": T,
               "dtype": "f32", "schedule": "plain", "launches_per_step": 4, "f32_gemm_mode": "f32 | bf16x3 (the two arms)"}
        for pname, fn in (("loop", loop), ("call", call)):
            times = {"f32": [], "bf16x3": []}
            for mode in times:
                for _ in range(max(1, args.warmup)):
                    fn(mode)
            for _ in range(reps):
                for mode in times:
                    times[mode].append(fn(mode))
            stat = {}
            for mode, t in times.items():
                med = sorted(t)[len(t) // 2]
                stat[mode] = {"reps_ms": t, "median_ms": med, "spread_ms": max(t) - min(t)}
                if pname == "loop":
                    stat[mode].update(us_per_step=med / T * 1e3, spread_us_per_step=(max(t) - min(t)) / T * 1e3)
            diff = stat["f32"]["median_ms"] - stat["bf16x3"]["median_ms"]
            spread = max(stat["f32"]["spread_ms"], stat["bf16x3"]["spread_ms"])
            row[pname] = dict(stat, f32_minus_bf16x3_ms=diff, f32_over_bf16x3=stat["f32"]["median_ms"] / stat["bf16x3"]["median_ms"],
                              max_spread_ms=spread, clears_10x_spread=bool(abs(diff) > 10 * spread))
        row.update({"value": row["loop"]["bf16x3"]["us_per_step"], "unit": "us/step", "higher_is_better": False})
        rows.append(row)
        del ws, prenet_all, hidden, align, mem, gt, masks
        dec._ws, dec._xchg = {}, {}
        torch.cuda.empty_cache()
    m.set_f32_gemm_mode(None)
    return rows


def row_stft(args):
    from cookietts_amd import TacotronSTFT
    taco = TacotronSTFT().cuda()
    B, T = 8, 230400
    y = (torch.rand(B, T, device="cuda") * 2 - 1) * 0.5
    dt = timed(lambda: taco.mel_spectrogram(y), args.warmup, args.steps)
    frames = T // 256 + 1
    flop = 2.0 * B * frames * (1026 * 1024 + 80 * 513)
    return {"row": "D/stft", "metric": "TacotronSTFT.mel_spectrogram, 8 x 230400 samples (1024/256/1024, 80 mel)",
            "value": B * T / dt, "unit": "samples/s", "ms_per_call": dt * 1e3, "dtype": "f32",
            "achieved_tflops_algorithmic": flop / dt / 1e12}


def row_waveglow_ax_untts(args):
    """The vocoder config printed by the reference's _2_ttm/untts/inference.ipynb: ax core, waveflow=False, 24 flows x
    8 x 384, n_group 24, 256-channel mel, conditioning upsampled at model level by a TransposedUpsampleNet (2*3*5) and
    handed to the WNs at sample rate.  Same 5.8375 s clip as the notebook row (468 frames, hop 600, 48 kHz)."""
    from cookietts_amd.waveglow_ax import WaveGlow
    cfg = synthetic.WAVEGLOW_AX_CONFIGS["untts"]
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(synthetic.waveglow_ax_state_dict(cfg, seed=1234)))
    m = m.cuda().eval()
    _mode(m, args)
    rows = []
    for B in _batches(args, (1, 4)):
        F = 468
        mel = torch.from_numpy(synthetic.synthetic_mel(B, F, cfg["n_mel_channels"])).cuda()
        ids = torch.zeros(B, dtype=torch.int64).cuda()
        dt = timed(lambda: m.infer(mel, speaker_ids=ids, sigma=1.0, return_CPU=False), args.warmup, args.steps)
        samples = B * (F - 1) * cfg["hop_length"]
        rows.append({"row": "W5/untts", "metric": "real-time factor (48 kHz), ax WaveGlow waveflow=False, 24 flows x 8 x 384, "
                                                  "upsample_first + TransposedUpsampleNet, 256x468 mel (5.84 s clip)",
                     "value": samples / dt / 48000.0, "unit": "x real time (48 kHz)", "batch": B, "ms_per_call": dt * 1e3,
                     "samples_per_s": samples / dt, "dtype": "f32"})
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="waveflow,tacotron,stft")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--gemm-mode", default="f32", choices=["f32", "bf16x3", "bf16x6"],
                    help="main loop of the rows' fp32 conv-GEMMs, set on each model (model.set_f32_gemm_mode)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "f16"],
                    help="waveglow_ax: f16 = IEEE-half storage of the WN stacks (model.set_compute_dtype(torch.float16))")
    ap.add_argument("--reps", type=int, default=5, help="waveglow_ax_ab, waveglow_ax_sep_ab, taco_forced, taco_bf16x3, taco_forced_bf16x3: repetitions of every arm (alternated)")
    ap.add_argument("--batches", default="", help="comma list: restrict the multi-batch rows (waveglow_ax, waveglow_ax_untts, taco_forced, taco_bf16x3, taco_forced_bf16x3) to these batch sizes (PMC passes)")
    ap.add_argument("--arms", default="hip,torch,hip_f16,torch_f16,hip_bf16x3",
                    help="hifigan: arms to run (hip, hip_f16 or hip_bf16x3 alone for a profiler pass); waveglow_ax_sep_ab: sep, fold; taco_forced: forced, free")
    ap.add_argument("--ks", default="3,7", help="waveglow_ax_sep_ab: comma list of depthwise kernel sizes")
    args = ap.parse_args()
    fns = {"hifigan": row_hifigan, "waveflow": row_waveflow, "waveflow_table": row_waveflow_table, "waveflow_author": row_waveflow_author, "tacotron": row_tacotron, "stft": row_stft,
           "waveglow_ax": row_waveglow_ax_notebook, "waveglow_ax_ab": row_waveglow_ax_notebook_ab, "waveglow_ax_untts": row_waveglow_ax_untts,
           "waveglow_ax_sep_ab": row_waveglow_ax_sep_ab, "taco_forced": row_taco_forced, "taco_bf16x3": row_taco_bf16x3,
           "taco_forced_bf16x3": row_taco_forced_bf16x3}
    for r in args.rows.split(","):
        out = fns[r](args)
        for line in (out if isinstance(out, list) else [out]):
            if "f32_gemm_mode" not in line:                      # (taco_bf16x3 and taco_forced_bf16x3 name their two arms themselves)
                line["f32_gemm_mode"] = line.get("arm") if line.get("arm") in ("f32", "bf16x3") else args.gemm_mode    # set on every model of the row (model.set_f32_gemm_mode)
            print(json.dumps(line), flush=True)
