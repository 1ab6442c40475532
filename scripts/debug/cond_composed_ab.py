"""Go / no-go of the composed conditioning at a config's shape: the two forms through their stage entries, alternated.

Arm "composed": ctts_wn_cond_composed_f32 (the padded copy of the mel + the one GEMM).
Arm "chain":    ctts_upsample_squeeze_f32 + ctts_wn_cond_f32 (upsampling launch, cond layer 0, cond layer 1).
Each round times `--calls` back-to-back calls of one arm between two events, then of the other; `--rounds` rounds.  Go: the
composed arm saves at least 5 x the larger arm's spread (max - min of its rounds).

    python scripts/debug/cond_composed_ab.py [--config full] [--batch 8] [--frames 900] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from cookietts_amd import WaveGlow, _lib, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="full")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=900)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = synthetic.WAVEGLOW_CONFIGS[a.config]
    m = WaveGlow(**cfg)
    m.load_state_dict(synthetic.to_torch(synthetic.waveglow_state_dict(cfg, seed=1234)))
    m = m.cuda().eval()
    dev = torch.device("cuda", 0)
    blob, _ = m._ensure_packed(dev)
    assert m._options() == _lib.WG_OPT_COMPOSED_COND, "this config has no composed conditioning"
    lib, c = _lib.lib(), m.c_config()
    B, F = a.batch, a.frames
    geo = _lib.WaveGlowGeometry()
    _lib.check(lib.ctts_waveglow_geometry_for(C.byref(c), F, C.byref(geo)), "geometry")
    n_mel, G, H = cfg["n_mel_channels"], cfg["n_group"], 256
    mel = torch.from_numpy(synthetic.synthetic_mel(B, F, n_mel, seed=1234)).to(dev)
    spect = torch.zeros(B, n_mel * G, geo.ld, device=dev)
    h_tmp = torch.zeros(B, m.n_flows * H, geo.ld, device=dev)
    h_all = torch.zeros_like(h_tmp)
    scratch = torch.zeros(lib.ctts_wn_cond_composed_scratch_bytes(C.byref(c), B, F) // 4, device=dev)
    st = _lib.stream(dev)

    def composed():
        _lib.check(lib.ctts_wn_cond_composed_f32(C.byref(c), _lib.ptr(blob), _lib.ptr(mel), _lib.ptr(scratch), _lib.ptr(h_all), B, F, st), "composed")

    def chain():
        _lib.check(lib.ctts_upsample_squeeze_f32(C.byref(c), _lib.ptr(blob), _lib.ptr(mel), _lib.ptr(spect), B, F, st), "upsample")
        _lib.check(lib.ctts_wn_cond_f32(C.byref(c), _lib.ptr(blob), _lib.ptr(spect), None, _lib.ptr(h_tmp), _lib.ptr(h_all), B, F, st), "cond")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls

    for fn in (composed, chain, composed, chain):       # warm-up
        fn()
    torch.cuda.synchronize()
    ms = {"composed": [], "chain": []}
    for _ in range(a.rounds):
        ms["composed"].append(timed(composed))
        ms["chain"].append(timed(chain))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    saving = med["chain"] - med["composed"]
    P, J = cfg["hop_length"] // G, cfg["win_length"] // cfg["hop_length"]
    gflop = 2.0 * m.n_flows * P * H * J * n_mel * B * F / 1e9
    rec = {"config": a.config, "batch": B, "frames": F, "rounds": a.rounds, "calls_per_round": a.calls, "ms_per_call": ms,
           "median_ms": med, "spread_ms": spread, "saving_ms": saving, "saving_over_larger_spread": saving / max(max(spread.values()), 1e-9),
           "composed_gflop_unpadded": gflop, "composed_tflops_incl_pad_copy": gflop / med["composed"],
           "go": bool(saving >= 5.0 * max(spread.values()))}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
