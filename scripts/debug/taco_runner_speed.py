#!/usr/bin/env python3
"""Step time of the Tacotron2 decoder's per-launch loops, and of one WaveFlow call, in two checkouts alternated: the check that a
host-only change of the step runner and of the LDS opt-in did not make the enqueue heavier.  One child process per checkout and
repeat (a process loads one library); text of 200 symbols, 256 steps in one block, host clock around a device synchronise.

  free-running and teacher-forced loop, fp32 entry points, 16 / 32 / 64 / 128 / 256 rows       us per step
  both loops, bf16x3 entry points on the bf16x3 blob, 128 / 256 rows                           us per step
  WaveFlow config 4 (synthetic "full"), inverse of 100 frames, B = 1 and 8                     ms per call

The rule: for each row the new median is at most the parent's median plus the parent's own spread (max - min of its repeats).
usage: taco_runner_speed.py PARENT_ROOT NEW_ROOT OUT.jsonl [--reps 5]      (exit status 1 if a row misses the rule)
       taco_runner_speed.py --child ROOT                                   (one repeat of every row, one JSON object on stdout)"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

TEXT, STEPS, WF_FRAMES = 200, 256, 100


def child(root):
    root = os.path.abspath(root)
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import cookietts_amd
    from cookietts_amd import Tacotron2, WaveFlow, synthetic, _lib
    assert os.path.dirname(os.path.dirname(os.path.abspath(cookietts_amd.__file__))) == root, cookietts_amd.__file__
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    hp = synthetic.tacotron_hparams()
    m = Tacotron2(hp)
    m.load_state_dict(synthetic.to_torch(synthetic.tacotron_state_dict(hp, seed=1234)), strict=False)
    dec = m.to(dev).eval().decoder
    cfg = dec.c_config()
    blobs = {"f32": dec._ensure_packed(dev)}
    dec.set_f32_gemm_mode("bf16x3")
    blobs["bf16x3"] = dec._ensure_packed(dev)
    n_mel, P, D = dec.n_mel_channels, dec.prenet_dim, dec.second_decoder_rnn_dim + dec.memory_dim
    stream, ptr = _lib.stream(dev), _lib.ptr
    res = {}

    def timed(fn, scale):        # one warm call, then the median of three
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * scale)
        return statistics.median(ts)

    for entry, rows in (("f32", (16, 32, 64, 128, 256)), ("bf16x3", (128, 256))):
        blob = blobs[entry]
        for B in rows:
            rng = np.random.default_rng(B)
            mem = torch.from_numpy((rng.standard_normal((B, TEXT, synthetic.tacotron_memory_in_dim(hp))) * 0.5).astype(np.float32)).to(dev)
            lens = torch.full((B,), TEXT, dtype=torch.int32, device=dev)
            masks = (torch.rand(STEPS, 2, B, P, device=dev) < 0.5).to(torch.uint8)
            frames = torch.from_numpy(synthetic.synthetic_mel(B, STEPS, n_mel, seed=B)).to(dev).contiguous()
            ws_bytes = _lib.nbytes(lib.ctts_taco_decoder_workspace_bytes, C.byref(cfg), B, TEXT, what="workspace")
            ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
            mel = torch.zeros(B, n_mel, STEPS, device=dev)
            gate = torch.zeros(B, STEPS, device=dev)
            align = torch.zeros(B, STEPS, TEXT, device=dev)
            hidden = torch.zeros(B, D, STEPS, device=dev)
            pre_bytes = _lib.nbytes(lib.ctts_taco_prenet_frames_bytes, C.byref(cfg), B, STEPS, what="prenet frames")
            prenet_all = torch.empty(pre_bytes // 4, dtype=torch.float32, device=dev)
            _lib.check(lib.ctts_taco_prenet_frames_f32(C.byref(cfg), ptr(blob), ptr(frames), None, ptr(masks), ptr(prenet_all), pre_bytes, B,
                                                      STEPS, stream), "prenet_frames")
            free_fn = lib.ctts_taco_decoder_steps_hidden_f32 if entry == "f32" else lib.ctts_taco_decoder_steps_bf16x3
            forced_fn = lib.ctts_taco_decoder_steps_forced_f32 if entry == "f32" else lib.ctts_taco_decoder_steps_forced_bf16x3

            def init():
                _lib.check(lib.ctts_taco_decoder_init_f32(C.byref(cfg), ptr(blob), ptr(mem), ptr(lens), B, TEXT, ptr(ws), ws_bytes, stream), "init")

            def free():
                init()
                _lib.check(free_fn(C.byref(cfg), ptr(blob), ptr(masks), ptr(mel), ptr(gate), ptr(align), None, B, TEXT, 0, STEPS, STEPS,
                                   ptr(ws), stream), "steps")

            def forced():
                init()
                _lib.check(forced_fn(C.byref(cfg), ptr(blob), ptr(prenet_all), ptr(align), ptr(hidden), B, TEXT, 0, STEPS, STEPS, ptr(ws),
                                     ws_bytes, stream), "forced steps")
            res[f"taco/free/{entry}/B{B} us_per_step"] = timed(free, 1e6 / STEPS)
            res[f"taco/forced/{entry}/B{B} us_per_step"] = timed(forced, 1e6 / STEPS)
    del dec, m, blobs
    wcfg = synthetic.WAVEFLOW_CONFIGS["full"]
    wf = WaveFlow(**wcfg)
    wf.load_state_dict(synthetic.to_torch(synthetic.waveflow_state_dict(wcfg, seed=78)))
    wf = wf.to(dev).eval()
    for B in (1, 8):
        mel = torch.from_numpy(synthetic.synthetic_mel(B, WF_FRAMES + 1, seed=3)).to(dev)
        z = (torch.randn(B, WF_FRAMES * 256, generator=torch.Generator().manual_seed(3)) * 0.6).to(dev)
        res[f"waveflow/config4/B{B} ms_per_call"] = timed(lambda: wf.inverse(z, mel, return_CPU=False), 1e3)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    argv = sys.argv[1:]
    reps = 5
    if "--reps" in argv:
        i = argv.index("--reps")
        reps = int(argv[i + 1])
        del argv[i:i + 2]
    trees = {"parent": argv[0], "new": argv[1]}
    runs = {"parent": [], "new": []}
    for r in range(reps):
        for name in ("parent", "new"):            # alternated; the first failure ends the run
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", trees[name]], capture_output=True, text=True, timeout=240)
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(f"{name} repeat {r}: exit status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", flush=True)
                return 2
            runs[name].append(json.loads(line[0][7:]))
            print(f"{name} repeat {r}: ok", flush=True)
    missed = []
    with open(argv[2], "w") as f:
        for row in runs["parent"][0]:
            a, b = [x[row] for x in runs["parent"]], [x[row] for x in runs["new"]]
            ma, mb, spread = statistics.median(a), statistics.median(b), max(a) - min(a)
            ok = mb <= ma + spread
            if not ok:
                missed.append(row)
            f.write(json.dumps({"row": row, "parent_median": round(ma, 3), "new_median": round(mb, 3), "parent_spread": round(spread, 3),
                                "within_rule": ok, "parent": [round(x, 3) for x in a], "new": [round(x, 3) for x in b]}) + "\n")
            print(f"{row:44s} parent {ma:9.3f} (spread {spread:6.3f})  new {mb:9.3f}  {'ok' if ok else 'MISS'}", flush=True)
    print("rows that miss the rule: " + (", ".join(missed) if missed else "none"), flush=True)
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(child(sys.argv[2]) if sys.argv[1] == "--child" else main())
