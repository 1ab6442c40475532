#!/usr/bin/env python3
"""Bits of the glow.py WaveGlow's C entry points, for a host-only change of their runner (waveglow_api.hip).  Drives the C ABI
through ``cookietts_amd._lib``; toy sizes, seeded.

  models   synthetic.WAVEGLOW_CONFIGS toy, toy_early, toy_spk_rezero (speaker ids), toy_hop512_g16 (n_group 16) at batch 1 and 3 and
           5, 9, 37 frames (the lengths of tests/test_waveglow_flow_stage_gpu.py: L = 160, 288, 1184 columns, whose pair and quad
           spaces straddle the 64- and 128-column tile edges); one case of small (batch 1, 9 frames: L = 288 is no multiple of
           4 d_max = 512).  The toy models' L = 32 frames is always a multiple of their 4 d_max <= 16.
  entries  infer_spk_f32; waveglow_flow_f32 (flow 0 with and without wave, the last flow); wn_stack_f32 + flow_tail_f32;
           wn_cond_f32; upsample_squeeze_f32; forward_spk_f32; waveglow_flow_forward_f32 (flow 0 from the waveform, the last flow);
           infer_spk_bf16 / _f16 / _bf16x3 (not toy_hop512_g16: the 16-bit flow boundaries hold 8 rows, listed as "refused")
  knobs    KNOBS below, each set followed by ctts_tuning_reload.  On the F(4,3) lines ctts_last_winograd_f43_width() must be 64, with
           CTTS_F32_NO_SMALL 128 - the two lines follow each other, so a fall-back to another form cannot pass on a stale value.
           Every model here has C = 128, H = 256 (small: C = 256), for which wn_winograd_layer_f43_supported holds.

One JSON line per (model, batch, frames); under "knobs" every knob line as "<outputs> <workspace>": the first 16 hex digits (64 bits)
of two SHA-256 digests over the entries in the order above - of every entry's output arrays (entry name, then per array its name and
bytes, in name order) and of the whole workspace after each call (entries without a workspace: the caller's scratch buffers).
Workspaces start zeroed.  --per-entry adds "entries": the same pair for every entry alone, to find which one moved.

usage: waveglow_runner_bits.py TREE_ROOT OUT.jsonl [--per-entry]   one listing (run each tree in a process of its own)
       waveglow_runner_bits.py --compare A.jsonl B.jsonl    every digest of B equals A's
       waveglow_runner_bits.py --speed PARENT_ROOT NEW_ROOT OUT.jsonl [--reps 5]
           the launch-bound case, trees alternated, one child process per tree and repeat: toy infer at batch 1, 9 frames, us per
           call by a host clock around a device synchronise, in three in-layer forms.  Rule per row: the new median is at most the
           parent's median plus the parent's own spread (max - min of its repeats); exit status 1 if a row misses it
       waveglow_runner_bits.py --speed-child ROOT           (one repeat of every row, one JSON object on stdout)"""
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

W = "CTTS_F32_WINOGRAD_"
KNOBS = (
    (),
    (("CTTS_F32_NO_WINOGRAD", "1"),),
    ((W + "MIN", "0"),),
    ((W + "MIN", "0"), (W + "PLAIN", "1")),
    ((W + "MIN", "0"), (W + "FUSED_MIN", "0"), (W + "NO_F43", "1")),
    ((W + "MIN", "0"), (W + "FUSED_MIN", "0"), (W + "F43_MIN", "0")),
    ((W + "MIN", "0"), (W + "FUSED_MIN", "0"), (W + "F43_MIN", "0"), ("CTTS_F32_NO_SMALL", "1")),
    (("CTTS_F32_NO_WN_FOLD", "1"), (W + "MIN", "0")),
    (("CTTS_F32_NO_DEFER_SKIP", "1"),),
    (("CTTS_F32_NO_GLDS", "1"), (W + "MIN", "0"), (W + "FUSED_MIN", "0")),
)
ALL_KNOBS = sorted({k for ks in KNOBS for k, _ in ks})
CASES = [(name, B, F) for name in ("toy", "toy_early", "toy_spk_rezero", "toy_hop512_g16") for B in (1, 3) for F in (5, 9, 37)]
CASES.append(("small", 1, 9))
MODES16 = (("bf16", "bfloat16"), ("f16", "float16"), ("bf16x3", "bf16x3"))
SPEED_ROWS = ((), KNOBS[2], KNOBS[5])


def knob_name(ks):
    return "+".join(k[5:] + ("" if v == "1" else "=" + v) for k, v in ks)


def set_knobs(_lib, ks):
    for k in ALL_KNOBS:
        os.environ.pop(k, None)
    for k, v in ks:
        os.environ[k] = v
    _lib.tuning_reload()


def compare(a_path, b_path):
    def load(path):
        out = {}
        for r in map(json.loads, open(path)):
            for knobs, digests in r["knobs"].items():
                out[(r["model"], r["batch"], r["frames"], knobs)] = (digests, r["entries_run"], tuple(r["refused"]))
        return out
    a, b = load(a_path), load(b_path)
    assert a.keys() == b.keys(), f"different runs: {len(a)} vs {len(b)}"
    moved = [k for k in a if a[k] != b[k]]
    for k in moved:
        print("MOVED", k, a[k], b[k])
    calls, refused = sum(v[1] for v in a.values()), sum(len(v[2]) for v in a.values())
    print(f"{len(a)} lines of {calls} entry runs ({refused} more listed as refused): " +
          ("all digests equal" if not moved else f"{len(moved)} DIFFER"))
    return 1 if moved else 0


def load_tree(root):
    root = os.path.abspath(root)
    sys.path.insert(0, root)
    import cookietts_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(cookietts_amd.__file__))) == root, cookietts_amd.__file__
    return root


class Model:
    """A toy model packed for every arithmetic mode, and what the entry points need of it."""

    def __init__(self, name, dev):
        import torch
        from cookietts_amd import WaveGlow, _lib, synthetic
        self.name, self.dev, self.cfg = name, dev, synthetic.WAVEGLOW_CONFIGS[name]
        sd = synthetic.to_torch(synthetic.waveglow_state_dict(self.cfg, seed=1234))

        def make():
            m = WaveGlow(**self.cfg)
            m.load_state_dict(sd)
            return m.to(dev).eval()
        self.m = make()
        self.blob, self.fwd, _ = self.m._ensure_forward_packed(dev)
        self.c = self.m.c_config()
        self.blob16 = {}
        if self.cfg["n_group"] <= 8:
            for mode, dtype in MODES16:
                m16 = make().set_compute_dtype(getattr(torch, dtype, dtype))
                self.blob16[mode] = m16._ensure_packed(dev)[1]
        wn = self.cfg["WN_config"]
        self.C, self.G, self.n_flows, self.hop = wn["n_channels"], self.cfg["n_group"], self.cfg["n_flows"], self.cfg["hop_length"]
        self.n_mel, self.sdim = self.cfg["n_mel_channels"], wn["speaker_embed_dim"]
        self.n_half = [h for _, h in synthetic.waveglow_flow_channels(self.cfg)]
        torch.cuda.synchronize()


def listing(root, out_path, per_entry=False):
    load_tree(root)
    import numpy as np
    import torch
    from cookietts_amd import _lib
    dev = torch.device("cuda", 0)
    lib, ptr, stream = _lib.lib(), _lib.ptr, _lib.stream(dev)
    H = 256

    def sha(entry, arrays):
        d = hashlib.sha256(entry.encode())
        for name, t in sorted(arrays.items()):
            d.update(name.encode())
            d.update(t.detach().contiguous().cpu().numpy().tobytes())
        return d

    def run_case(md, B, F):
        c, blob = C.byref(md.c), ptr(md.blob)
        geo = _lib.WaveGlowGeometry()
        _lib.check(lib.ctts_waveglow_geometry_for(c, F, C.byref(geo)), "geometry")
        L, ld, pad, G, K0 = geo.steps, geo.ld, geo.pad, md.G, md.n_mel * md.G
        rng = np.random.default_rng(1000 * B + F)

        def dev_of(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

        def padded(rows):          # [B][R][L] -> the padded layout [B][R][ld], zero halo
            t = torch.zeros(B, rows.shape[1], ld, device=dev)
            t[:, :, pad:pad + L] = dev_of(rows)
            return t
        mel = dev_of(rng.standard_normal((B, md.n_mel, F)).astype(np.float32))
        z0 = (rng.standard_normal((B, G, L)) * 0.6).astype(np.float32)
        audio_in = dev_of((rng.standard_normal((B, F * md.hop)) * 0.3).astype(np.float32))
        h_all = padded((rng.standard_normal((B, md.n_flows * H, L)) * 0.5).astype(np.float32))
        spect = padded((rng.standard_normal((B, K0, L)) * 0.5).astype(np.float32))
        ids = dev_of(np.array([3, 500, 17][:B], dtype=np.int64)) if md.sdim else None
        S = (md.sdim + 31) // 32 * 32
        spk = padded((rng.standard_normal((B, md.n_flows * S, L)) * 0.5).astype(np.float32)) if md.sdim else None
        last = md.n_flows - 1

        def ws_of(query):
            n = _lib.nbytes(getattr(lib, query), c, B, F, what=query)
            return torch.zeros(n // 4, dtype=torch.float32, device=dev), n
        res, refused, total = {}, [], (hashlib.sha256(), hashlib.sha256())

        def done(name, outputs, scratch):
            torch.cuda.synchronize()
            pair = (sha(name, outputs), sha(name, scratch))
            for t, d in zip(total, pair):
                t.update(d.digest())
            res[name] = " ".join(d.hexdigest()[:16] for d in pair)

        ws, n = ws_of("ctts_waveglow_workspace_bytes")
        wave = torch.zeros(B, L * G, device=dev)
        _lib.check(lib.ctts_waveglow_infer_spk_f32(c, blob, ptr(mel), ptr(dev_of(z0)), ptr(ids), ptr(wave), B, F, ptr(ws), n, stream), "infer")
        done("infer_spk_f32", {"wave": wave}, {"": ws})
        f43 = lib.ctts_last_winograd_f43_width()

        for name, k, with_wave in (("flow_f32/k0/wave", 0, True), ("flow_f32/k0", 0, False), (f"flow_f32/k{last}", last, False)):
            ws, n = ws_of("ctts_waveglow_workspace_bytes")
            a = dev_of(z0)
            wave = torch.zeros(B, L * G, device=dev) if with_wave else None
            _lib.check(lib.ctts_waveglow_flow_f32(c, blob, k, ptr(a), ptr(h_all), ptr(wave), B, F, ptr(ws), n, stream), name)
            done(name, {"audio": a, **({"wave": wave} if with_wave else {})}, {"": ws})

        for k in sorted({0, last}):
            a = dev_of(z0)
            x, act, out = (torch.zeros(B, md.C, ld, device=dev) for _ in range(3))
            _lib.check(lib.ctts_wn_stack_f32(c, blob, k, ptr(a), ptr(h_all), ptr(x), ptr(act), ptr(out), B, F, stream), "wn_stack")
            _lib.check(lib.ctts_flow_tail_f32(c, blob, k, ptr(out), ptr(a), None, B, F, stream), "flow_tail")
            done(f"wn_stack_f32+flow_tail_f32/k{k}", {"audio": a, "out": out}, {"act": act, "x": x})

        h_tmp, h_out = (torch.zeros(B, md.n_flows * H, ld, device=dev) for _ in range(2))
        _lib.check(lib.ctts_wn_cond_f32(c, blob, ptr(spect), ptr(spk), ptr(h_tmp), ptr(h_out), B, F, stream), "wn_cond")
        done("wn_cond_f32", {"h_all": h_out}, {"h_tmp": h_tmp})

        sp = torch.zeros(B, K0, ld, device=dev)
        _lib.check(lib.ctts_upsample_squeeze_f32(c, blob, ptr(mel), ptr(sp), B, F, stream), "upsample_squeeze")
        done("upsample_squeeze_f32", {"spect": sp}, {})

        ws, n = ws_of("ctts_waveglow_forward_workspace_bytes")
        z = torch.zeros(B, G, L, device=dev)
        log_s = torch.zeros(B, sum(md.n_half), L, device=dev)
        sums = torch.zeros(B, md.n_flows + 1, dtype=torch.float64, device=dev)
        _lib.check(lib.ctts_waveglow_forward_spk_f32(c, blob, ptr(md.fwd), ptr(mel), ptr(audio_in), ptr(ids), ptr(z), ptr(log_s), ptr(sums),
                                                     B, F, ptr(ws), n, stream), "forward")
        done("forward_spk_f32", {"z": z, "log_s": log_s, "sums": sums}, {"": ws})

        for name, k, from_wave in (("flow_forward_f32/k0/wave", 0, True), (f"flow_forward_f32/k{last}", last, False)):
            ws, n = ws_of("ctts_waveglow_forward_workspace_bytes")
            z = torch.zeros(B, G, L, device=dev) if from_wave else dev_of(z0)
            log_s = torch.zeros(B, md.n_half[k], L, device=dev)
            sum_ls = torch.zeros(B, dtype=torch.float64, device=dev)
            _lib.check(lib.ctts_waveglow_flow_forward_f32(c, blob, ptr(md.fwd), k, ptr(z), ptr(audio_in) if from_wave else None, ptr(h_all),
                                                          ptr(log_s), ptr(sum_ls), B, F, ptr(ws), n, stream), name)
            done(name, {"z": z, "log_s": log_s, "sum_log_s": sum_ls}, {"": ws})

        for mode, _ in MODES16:
            name = f"infer_spk_{mode}"
            if mode not in md.blob16:
                refused.append(name)
                continue
            ws, n = ws_of("ctts_waveglow_workspace_bf16x3_bytes" if mode == "bf16x3" else "ctts_waveglow_workspace_bf16_bytes")
            wave = torch.zeros(B, L * G, device=dev)
            _lib.check(getattr(lib, "ctts_waveglow_" + name)(c, blob, ptr(md.blob16[mode]), ptr(mel), ptr(dev_of(z0)), ptr(ids), ptr(wave), B, F,
                                                            ptr(ws), n, stream), name)
            done(name, {"wave": wave}, {"": ws})
        return res, refused, f43, " ".join(t.hexdigest()[:16] for t in total)

    models = {}
    with open(out_path, "w") as f:
        for name, B, F in CASES:
            if name not in models:
                models.clear()
                models[name] = Model(name, dev)
            rec = {"model": name, "batch": B, "frames": F, "knobs": {}}
            for ks in KNOBS:
                set_knobs(_lib, ks)
                res, refused, f43, both = run_case(models[name], B, F)
                if (W + "F43_MIN", "0") in ks:
                    want = 128 if ("CTTS_F32_NO_SMALL", "1") in ks else 64
                    assert f43 == want, f"{name} B={B} F={F} {knob_name(ks)}: F(4,3) layer width {f43}, expected {want}"
                rec["knobs"][knob_name(ks)] = both
                rec.update(entries_run=len(res), refused=refused)
                if per_entry:
                    rec.setdefault("entries", {})[knob_name(ks)] = res
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(f"{name} batch {B} frames {F}: done", flush=True)
    set_knobs(_lib, ())
    print("done", flush=True)
    return 0


def speed_child(root):
    load_tree(root)
    import numpy as np
    import torch
    from cookietts_amd import _lib
    dev = torch.device("cuda", 0)
    lib, ptr, stream = _lib.lib(), _lib.ptr, _lib.stream(dev)
    md = Model("toy", dev)
    B, F, CALLS = 1, 9, 20
    L = F * md.hop // md.G
    rng = np.random.default_rng(7)
    mel = torch.from_numpy(rng.standard_normal((B, md.n_mel, F)).astype(np.float32)).to(dev)
    z = torch.from_numpy((rng.standard_normal((B, md.G, L)) * 0.6).astype(np.float32)).to(dev)
    wave = torch.zeros(B, L * md.G, device=dev)
    res = {}
    for ks in SPEED_ROWS:
        set_knobs(_lib, ks)
        n = _lib.nbytes(lib.ctts_waveglow_workspace_bytes, C.byref(md.c), B, F, what="workspace")
        ws = torch.zeros(n // 4, dtype=torch.float32, device=dev)

        def calls(count):
            for _ in range(count):
                _lib.check(lib.ctts_waveglow_infer_spk_f32(C.byref(md.c), ptr(md.blob), ptr(mel), ptr(z), None, ptr(wave), B, F, ptr(ws), n,
                                                           stream), "infer")
            torch.cuda.synchronize()
        calls(5)
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            calls(CALLS)
            ts.append((time.perf_counter() - t0) * 1e6 / CALLS)
        res[f"toy/B{B}/F{F}/{knob_name(ks) or 'default'} us_per_call"] = statistics.median(ts)
    set_knobs(_lib, ())
    print("RESULT " + json.dumps(res), flush=True)
    return 0


def speed(argv):
    reps = 5
    if "--reps" in argv:
        i = argv.index("--reps")
        reps = int(argv[i + 1])
        del argv[i:i + 2]
    trees = {"parent": argv[0], "new": argv[1]}
    runs = {"parent": [], "new": []}
    for r in range(reps):
        for name in ("parent", "new"):            # alternated; the first failure ends the run
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--speed-child", trees[name]], capture_output=True, text=True,
                               timeout=120)
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
            print(f"{row:60s} parent {ma:9.3f} (spread {spread:6.3f})  new {mb:9.3f}  {'ok' if ok else 'MISS'}", flush=True)
    print("rows that miss the rule: " + (", ".join(missed) if missed else "none"), flush=True)
    return 1 if missed else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if sys.argv[1] == "--speed-child":
        sys.exit(speed_child(sys.argv[2]))
    sys.exit(speed(sys.argv[2:]) if sys.argv[1] == "--speed" else listing(sys.argv[1], sys.argv[2], "--per-entry" in sys.argv[3:]))
