#!/usr/bin/env python3
"""Bits of the Tacotron2 decoder's per-launch step entry points, for a host-only change of their runner.  Drives the C ABI
through ``cookietts_amd._lib``; default widths, text of 40 symbols, ragged lengths, seeded.

  rows    3, 16, 17, 32, 33, 64, 65, 130
  loop    free-running without / with hidden_out; teacher-forced (prenet_all from ctts_taco_prenet_frames_f32)
  entry   the fp32 entry point on the fp32 blob; the bf16x3 entry point on the bf16x3 blob
  knobs   none; CTTS_TACO_BG_NO_PIPE; at 3 rows also CTTS_TACO_VALU with and without CTTS_TACO_NO_FUSE
  blocks  7 steps as [7], [1, 6], [3, 4], [2, 2, 3] with max_steps = 7, and [7] with max_steps = 9

One JSON line per (rows, loop, entry, knobs); under "blocks" every run of it as "<blocks>/<max_steps>": "<outputs> <workspace>".
outputs = SHA-256 over every output array of the loop (name, then bytes, in name order), workspace = SHA-256 of the whole decoder
workspace after the last block (what a block leaves for the next one); the first 16 hex digits of each are listed - 64 bits, for an
equality check among a few hundred runs - so that the two listings stay small enough to be read next to a diff.

usage: taco_steps_bits.py TREE_ROOT OUT.jsonl      one listing (run each tree in a process of its own)
       taco_steps_bits.py --compare A.jsonl B.jsonl   every digest of B equals A's; within B, at 64 rows or fewer the bf16x3
                                                      entry point's digests equal the fp32 entry point's"""
import ctypes as C
import hashlib
import json
import os
import sys

ROWS = (3, 16, 17, 32, 33, 64, 65, 130)
LOOPS = ("free", "free_hidden", "forced")
ENTRIES = ("f32", "bf16x3")
BLOCKS = (([7], 7), ([1, 6], 7), ([3, 4], 7), ([2, 2, 3], 7), ([7], 9))
TEXT = 40


def compare(a_path, b_path):
    def load(path):
        out = {}
        for r in map(json.loads, open(path)):
            for split, digests in r["blocks"].items():
                out[(r["rows"], r["loop"], r["entry"], r["knobs"], split)] = digests
        return out
    a, b = load(a_path), load(b_path)
    assert a.keys() == b.keys(), f"different runs: {len(a)} vs {len(b)}"
    moved = [k for k in a if a[k] != b[k]]
    for k in moved:
        print("MOVED", k, a[k], b[k])
    twins = [k for k in b if k[2] == "bf16x3" and k[0] <= 64]
    for k in twins:
        if b[k] != b[(k[0], k[1], "f32") + k[3:]]:
            moved.append(k)
            print("BF16X3 != F32", k)
    print(f"{len(a)} runs, {len(twins)} bf16x3 runs at <= 64 rows held to their fp32 twins: " + ("all digests equal" if not moved else f"{len(moved)} DIFFER"))
    return 1 if moved else 0


def main():
    root, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import cookietts_amd
    from cookietts_amd import Tacotron2, synthetic, _lib
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
    assert blobs["bf16x3"].numel() > blobs["f32"].numel()
    n_mel, P, D = dec.n_mel_channels, dec.prenet_dim, dec.second_decoder_rnn_dim + dec.memory_dim
    stream = _lib.stream(dev)
    ptr = _lib.ptr

    def sha(arrays):
        d = hashlib.sha256()
        for name, t in sorted(arrays.items()):
            d.update(name.encode())
            d.update(t.detach().contiguous().cpu().numpy().tobytes())
        return d.hexdigest()[:16]

    def knobs(names):
        for k in ("CTTS_TACO_BG_NO_PIPE", "CTTS_TACO_VALU", "CTTS_TACO_NO_FUSE"):
            os.environ.pop(k, None)
        for k in names:
            os.environ[k] = "1"
        _lib.tuning_reload()
        assert all(_lib.tuning_active(k) for k in names)

    def run(B, loop, entry, blocks, max_steps):
        rng = np.random.default_rng(1000 + B)
        mem = torch.from_numpy((rng.standard_normal((B, TEXT, synthetic.tacotron_memory_in_dim(hp))) * 0.5).astype(np.float32)).to(dev)
        lens = np.sort(rng.integers(12, TEXT + 1, size=B))[::-1].copy()
        lens[0] = TEXT
        lens = torch.from_numpy(lens.astype(np.int32)).to(dev)
        masks = torch.from_numpy(synthetic.prenet_dropout_masks(max_steps, B, P, seed=2000 + B)).to(device=dev, dtype=torch.uint8).contiguous()
        blob = blobs[entry]
        ws_bytes = _lib.nbytes(lib.ctts_taco_decoder_workspace_bytes, C.byref(cfg), B, TEXT, what="workspace")
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
        mel = torch.zeros(B, n_mel, max_steps, dtype=torch.float32, device=dev)
        gate = torch.zeros(B, max_steps, dtype=torch.float32, device=dev)
        align = torch.zeros(B, max_steps, TEXT, dtype=torch.float32, device=dev)
        hidden = torch.zeros(B, D, max_steps, dtype=torch.float32, device=dev)
        arrays = {"align": align}
        if loop == "forced":
            frames = torch.from_numpy(synthetic.synthetic_mel(B, max_steps, n_mel, seed=3000 + B)).to(dev).contiguous()
            pre_bytes = _lib.nbytes(lib.ctts_taco_prenet_frames_bytes, C.byref(cfg), B, max_steps, what="prenet frames")
            prenet_all = torch.empty(pre_bytes // 4, dtype=torch.float32, device=dev)
            _lib.check(lib.ctts_taco_prenet_frames_f32(C.byref(cfg), ptr(blob), ptr(frames), None, ptr(masks), ptr(prenet_all), pre_bytes,
                                                      B, max_steps, stream), "prenet_frames")
            arrays.update(hidden=hidden)
        else:
            arrays.update(mel=mel, gate=gate)
            if loop == "free_hidden":
                arrays["hidden"] = hidden
        _lib.check(lib.ctts_taco_decoder_init_f32(C.byref(cfg), ptr(blob), ptr(mem), ptr(lens), B, TEXT, ptr(ws), ws_bytes, stream), "init")
        step0 = 0
        for n in blocks:
            if loop == "forced":
                fn = lib.ctts_taco_decoder_steps_forced_f32 if entry == "f32" else lib.ctts_taco_decoder_steps_forced_bf16x3
                rc = fn(C.byref(cfg), ptr(blob), ptr(prenet_all), ptr(align), ptr(hidden), B, TEXT, step0, n, max_steps, ptr(ws), ws_bytes, stream)
            else:
                fn = lib.ctts_taco_decoder_steps_hidden_f32 if entry == "f32" else lib.ctts_taco_decoder_steps_bf16x3
                rc = fn(C.byref(cfg), ptr(blob), ptr(masks), ptr(mel), ptr(gate), ptr(align), ptr(hidden) if loop == "free_hidden" else None,
                        B, TEXT, step0, n, max_steps, ptr(ws), stream)
            _lib.check(rc, "steps")
            step0 += n
        torch.cuda.synchronize()
        return sha(arrays) + " " + sha({"": ws})

    with open(out_path, "w") as f:
        for B in ROWS:
            sets = [(), ("CTTS_TACO_BG_NO_PIPE",)]
            if B == 3:
                sets += [("CTTS_TACO_VALU",), ("CTTS_TACO_VALU", "CTTS_TACO_NO_FUSE")]
            for ks in sets:
                knobs(ks)
                for loop in LOOPS:
                    for entry in ENTRIES:
                        runs = {"+".join(map(str, blocks)) + f"/{max_steps}": run(B, loop, entry, blocks, max_steps) for blocks, max_steps in BLOCKS}
                        f.write(json.dumps({"rows": B, "loop": loop, "entry": entry, "knobs": "+".join(k[5:] for k in ks), "blocks": runs}) + "\n")
                        f.flush()
            print(f"rows {B}: done", flush=True)
    knobs(())
    print("done", flush=True)


if __name__ == "__main__":
    sys.exit(compare(sys.argv[2], sys.argv[3]) if sys.argv[1] == "--compare" else main())
