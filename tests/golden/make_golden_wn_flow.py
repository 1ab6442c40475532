#!/usr/bin/env python3
"""Generate tests/golden/waveglow_flow_f64_<case>.npz: the float64 reference of ONE flow of the fp32 WaveGlow path at the project's
real channel counts, from tests/waveglow_f64_restatement.py (numpy on the CPU; nothing else is read).

    python tests/golden/make_golden_wn_flow.py [case ...]

Data only.  Inputs and weights are never stored: the tests rebuild them from the seeds (numpy generators).  Per case:
  e                 float64 (b, log_s)                 [B][2 n_half][L]
  rows              float64 rows of the latent after coupling and mix   [B][n_rem][L]
  h_scale           RMS of the flow's real cond hidden on synthetic.synthetic_mel: the scale of the drawn hidden
  ref_fp32_vs_fp64  L-inf of the SAME restatement run in fp32 (direct form) against the float64 run, for e and for rows: what the
                    GPU tests scale their bound from
  config, weight_seed, flow, batch, frames, seed
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import waveglow_f64_restatement as wr  # noqa: E402

MAX_FILE = 1 << 20
MAX_TOTAL = 2 << 20


def main(names):
    total = 0
    for name in names or list(wr.FLOW_CASES):
        key, wseed, k, B, F, seed = wr.FLOW_CASES[name]
        t0 = time.time()
        r = wr.compute_flow_case(name)
        path = wr.flow_case_path(name)
        np.savez(path, e=r["e"], rows=r["rows"], h_scale=np.float64(r["h_scale"]), ref_fp32_vs_fp64=r["ref_fp32_vs_fp64"],
                 config=key, weight_seed=wseed, flow=k, batch=B, frames=F, seed=seed)
        size = os.path.getsize(path)
        assert size < MAX_FILE, (name, size)
        print(f"{name}: {time.time() - t0:.1f} s, {size} bytes, h_scale {r['h_scale']:.4f}, max |rows| {np.abs(r['rows']).max():.2f}, "
              f"ref_fp32_vs_fp64 e {r['ref_fp32_vs_fp64'][0]:.3e} rows {r['ref_fp32_vs_fp64'][1]:.3e}")
    total = sum(os.path.getsize(wr.flow_case_path(n)) for n in wr.FLOW_CASES if os.path.exists(wr.flow_case_path(n)))
    assert total < MAX_TOTAL, total
    print(f"all fixtures: {total} bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
