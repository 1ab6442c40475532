"""Float64 parity of the WaveFlow 2-D core (``ctts_waveflow_inverse_f32`` / ``ctts_waveflow_inverse_cond_f32``) in every launch form,
row by row and element by element, against ``waveflow_core_f64_restatement`` - the tighter anchor behind the whole-model
``WAVE_TOL = 1e-3`` RMS tests and the bit-identity tests between forms (which show that the forms agree, not that they are right).

CPU part: the restatement reproduces the reference's goldens (float64 run) and the fp32 oracle (fp32 run) within test_waveflow's own
``ORACLE_TOL``; every ``perturb`` hook moves the float64 output by more than 10 x the bound on the case that is meant to catch it; the
floor carries the bound where e32 is exactly 0 (row 0 of a one-flow PermuteHeight model is a pure move).

GPU part: the C ABI is packed straight from the restatement's numpy weights (no model class in between), so n_flows, kernel, dilations,
unit, separable, mixing and ``cond_precomputed`` are free parameters.  Per latent row r, over all items and columns,

    |hip - ref64|_inf  <=  FACTOR * max(e_r, 4 * 2^-23 * max|ref64_r|),      FACTOR = 8 (ax_cond_f64_restatement.FACTOR)

with e_r the distance of the restatement's own fp32 run (or, where ``ctts_last_gemm_loop()`` reports the split-bf16 loop, of its
split-bf16 variant, floored by the fp32 one) from its float64 run - never a figure of the code under test.  After every call the abort
status must be CTTS_OK and ``ctts_last_gemm_loop()`` must name the loop the case is about (bit 4 small shape, 5 split-K body, 6 row
queue, 7 whole-flow queue, low bits the split level).  Row 0 of every one-flow PermuteHeight case holds z's row bit for bit.  Four
cases repeat a call on a workspace a 50 x larger call has run on in between and must give the same bits.

Every case prints and appends (case, form, loop code, worst row, HIP L-inf, e, ratio = L-inf / max(e_r, floor_r)) to
profiles/waveflow_core_parity.jsonl.

MEASURED RATIOS (MI355X)
ratio = HIP L-inf / max(e_r, floor_r) of the worst row of each case, the bound being 8; "loop" is what ctts_last_gemm_loop() reported.
At these weight scales e32 is 3e-8 ... 4e-7 per row and the floor (about 1e-6 at max|ref| = 2 ... 3) is the larger of the two in most
rows of the fp32 cases, so their ratios sit below 1; the HIP error of those worst rows is 0.5 ... 3.7 of the row's own e32.

    family                                   cases  loop       ratio
    fused C = 64, default                       14  48         0.12 ... 0.37
    fused C = 64, CTTS_F32_NO_SPLITK             8  16         0.14 ... 0.28
    fused C = 64, CTTS_F32_NO_SMALL              9  0          0.14 ... 0.28
    fused C = 64, CTTS_F32_NO_GLDS               8  0          0.14 ... 0.28
    fused C = 64, CTTS_WF_NO_FUSE                4  16         0.20 ... 0.29
    row queue, 128 x 128 body (debug 16)         6  208        0.20 ... 0.28
    row queue, split-K body (debug 32)           7  240        0.18 ... 0.27
    row queue, one launch per row (debug 128)    5  112        0.18 ... 0.27
    CTTS_WF_NO_VEC_INTERP                        2  48         0.24 ... 0.26
    kh 1 / 2 / 3 with dilation_h [1, 2, 1]       6  0 / 48     0.18 ... 0.22
    2 x 5 taps + mel segment                     2  0 / 48     0.23 ... 0.24
    C = 128 dense, and with merge_res_skip       4  0 / 16     0.23 ... 0.25
    units GTRU GTLRU GLU TTU STU GTSU SPTU      14  0 / 16     0.14 ... 0.31
    unit GSIU, GTSRU                             4  0 / 16     0.14 ... 0.24
    units GSIRRU GSIRLRU GSIRRLRU                6  0 / 16     1.57 ... 1.78
    unit GSIRU                                   2  0 / 16     3.17
    separable C = 128 fused, kw 3 / 5 / 7, d 3   8  0          0.21 ... 0.26
    separable C = 256, C = 128 folded            4  0 / 16     0.23 ... 0.26
    separable C = 64 (fused launch, unfused)     3  0 / 16 / 48  0.18 ... 0.20
    two flows (permute x 2, 1x1 conv, early)     8  0 / 48     0.26 ... 0.40
    bf16x6: fp32 where the host routes it        2  48, 0      0.25 ... 0.26
    bf16x6: split loop                           4  6, 22      0.21 ... 0.22
    bf16x3: fp32 split-K range                   1  48         0.26
    bf16x3: split loop (e = the x3 variant's)    5  3, 19      1.00 ... 1.28

The sin(16 x) units sit highest, as expected: the argument 16 x carries 16 times the absolute error of x into a function of slope 1,
and the device's sin sees an fp32 product where float64 keeps it exact; all of them stay below half the bound, so FACTOR is 8 everywhere.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import ax_cond_f64_restatement as acr
import waveflow_core_f64_restatement as wcr
from conftest import GOLDEN, REPO, rms_rel_err
from cookietts_amd import synthetic
from oracle import waveflow_oracle as wf

ORACLE_TOL = 5e-6                      # test_waveflow.ORACLE_TOL
FACTOR = acr.FACTOR
PARITY_LOG = os.path.join(REPO, "profiles", "waveflow_core_parity.jsonl")
B = 3
N_LAYERS = 3
N_MEL = 20                             # not a multiple of the GEMM's 16-row K chunk: the folded segment has a ragged last chunk

# ----------------------------------------------------------------------------------------------------------- the cases ----
def _case(C_=64, G=4, L=129, frames=7, kh=3, kw=3, dil_w=None, dil_h=None, unit='GTU', merge=False, sep=False, folded=False,
          n_flows=1, mixing='permuteheight', mix_first=False, early=(100, 2), seed=3):
    return dict(C=C_, G=G, L=L, frames=frames, kh=kh, kw=kw, dil_w=dil_w, dil_h=dil_h, unit=unit, merge=merge, sep=sep, folded=folded,
                n_flows=n_flows, mixing=mixing, mix_first=mix_first, early=early, seed=seed)


CASES = {}
# the fused dense layer (C = 64, GTU, 3 x 3, dilations 2^i): one column; either side of the 64-column split-K item / queue flag tile;
# either side of the 128- and 256-column tiles; a ragged third tile.  frames 1 (position scale 0), 7 (non-integer ratio), L (identity)
for _L, _G, _F in ((1, 4, 7), (63, 4, 7), (65, 10, 1), (129, 10, 7), (257, 4, 257), (300, 10, 7)):
    for _folded in (False, True):
        CASES[f"c64_L{_L}_{'mel' if _folded else 'cond'}"] = _case(G=_G, L=_L, frames=_F, folded=_folded)
CASES["c64_dil128"] = _case(G=4, L=300, dil_w=[1, 128, 5])            # a fresh segment reaches a whole neighbouring tile
CASES["c64_dil136"] = _case(G=4, L=129, dil_w=[1, 3, 6])              # not 2^i
# structure
for _kh in (1, 2, 3):
    CASES[f"kh{_kh}_dh121"] = _case(G=10, kh=_kh, dil_h=[1, 2, 1])    # ring deeper than kh, a_min on rows 0 .. 3
CASES["k2x5_mel"] = _case(G=10, kh=2, kw=5, dil_h=[1, 2, 1], folded=True)   # 10 taps + the mel segment
CASES["c128"] = _case(C_=128)
CASES["c128_merge"] = _case(C_=128, merge=True)
for _u in wcr.UNITS[1:]:
    CASES[f"unit_{_u}"] = _case(unit=_u)
for _kw in (3, 5, 7):
    CASES[f"sep128_k{_kw}"] = _case(C_=128, sep=True, kw=_kw, dil_w=[1, 2, 4], L=300 if _kw == 3 else 129)
CASES["sep128_d3"] = _case(C_=128, sep=True, dil_w=[3, 6, 3])        # not the vector depthwise kernel
CASES["sep256"] = _case(C_=256, sep=True)
CASES["sep64_k5"] = _case(sep=True, kw=5, dil_w=[1, 2, 4])           # the depthwise stage in front of the fused dense layer's launch
CASES["sep128_mel"] = _case(C_=128, sep=True, folded=True)
CASES["two_permute"] = _case(n_flows=2)
CASES["two_permute_mixfirst"] = _case(n_flows=2, mix_first=True)
CASES["two_conv1x1"] = _case(n_flows=2, mixing='1x1conv', mix_first=True)
CASES["two_early"] = _case(n_flows=2, G=10, early=(1, 2))             # flow 1 on 8 rows, the chunk re-joins in front

KNOBS = {
    "default": (),
    "no_splitk": (("CTTS_F32_NO_SPLITK", "1"),),
    "no_small": (("CTTS_F32_NO_SMALL", "1"),),
    "no_glds": (("CTTS_F32_NO_GLDS", "1"),),
    "no_fuse": (("CTTS_WF_NO_FUSE", "1"),),
    "queue_small": (("CTTS_WF_ROW_QUEUE_MIN", "1"), ("CTTS_WF_QUEUE_DEBUG", "16")),
    "queue_splitk": (("CTTS_WF_ROW_QUEUE_MIN", "1"), ("CTTS_WF_QUEUE_DEBUG", "32")),
    "queue_per_row": (("CTTS_WF_ROW_QUEUE_MIN", "1"), ("CTTS_WF_QUEUE_DEBUG", "128")),
    "no_vec_interp": (("CTTS_WF_NO_VEC_INTERP", "1"),),
}
MODES = {"f32": (0, 0), "bf16x3": (2, 3), "bf16x6": (3, 6)}          # name -> (CTTS_GEMM_*, split level)

RUNS = []                                                             # (case, form, mode)
for _L in (1, 65, 257, 300):
    for _c in ("cond", "mel"):
        RUNS += [(f"c64_L{_L}_{_c}", f, "f32") for f in ("default", "no_splitk", "no_small", "no_glds")]
RUNS += [("c64_L63_cond", "default", "f32"), ("c64_L63_mel", "default", "f32")]
for _L in (129, 300):
    for _c in ("cond", "mel"):
        RUNS += [(f"c64_L{_L}_{_c}", f, "f32") for f in ("no_fuse", "queue_small", "queue_splitk", "queue_per_row")]
    RUNS += [(f"c64_L{_L}_cond", "no_vec_interp", "f32")]
RUNS += [("c64_L129_cond", "default", "f32"), ("c64_L129_mel", "default", "f32")]
RUNS += [("c64_L63_cond", f, "f32") for f in ("queue_small", "queue_splitk", "queue_per_row")]
RUNS += [("c64_dil128", f, "f32") for f in ("queue_small", "queue_splitk", "default")]
RUNS += [("c64_dil136", f, "f32") for f in ("default", "no_small", "queue_splitk")]
_SHAPE_OR_FORM = {n for n in CASES if n.startswith("c64_")}
RUNS += [(n, f, "f32") for n in CASES if n not in _SHAPE_OR_FORM for f in ("default", "no_small")]
RUNS += [("sep64_k5", "no_fuse", "f32")]
# f32_gemm_mode: the host routes some launches to fp32 MFMA (the fused layer's split-K range, the fused separable layer under x6)
for _m in ("bf16x6", "bf16x3"):
    RUNS += [("c64_L129_cond", "default", _m), ("c64_L129_cond", "no_splitk", _m), ("c64_L129_mel", "no_splitk", _m),
             ("c128", "default", _m), ("c128", "no_small", _m), ("sep128_k5", "default", _m)]


def expected_loop(c, form, mode):
    """What ``ctts_last_gemm_loop()`` must report after the call: the LAST conv-GEMM launch of the last row (include/cookietts_hip.h,
    "Which loop a launch really runs")."""
    knobs = {k for k, _ in KNOBS[form]}
    level = MODES[mode][1]
    no_glds, no_small = "CTTS_F32_NO_GLDS" in knobs, "CTTS_F32_NO_SMALL" in knobs
    no_splitk, no_fuse = "CTTS_F32_NO_SPLITK" in knobs, "CTTS_WF_NO_FUSE" in knobs
    if c["sep"] and c["C"] == 128 and not c["folded"] and not no_fuse:      # the fused separable layer: fp32 MFMA unless bf16x3
        return 3 if level == 3 else 0
    if c["C"] == 64 and c["unit"] == 'GTU' and not no_fuse:
        if "CTTS_WF_ROW_QUEUE_MIN" in knobs:
            assert level == 0 and not no_glds and not no_small and not c["sep"]
            return {"queue_small": 16 | 64 | 128, "queue_splitk": 16 | 32 | 64 | 128, "queue_per_row": 16 | 32 | 64}[form]
        if no_glds or no_small:
            return 0 if no_glds else level                                  # the 128 x 256 shape
        assert -(-c["L"] // 256) * B <= 128
        if level:
            return level if no_splitk else 16 | 32                         # split modes: fp32 split-K in its range, else the split loop
        return 16 if no_splitk else 16 | 32
    # two launches per layer: the last one is the res/skip GEMM (128-row packing)
    if no_glds:
        return 0
    return level if no_small else 16 | level


# ------------------------------------------------------------------------------------------------------ the reference ----
def _cfg_of(c):
    return synthetic.waveflow_config(
        n_flows=c["n_flows"], n_group=c["G"], n_channels=c["C"], n_layers=N_LAYERS, kernel_size_w=c["kw"], kernel_size_h=c["kh"],
        n_mel_channels=N_MEL, channel_mixing=c["mixing"], mix_first=c["mix_first"], n_early_every=c["early"][0],
        n_early_size=c["early"][1],
        WN=dict(n_layers_dilations_w=c["dil_w"], n_layers_dilations_h=c["dil_h"] or [1] * N_LAYERS, gated_unit=c["unit"],
                merge_res_skip=c["merge"], seperable_conv=c["sep"]))


@functools.lru_cache(maxsize=None)
def _inputs(name, variant=0):
    """(p, weights, z, cond | None, mel | None) of a case; ``variant`` 1 = other inputs of the same geometry, 50 x larger."""
    c = CASES[name]
    cfg = _cfg_of(c)
    p = wcr.params(cfg)
    sd = synthetic.waveflow_state_dict(cfg, seed=c["seed"])
    weights = [wcr.flow_weights(sd, cfg, k, folded=c["folded"]) for k in range(c["n_flows"])]
    rng = np.random.default_rng(1000 * c["seed"] + c["L"] + 7 * variant)
    scale = np.float32(50.0 if variant else 1.0)
    z = (rng.standard_normal((B, c["G"] * c["L"]), dtype=np.float32) * np.float32(0.6) * scale).astype(np.float32)
    cond = mel = None
    if c["folded"]:
        mel = (synthetic.synthetic_mel(B, c["frames"], seed=c["seed"] + variant)[:, :N_MEL] * scale).astype(np.float32)
        assert mel.shape == (B, N_MEL, c["frames"])
    else:
        cond = (rng.standard_normal((c["n_flows"], B, 2 * c["C"] * N_LAYERS, c["frames"]), dtype=np.float32)
                * np.float32(0.5) * scale).astype(np.float32)
    return p, weights, z, cond, mel


@functools.lru_cache(maxsize=None)
def _reference(name, x3=False):
    """float64 audio, and the restatement's own fp32 (or split-bf16) run on the same inputs: computed once, shared, never changed."""
    p, weights, z, cond, mel = _inputs(name)
    if x3:
        y = wcr.inverse(weights, p, z, cond=cond, mel=mel, dtype=np.float64, x3=True)
        y.setflags(write=False)
        return y
    y64 = wcr.inverse(weights, p, z, cond=cond, mel=mel, dtype=np.float64)
    y32 = wcr.inverse(weights, p, z, cond=cond, mel=mel, dtype=np.float32)
    assert y32.dtype == np.float32 and np.isfinite(y64).all()
    y64.setflags(write=False)
    y32.setflags(write=False)
    return y64, y32


def _pass_row(c):
    """(output row, z row) of the row a one-flow PermuteHeight model only moves."""
    perm = wf.permutation(0, c["G"])
    return (perm.index(0), 0) if c["mix_first"] else (0, perm[0])


# ---------------------------------------------------------------------------------------------------------- CPU tests ----
PINNED = ["toy", "toy_dilations_h", "toy_merge", "toy_conv_early", "toy_permute_mixfirst_early", "author_toy"]


@pytest.mark.parametrize("name", PINNED)
def test_restatement_matches_reference_golden(name):
    """cond_frames + the core restatement in float64 reproduce the reference's ``inverse`` output; the fp32 run agrees with the fp32
    oracle - both within test_waveflow's bound for its oracle."""
    g = np.load(os.path.join(GOLDEN, f"waveflow_{name}.npz"))
    cfg = synthetic.WAVEFLOW_CONFIGS[str(g["config_key"])]
    sd = synthetic.waveflow_state_dict(cfg, seed=int(g["seed"]))
    ids = g["speaker_ids"] if "speaker_ids" in g.files else None
    melp = np.pad(g["mel"], ((0, 0), (0, 0), (0, 1)))
    p = wcr.params(cfg)
    L = g["z"].shape[1] // p["n_group"]
    weights = [wcr.flow_weights(sd, cfg, k) for k in range(p["n_flows"])]
    out = {}
    for dtype in (np.float64, np.float32):
        frames, T = acr.cond_frames(sd, cfg, melp, ids, L, dtype)
        assert T != L                                                     # the core's own lerp is on the path
        y = wcr.inverse(weights, p, g["z"], cond=frames, dtype=dtype)
        assert y.dtype == dtype
        if cfg.get("preempthasis"):                                       # ax:351-355, behind the core
            y = acr.deemphasis64(y, cfg["preempthasis"]).astype(dtype)
        out[dtype] = y
    d64 = rms_rel_err(out[np.float64], g["inverse_full"])
    d32 = rms_rel_err(out[np.float32], wf.waveflow_inverse(sd, cfg, g["z"], melp, ids))
    print(f"{name}: float64 restatement vs golden {d64:.2e}, fp32 restatement vs fp32 oracle {d32:.2e}")
    assert d64 < ORACLE_TOL and d32 < ORACLE_TOL


# hook -> the GPU case that is meant to catch it
CAUGHT_BY = {'tap_row': "kh3_dh121", 'first_rows': "kh2_dh121", 'halo': "c64_L65_cond", 'lerp_shift': "c64_L129_cond",
             'skip_init': "c64_L129_mel", 'end_rows': "c64_L63_cond"}


@pytest.mark.parametrize("hook", wcr.PERTURBATIONS)
def test_every_perturbation_matters(hook):
    name = CAUGHT_BY[hook]
    c = CASES[name]
    p, weights, z, cond, mel = _inputs(name)
    y64, y32 = _reference(name)
    _, bound = wcr.row_bounds(y32, y64, c["G"])
    bad = wcr.inverse(weights, p, z, cond=cond, mel=mel, dtype=np.float64, perturb=(hook,))
    d = np.abs(wcr.rows_of(bad, c["G"]) - wcr.rows_of(y64, c["G"])).max(axis=(0, 2))
    ratio = d / bound
    print(f"{hook} on {name}: largest distance / bound per row {np.array2string(ratio, precision=1)}")
    assert ratio.max() > 10, (hook, name, ratio)


def test_perturbation_cases_have_what_the_hooks_need():
    assert all(name in {r[0] for r in RUNS} for name in CAUGHT_BY.values())
    assert CASES[CAUGHT_BY['first_rows']]["kh"] >= 2 and CASES[CAUGHT_BY['tap_row']]["kh"] >= 2
    assert CASES[CAUGHT_BY['lerp_shift']]["frames"] != CASES[CAUGHT_BY['lerp_shift']]["L"]
    assert CASES[CAUGHT_BY['halo']]["kw"] >= 3


def test_floor_carries_the_bound_where_e32_is_zero():
    """Row 0 of a one-flow PermuteHeight model is a pure move: e32 is exactly 0 there and the bound is the floor alone."""
    for name in ("c64_L129_cond", "kh3_dh121", "sep128_k5"):
        c = CASES[name]
        y64, y32 = _reference(name)
        e, bound = wcr.row_bounds(y32, y64, c["G"])
        out_row, z_row = _pass_row(c)
        r64 = wcr.rows_of(y64, c["G"])
        assert e[out_row] == 0.0 and np.all(e[np.arange(c["G"]) != out_row] > 0)
        assert bound[out_row] == FACTOR * 4 * acr.EPS32 * np.abs(r64[:, out_row]).max() > 0
        assert np.array_equal(r64[:, out_row], wcr.rows_of(_inputs(name)[2], c["G"])[:, z_row].astype(np.float64))


def test_bound_helper_takes_the_larger_of_e32_and_floor():
    y64 = np.array([[1.0, 100.0, 2.0, 200.0]])                            # G = 2: rows (1, 2) and (100, 200)
    y32 = y64 + np.array([[1e-3, 0.0, 0.0, 1e-7]])
    e, bound = wcr.row_bounds(y32, y64, 2)
    assert np.allclose(e, [1e-3, 1e-7]) and np.allclose(bound, [FACTOR * 1e-3, FACTOR * 4 * acr.EPS32 * 200.0])
    e, bound = wcr.row_bounds(y32, y64, 2, y_x3=y64 + 0.5)
    assert np.allclose(e, [0.5, 0.5])


def test_expected_loop_table_is_complete():
    for name, form, mode in RUNS:
        assert 0 <= expected_loop(CASES[name], form, mode) < 256
    assert len(set(RUNS)) == len(RUNS)


# ---------------------------------------------------------------------------------------------------------- GPU side ----
class _Device:
    """One packed model on the device, straight from numpy weights through the C ABI."""

    def __init__(self, name, mode="f32"):
        import torch
        from cookietts_amd import _lib
        self.torch, self._lib, self.lib = torch, _lib, _lib.lib()
        c = self.c = CASES[name]
        p, weights, _, _, _ = _inputs(name)
        self.dev = torch.device("cuda", torch.cuda.current_device())
        n = N_LAYERS
        self.cfg = _lib.WaveFlowConfig(
            n_mel_channels=N_MEL, n_flows=c["n_flows"], n_group=c["G"], n_layers=n, n_channels=c["C"], kernel_size_w=c["kw"],
            kernel_size_h=c["kh"], dilation_h=1, seperable_conv=1 if c["sep"] else 0, cond_precomputed=0 if c["folded"] else 1,
            gated_unit=_lib.GATED_UNITS[c["unit"]], merge_res_skip=1 if c["merge"] else 0, n_early_every=c["early"][0],
            n_early_size=c["early"][1], mixing=_lib.MIX_CONV1X1 if p["conv_mix"] else _lib.MIX_PERMUTE,
            mix_first=1 if c["mix_first"] else 0, dilation_w=_lib.dilation_array(c["dil_w"], n),
            dilation_h_l=_lib.dilation_array(c["dil_h"], n), f32_gemm_mode=MODES[mode][0])
        nbytes = _lib.nbytes(self.lib.ctts_waveflow_packed_bytes, C.byref(self.cfg), what="ctts_waveflow_packed_bytes")
        self.blob = torch.zeros(nbytes // 4 + 1, dtype=torch.float32, device=self.dev)
        keep = []

        def dev(a):
            t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev)
            keep.append(t)
            return t.data_ptr()

        def arr(items):
            a = (C.c_void_p * n)()
            for i, v in enumerate(items):
                a[i] = dev(v)
            return a
        with torch.cuda.device(self.dev):
            for k, w in enumerate(weights):
                fw = _lib.WaveFlowFlowWeights()
                fw.start_w, fw.start_b, fw.end_w, fw.end_b = dev(w["start_w"]), dev(w["start_b"]), dev(w["end_w"]), dev(w["end_b"])
                fw.in_w, fw.in_b, fw.rs_w, fw.rs_b = arr(w["in_w"]), arr(w["in_b"]), arr(w["rs_w"]), arr(w["rs_b"])
                if c["sep"]:
                    fw.dw_w, fw.dw_b = arr(w["dw_w"]), arr(w["dw_b"])
                if c["folded"]:
                    fw.cond_w, fw.cond_b = dev(w["cond_w"]), dev(w["cond_b"])
                if p["conv_mix"]:
                    fw.w_inverse = dev(w["w_inverse"])
                _lib.check(self.lib.ctts_waveflow_pack_flow(C.byref(self.cfg), k, C.byref(fw), _lib.ptr(self.blob),
                                                            _lib.stream(self.dev)), f"ctts_waveflow_pack_flow({k})")
            torch.cuda.synchronize()
        self.T = c["G"] * c["L"]
        self.ws_bytes = _lib.nbytes(self.lib.ctts_waveflow_workspace_bytes, C.byref(self.cfg), B, self.T,
                                    what="ctts_waveflow_workspace_bytes")

    def workspace(self):
        return self.torch.zeros(self.ws_bytes // 4 + 1, dtype=self.torch.float32, device=self.dev)

    def __call__(self, z, cond, mel, ws):
        """-> (audio [B, T] fp32 numpy, loop code); the abort status must be CTTS_OK."""
        torch, _lib, lib, c = self.torch, self._lib, self.lib, self.c
        frames = c["frames"]
        zz = torch.from_numpy(z).to(self.dev)
        audio = torch.full((B, self.T), float("nan"), dtype=torch.float32, device=self.dev)
        with torch.cuda.device(self.dev):
            stream = _lib.stream(self.dev)
            if c["folded"]:
                m = torch.from_numpy(np.ascontiguousarray(mel)).to(self.dev)
                rc = lib.ctts_waveflow_inverse_f32(C.byref(self.cfg), _lib.ptr(self.blob), _lib.ptr(zz), _lib.ptr(m), _lib.ptr(audio),
                                                   B, self.T, frames, _lib.ptr(ws), self.ws_bytes, stream)
            else:
                pad, ld = 3, 3 + frames + 5                               # cond_ld > cond_pad + frames, zeros in the pad
                buf = torch.zeros(cond.shape[:3] + (ld,), dtype=torch.float32, device=self.dev)
                buf[..., pad:pad + frames] = torch.from_numpy(cond).to(self.dev)
                rc = lib.ctts_waveflow_inverse_cond_f32(C.byref(self.cfg), _lib.ptr(self.blob), _lib.ptr(zz), _lib.ptr(buf), ld, pad,
                                                        _lib.ptr(audio), B, self.T, frames, _lib.ptr(ws), self.ws_bytes, stream)
            _lib.check(rc, "ctts_waveflow_inverse")
            code = lib.ctts_last_gemm_loop()
            _lib.check(lib.ctts_waveflow_abort_status(C.byref(self.cfg), B, self.T, _lib.ptr(ws), self.ws_bytes, stream),
                       "ctts_waveflow_abort_status")
            return audio.cpu().numpy(), code


def _set_knobs(tuning, form):
    for name, value in KNOBS[form]:
        tuning.set(name, value)


def _log(rec):
    print(json.dumps(rec))
    try:
        with open(PARITY_LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


@pytest.mark.gpu
@pytest.mark.parametrize("name,form,mode", RUNS, ids=[f"{n}-{f}-{m}" for n, f, m in RUNS])
def test_core_matches_float64_row_by_row(hip_lib_path, tuning, name, form, mode):
    c = CASES[name]
    _, _, z, cond, mel = _inputs(name)
    y64, y32 = _reference(name)
    d = _Device(name, mode)
    _set_knobs(tuning, form)
    got, code = d(z, cond, mel, d.workspace())
    want = expected_loop(c, form, mode)
    ran_x3 = (code & 15) == 3
    e, bound = wcr.row_bounds(y32, y64, c["G"], y_x3=_reference(name, True) if ran_x3 else None)
    err = np.abs(wcr.rows_of(got.astype(np.float64), c["G"]) - wcr.rows_of(y64, c["G"]))
    err = np.where(np.isnan(err), np.inf, err).max(axis=(0, 2))
    ratio = err / (bound / FACTOR)
    r = int(np.argmax(ratio))
    _log(dict(case=name, form=form, mode=mode, loop=code, worst_row=r, hip_linf=float(err[r]), e=float(e[r]),
              ratio=float(ratio[r])))
    assert code == want, f"{name} / {form} / {mode}: ctts_last_gemm_loop() = {code}, the case is about loop {want}"
    assert np.all(err <= bound), (f"{name} / {form} / {mode} (loop {code}): rows over the bound {np.nonzero(err > bound)[0].tolist()}, "
                                  f"ratio to max(e, floor) per row {np.array2string(ratio, precision=2)}; {wcr.worst(got, y64, c['G'])}")
    if c["n_flows"] == 1:                                                  # the row the flow only moves: z's bits
        out_row, z_row = _pass_row(c)
        assert np.array_equal(wcr.rows_of(got, c["G"])[:, out_row], wcr.rows_of(z, c["G"])[:, z_row])


@pytest.mark.gpu
@pytest.mark.parametrize("name,form", [("c64_L129_cond", "default"), ("c64_L300_mel", "queue_splitk"), ("c128", "default"),
                                       ("sep128_k5", "default")])
def test_workspace_reuse_gives_the_same_bits(hip_lib_path, tuning, name, form):
    """A call on a freshly zeroed workspace, a call with other inputs of the same geometry 50 x larger, the first inputs again: a stale
    ring slot, skip sum or out-row read would show in the third result."""
    _, _, z, cond, mel = _inputs(name)
    _, _, z2, cond2, mel2 = _inputs(name, 1)
    d = _Device(name)
    _set_knobs(tuning, form)
    ws = d.workspace()
    first, code = d(z, cond, mel, ws)
    assert code == expected_loop(CASES[name], form, "f32") and np.isfinite(first).all()
    other, _ = d(z2, cond2, mel2, ws)
    assert not np.array_equal(other, first)
    again, _ = d(z, cond, mel, ws)
    assert np.array_equal(again, first)
