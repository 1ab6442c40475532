"""HiFi-GAN generator at the edges of its plan, in all three formats (csrc/hifigan.hip, hifigan_f16.hip, hifigan_bf16x3.hip over
csrc/hifigan_plan.h): ragged channel counts (Cin % KC != 0, Cin % 8 != 0, M-blocks partly empty, cout % 4 != 0), transposed convs
with kernel == rate, kernel == rate + 2, odd rates and rate 1, resblock kernels of 1 and halos at HG_MAX_HALO, one and four
resblocks per stage, 1- and 2-frame calls, lengths on and just past a column tile, and the C ABI with a strided unaligned mel.

Configs, cases and the restated shape rules: tests/hifigan_edge_cases.py.  Fixtures: tests/golden/hgedge_<config>.npz, the
REFERENCE'S OWN generator in fp32, fp64 and half on the CPU (tests/golden/make_golden_hifigan_edge.py).

Bounds - every one scaled from the reference's own rounding, never from the code under test:

* fp32 path vs the reference's fp32 waveform: relative RMS < WAVE_TOL and L-inf < EDGE_LINF_FACTOR (8) x the config's base, the
  largest ``ref_fp32_vs_fp64`` L-inf over the config's cases (a 12-sample waveform gives a noisy L-inf; the per-sample rounding
  does not depend on the frame count).  8 is FACTOR of tests/test_tacotron_text_side.py, on top of the 1.45 .. 1.91 x the
  existing goldens measure (profiles/r9_01_hifigan_parity.jsonl; test_hifigan.py allows 100).  The five planted faults of
  test_deliberately_wrong_references_are_outside_the_bound land 10 x outside it or further.
* f16 mode: test_hifigan_f16.py's RMS_FACTOR (2) / LINF_FACTOR (4) x the case's ``ref_half_vs_fp32``, against the fp32 fixture
  and against the f16 restatement.
* bf16x3 mode: test_hifigan_bf16x3.py's WAVE_TOL and LINF_FACTOR (100) x the case's own ``ref_fp32_vs_fp64`` L-inf, against the
  fp32 fixture and against the bf16x3 restatement.
* the wide-shape case has no fixture of its own: its bounds scale from the largest figures over the config's fixtures.

Every measured ratio is printed and appended to profiles/r33_01_hifigan_edge_parity.jsonl.  Measured on the MI355X: fp32 L-inf
0.01 .. 2.29 x the base (0.40 .. 2.29 from 7 frames up), f16 0.35 .. 1.21 x / 0.23 .. 1.39 x the reference's half-mode RMS / L-inf,
bf16x3 16.4 .. 92.0 x the case's own reference L-inf (the largest on k4 b2_f2, where its restatement sits at 92.0 x on the CPU as well;
2.8 .. 41.9 x against the restatement); every bit-equality holds.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import REPO, rms_rel_err
from cookietts_amd import HiFiGANGenerator, _lib, synthetic
from cookietts_amd import hifigan as hg
import hifigan_bf16x3_restatement as h3
import hifigan_edge_cases as ec
import hifigan_f16_restatement as h16
import hifigan_restatement as hr

ORACLE_TOL = 5e-6             # tests/test_hifigan.py
WAVE_TOL = 1e-3               # tests/test_hifigan.py
EDGE_LINF_FACTOR = 8.0        # fp32 path, x the config's largest ref_fp32_vs_fp64 L-inf
F16_RMS_FACTOR = 2.0          # tests/test_hifigan_f16.py
F16_LINF_FACTOR = 4.0         # tests/test_hifigan_f16.py
BF16X3_LINF_FACTOR = 100.0    # tests/test_hifigan_bf16x3.py
FAULT_FACTOR = 10.0           # a planted fault must be this far OUTSIDE the fp32 L-inf bound
FORMATS = ("f32", "f16", "bf16x3")
KEYS = tuple(ec.CONFIGS)
ALL_CASES = [(key, ec.case_name(b, f)) for key in KEYS for b, f, _ in ec.CASES[key]]
PARITY_LOG = os.path.join(REPO, "profiles", "r33_01_hifigan_edge_parity.jsonl")
SENTINEL = 0xA5               # byte of the guard zones around the audio buffer and behind the workspace


@functools.lru_cache(maxsize=None)
def _fixture(key):
    cases = dict(ec.load_cases(key))
    for z in cases.values():
        for v in z.values():
            v.setflags(write=False)
    return cases


@functools.lru_cache(maxsize=None)
def _base_linf(key):
    """The config's base: the largest L-inf of the reference's fp32 forward against its fp64 forward over the config's cases."""
    return max(float(z["ref_fp32_vs_fp64"][1]) for z in _fixture(key).values())


@functools.lru_cache(maxsize=None)
def _sd(key, seed):
    return ec.state_dict(key, seed)


@functools.lru_cache(maxsize=None)
def _restated(fmt, key, name):
    """The restatement's waveform of a fixture case (f32: in float64): computed once, shared by the CPU and the GPU tests."""
    z = _fixture(key)[name]
    cfg, sd = ec.CONFIGS[key], _sd(key, int(z["seed"]))
    out = {"f32": hr.generator_np, "f16": h16.generator_np, "bf16x3": h3.generator_np}[fmt](cfg, sd, z["mel"].copy())
    out.setflags(write=False)
    return out


def _linf(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _log(rec):
    print(json.dumps(rec))
    try:
        with open(PARITY_LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


# --------------------------------------------------------------------------- without a GPU ----
def test_edge_configs_stay_out_of_the_shared_tables():
    assert not set(ec.CONFIGS) & set(synthetic.HIFIGAN_CONFIGS)
    listed = {f"hifigan_{n}.npz" for n in hr.golden_cases()}                  # the files the existing parametrisations read
    for key, cfg in ec.CONFIGS.items():
        hg.check_config(cfg)
        assert os.path.isfile(ec.fixture_path(key)) and os.path.basename(ec.fixture_path(key)) == f"hgedge_{key}.npz"
        assert os.path.basename(ec.fixture_path(key)) not in listed and f"hifigan_{key}.npz" not in listed
        assert os.path.getsize(ec.fixture_path(key)) < (1 << 20)


@pytest.mark.parametrize("key", KEYS)
def test_edge_case_inputs_meet_the_conditions(key):
    """The rules the frame counts were chosen by, from the restated shape rule of hifigan_plan.h."""
    cfg, cases = ec.CONFIGS[key], ec.CASES[key]
    frames = [f for _, f, _ in cases]
    assert {1, 2} <= set(frames) and max(frames) <= ec.MAX_FRAMES                      # (a)
    assert {f % 4 for f in frames} == {0, 1, 2, 3}                                     # (b)
    assert sorted(b for b, _, _ in cases).count(3) == 1 and {b for b, _, _ in cases} == {2, 3}
    for b, f, seed in cases:                                                           # the items of a case differ
        mel = ec.mel(key, b, f, seed)
        assert all(not np.array_equal(mel[i], mel[j]) for i in range(b) for j in range(i))
    # (c) every (layer, edge) that some frame count <= MAX_FRAMES reaches at the cases' launch size is reached by a case
    for esz in (4, 2):
        reachable = set().union(*(ec.edges_reached(cfg, 2, f, esz) for f in range(1, ec.MAX_FRAMES + 1)))
        reached = set().union(*(ec.edges_reached(cfg, b, f, esz) for b, f, _ in cases))
        assert reachable <= reached, sorted(reachable - reached)
        assert reachable, key


def _facts(key, esz):
    """What the plan does with a config: {fact: [layer names]}."""
    kc_hi = 32 if esz == 2 else 16
    out = {"ragged_kc": [], "ragged_8": [], "partly_empty_m": [], "cout_not_by_4": [], "m_not_by_4": [], "kc_lo_cin": [], "kc_lo_lds": [],
           "one_tap": [], "halo": {}}
    for l in ec.plan(ec.CONFIGS[key], esz):
        if l.Cin % l.KC:
            out["ragged_kc"].append(l.name)
        if l.Cin % 8:
            out["ragged_8"].append(l.name)
        if l.M % l.BM and l.M > 1:
            out["partly_empty_m"].append(l.name)
        if l.kind == "convt" and l.cout % 4:
            out["cout_not_by_4"].append(l.name)
        if l.M % 4 and l.M > 1:
            out["m_not_by_4"].append(l.name)
        if l.KC < kc_hi:
            out["kc_lo_" + l.kc_rule].append(l.name)
        if l.ntap == 1:
            out["one_tap"].append(l.name)
        out["halo"][l.name] = (l.ntap - 1) * l.dil
    return out


def test_edge_configs_reach_the_edges_they_are_for():
    """The coverage each config is there for, per layer, from the restated plan: a later edit of the plan (block heights, the K
    chunk rule, the tap count of a phase convolution) that silently removes an edge fails here."""
    every = {key: [l.name for l in ec.plan(ec.CONFIGS[key])] for key in KEYS}
    res = {key: [n for n in every[key] if n.startswith("resblocks")] for key in KEYS}
    by_name = {key: {esz: {l.name: l for l in ec.plan(ec.CONFIGS[key], esz)} for esz in (4, 2)} for key in KEYS}

    # r24: channels 13 -> 24 -> 12 -> 6
    for esz in (4, 2):
        f = _facts("r24", esz)
        assert f["ragged_kc"] == every["r24"]                                 # 13, 24, 12, 6 against 16 / 8 (fp32), 32 / 16 (half)
        assert f["ragged_8"] == [n for n in every["r24"] if n != "ups.0"]     # all but the 24 input channels of ups.0
        assert f["partly_empty_m"] == [n for n in every["r24"] if n != "conv_post"]
        assert f["cout_not_by_4"] == ["ups.1"] and by_name["r24"][esz]["ups.1"].cout == 6
        assert set(f["m_not_by_4"]) == {n for n in every["r24"] if by_name["r24"][esz][n].M == 6} and len(f["m_not_by_4"]) == 12
        assert not f["kc_lo_lds"]
    assert _facts("r24", 4)["kc_lo_cin"] == [n for n in every["r24"] if by_name["r24"][4][n].Cin == 6]
    assert _facts("r24", 2)["kc_lo_cin"] == [n for n in every["r24"] if n != "ups.0"]
    u0, u1 = by_name["r24"][4]["ups.0"], by_name["r24"][4]["ups.1"]
    assert (u0.up, u0.ku, u0.ntap, u0.left) == (3, 5, 3, 1)                   # odd rate, kernel = rate + 2: three taps, dead ones per phase
    assert (u1.up, u1.ku, u1.ntap, u1.left) == (2, 2, 1, 0)                   # kernel == rate: one tap, no padding

    # r80: channels 20 -> 80 -> 40 -> 20
    for esz in (4, 2):
        f = _facts("r80", esz)
        assert {f["halo"][n] for n in res["r80"]} >= {128, 120, 126}
        assert by_name["r80"][esz]["ups.0"].M == 200 and by_name["r80"][esz]["ups.0"].MB == 2      # the second block 72 of 128 rows
        assert {(l.M, l.BM) for l in by_name["r80"][esz].values()} == {(80, 128), (200, 128), (40, 64), (20, 32), (1, 32)}
        assert f["partly_empty_m"] == [n for n in every["r80"] if n != "conv_post"]
        assert not f["kc_lo_cin"]
        assert "resblocks.1.convs.1" in f["kc_lo_lds"] and by_name["r80"][esz]["resblocks.1.convs.1"].Cin == 40   # k 11, d 12
    # 20 and 40 channels against chunks of 16 (and 20 against 8); 80 / 16 and 40 / 8 divide
    divides = ["ups.0"] + [n for n in res["r80"] if n.startswith(("resblocks.1.", "resblocks.2."))]
    assert _facts("r80", 4)["ragged_kc"] == [n for n in every["r80"] if n not in divides]
    assert _facts("r80", 4)["kc_lo_lds"] == ["conv_pre", "resblocks.1.convs.0", "resblocks.1.convs.1", "resblocks.2.convs.0",
                                             "resblocks.2.convs.1", "resblocks.4.convs.1"]
    assert _facts("r80", 2)["kc_lo_lds"] == _facts("r80", 4)["kc_lo_lds"]
    u0, u1 = by_name["r80"][4]["ups.0"], by_name["r80"][4]["ups.1"]
    assert (u0.up, u0.ku, u0.ntap) == (5, 11, 3) and (u1.up, u1.ku, u1.ntap) == (4, 6, 3)

    # k1: rate 1, kernel 1, one resblock per stage
    for esz in (4, 2):
        f = _facts("k1", esz)
        assert f["one_tap"] == res["k1"] and len(res["k1"]) == 6 and all(f["halo"][n] == 0 for n in res["k1"])
        u0 = by_name["k1"][esz]["ups.0"]
        assert (u0.kind, u0.up, u0.ku, u0.ntap, u0.left) == ("convt", 1, 3, 3, 1)
    assert len(ec.CONFIGS["k1"]["resblock_kernel_sizes"]) == 1

    # k4: four resblocks per stage, channels 7 -> 16 -> 8 -> 4 -> 2
    assert len(ec.CONFIGS["k4"]["resblock_kernel_sizes"]) == 4 == _lib.HifiganConfig.MAX_KERNELS
    assert _facts("k4", 4)["kc_lo_cin"] == [n for n in every["k4"] if n != "ups.0"]       # 16 input channels: the one high chunk
    assert _facts("k4", 2)["kc_lo_cin"] == every["k4"]
    for esz in (4, 2):
        f = _facts("k4", esz)
        assert f["cout_not_by_4"] == ["ups.2"] and by_name["k4"][esz]["ups.2"].cout == 2
        assert max(f["halo"].values()) == ec.HG_MAX_HALO and by_name["k4"][esz]["resblocks.3.convs.1"].ntap == 9
        # kernel 1 under the low chunk: the split-bf16 tap-pair step with a phantom second half at ntap = 1
        assert [n for n in f["one_tap"] if n.startswith("resblocks")] == [n for n in res["k4"] if int(n.split(".")[1]) % 4 == 0]
        assert by_name["k4"][esz]["ups.0"].ntap == 1 and by_name["k4"][esz]["ups.1"].ntap == 3


@pytest.mark.parametrize("key", KEYS)
def test_edge_fixtures_are_complete(key):
    cfg = ec.CONFIGS[key]
    up = int(np.prod(cfg["upsample_rates"]))
    assert list(_fixture(key)) == [ec.case_name(b, f) for b, f, _ in ec.CASES[key]]
    for (b, f, seed), (name, z) in zip(ec.CASES[key], _fixture(key).items()):
        assert int(z["seed"]) == seed and np.array_equal(z["mel"], ec.mel(key, b, f, seed))
        assert z["audio"].dtype == np.float32 and z["audio_half"].dtype == np.float16
        assert z["audio"].shape == z["audio_half"].shape == (b, 1, f * up)
        rms = float(np.sqrt(np.mean(z["audio"].astype(np.float64) ** 2)))
        assert 0.05 <= rms <= 0.8 and float(np.mean(np.abs(z["audio"]) > 0.999)) <= 0.01
        rel, linf = (float(v) for v in z["ref_fp32_vs_fp64"])
        assert 0 < rel < 5e-6 and 0 < linf < 5e-6
        rel, linf = (float(v) for v in z["ref_half_vs_fp32"])
        assert 1e-4 < rel < 5e-3 and 2e-5 < linf < 1e-2                    # a bound scaled from it is neither vacuous nor zero
        assert abs(rms_rel_err(z["audio_half"], z["audio"]) - rel) < 1e-9 and abs(_linf(z["audio_half"], z["audio"]) - linf) < 1e-9


@pytest.mark.parametrize("key,name", ALL_CASES)
def test_edge_restatement_matches_reference_golden(key, name):
    z = _fixture(key)[name]
    out = _restated("f32", key, name)
    err = rms_rel_err(out, z["audio"])
    bound = max(ORACLE_TOL, 4.0 * float(z["ref_fp32_vs_fp64"][0]))
    print(f"{key} {name}: restatement vs golden rel rms {err:.3e} (bound {bound:.3e})")
    assert out.shape == z["audio"].shape and out.dtype == np.float64
    assert err < bound


@pytest.mark.parametrize("key,name", ALL_CASES)
def test_edge_f16_restatement_matches_reference_golden(key, name):
    z = _fixture(key)[name]
    ref_rel, ref_linf = (float(v) for v in z["ref_half_vs_fp32"])
    out = _restated("f16", key, name)
    assert out.shape == z["audio"].shape and out.dtype == np.float32 and np.isfinite(out).all()
    err, linf = rms_rel_err(out, z["audio"]), _linf(out, z["audio"])
    print(f"{key} {name}: f16 restatement vs fp32 golden rel rms {err:.3e} ({err / ref_rel:.2f} x ref half) linf {linf:.3e} "
          f"({linf / ref_linf:.2f} x)")
    assert err < F16_RMS_FACTOR * ref_rel
    assert linf < F16_LINF_FACTOR * ref_linf


@pytest.mark.parametrize("key,name", ALL_CASES)
def test_edge_bf16x3_restatement_matches_reference_golden(key, name):
    z = _fixture(key)[name]
    out = _restated("bf16x3", key, name)
    assert out.shape == z["audio"].shape and out.dtype == np.float32 and np.isfinite(out).all()
    err, linf = rms_rel_err(out, z["audio"]), _linf(out, z["audio"])
    ref_linf = float(z["ref_fp32_vs_fp64"][1])
    print(f"{key} {name}: bf16x3 restatement vs fp32 golden rel rms {err:.3e} linf {linf:.3e} ({linf / ref_linf:.2f} x the case's "
          f"ref_fp32_vs_fp64 L-inf)")
    assert err < WAVE_TOL
    assert linf < BF16X3_LINF_FACTOR * ref_linf


def test_edge_size_queries_without_gpu(hip_lib_path):
    """All three plans accept the four configs; a hi | lo pair is the fp32 value's 4 bytes, so the split sizes are the fp32 ones.
    The packed sizes are the ones the restated plan of hifigan_edge_cases.py gives - for the shipped configs and the toys as
    well - which pins its block heights, tap counts and K chunks to the library's."""
    lib = _lib.lib()
    for key, cfg in synthetic.HIFIGAN_CONFIGS.items():
        c = hg.c_config(cfg)
        assert lib.ctts_hifigan_packed_bytes(ctypes.byref(c)) == ec.packed_bytes(cfg, 4), key
        assert lib.ctts_hifigan_packed_f16_bytes(ctypes.byref(c)) == ec.packed_bytes(cfg, 2), key
    for key, cfg in ec.CONFIGS.items():
        c = hg.c_config(cfg)
        n = lib.ctts_hifigan_weight_floats(ctypes.byref(c))
        assert n == sum(int(np.prod(shape)) + (shape[1] if tr else shape[0]) for _, shape, tr in synthetic.hifigan_layers(cfg)), key
        p32, p16, p3 = (getattr(lib, hg._ENTRY[f][0])(ctypes.byref(c)) for f in FORMATS)
        assert p32 > 0 and p16 > 0 and p3 == p32, (key, lib.ctts_last_error())
        assert (p32, p16) == (ec.packed_bytes(cfg, 4), ec.packed_bytes(cfg, 2)), key
        for b, f, _ in ec.CASES[key]:
            w32, w16, w3 = (getattr(lib, hg._ENTRY[fmt][2])(ctypes.byref(c), b, f) for fmt in FORMATS)
            assert w32 > 0 and w16 > 0 and w3 == w32, (key, b, f, lib.ctts_last_error())
        HiFiGANGenerator(hg.AttrDict(cfg)).set_compute_dtype(torch.float16).set_f32_gemm_mode("bf16x3")


# the five planted faults, as (folded weights, mel, final slope) -> the same three, edited
def _lose_conv_pre_channel(cfg, w, mel, slope):
    w["conv_pre"][0][:, -1, :] = 0
    return w, mel, slope


def _lose_ups0_channel(cfg, w, mel, slope):
    w["ups.0"][0][-1, :, :] = 0                      # on the folded weight: a zero weight_v row would make the weight norm 0
    return w, mel, slope


def _lose_last_resblock_row(cfg, w, mel, slope):
    n = len(cfg["upsample_rates"]) * len(cfg["resblock_kernel_sizes"]) - 1
    p = f"resblocks.{n}.convs2.2" if cfg["resblock"] == "1" else f"resblocks.{n}.convs.1"
    w[p][0][-1, :, :] = 0
    w[p][1][-1] = 0
    return w, mel, slope


def _slope_01(cfg, w, mel, slope):
    return w, mel, 0.1


def _zero_last_frame(cfg, w, mel, slope):
    mel = mel.clone()
    mel[:, :, -1] = 0
    return w, mel, slope


FAULTS = [
    ("last input channel of conv_pre lost", _lose_conv_pre_channel, ("r24", "r80", "k4")),      # 13, 20, 7 mel channels
    ("last input channel of ups.0 lost", _lose_ups0_channel, ("r24", "k1")),                    # 24 and 40 against chunks of 16
    ("last output row of the last resblock conv lost", _lose_last_resblock_row, ("r24", "r80", "k4")),   # M = 6, 20, 2
    ("slope 0.1 in front of conv_post", _slope_01, KEYS),
    ("last mel frame zeroed", _zero_last_frame, KEYS),
]


@pytest.mark.parametrize("what,plant,keys", FAULTS, ids=[f[0].replace(" ", "_") for f in FAULTS])
def test_deliberately_wrong_references_are_outside_the_bound(what, plant, keys):
    """Each fault, planted in the float64 restatement on the configs where it sits on a ragged edge, at the config's longest case,
    is more than FAULT_FACTOR x the fp32 L-inf bound away from the reference's waveform."""
    for key in keys:
        cfg = ec.CONFIGS[key]
        name, z = list(_fixture(key).items())[-1]
        bound = EDGE_LINF_FACTOR * _base_linf(key)
        with torch.no_grad():
            w = {p: (wt.clone(), b.clone()) for p, (wt, b) in hr.folded_weights(cfg, _sd(key, int(z["seed"])), torch.float64).items()}
            w, mel, slope = plant(cfg, w, torch.from_numpy(z["mel"].copy()).double(), 0.01)
            bad = hr.generator(cfg, w, mel, slope).numpy()
        good = _linf(_restated("f32", key, name), z["audio"])
        ratio = _linf(bad, z["audio"]) / bound
        print(f"{what} on {key} {name}: L-inf {ratio:.3g} x the fp32 bound (the unedited restatement: {good / bound:.3g} x)")
        assert good < bound
        assert ratio > FAULT_FACTOR, (what, key)


# --------------------------------------------------------------------------- on the GPU ----
@functools.lru_cache(maxsize=None)
def _model(key, seed):
    m = HiFiGANGenerator(hg.AttrDict(ec.CONFIGS[key]))
    m.load_state_dict(synthetic.to_torch(_sd(key, seed)))
    return m.to("cuda:0").eval()


def _set(m, fmt):
    """The model switched to one of the three formats."""
    return m.set_compute_dtype(torch.float16 if fmt == "f16" else torch.float32).set_f32_gemm_mode("bf16x3" if fmt == "bf16x3" else "f32")


def _run(key, seed, fmt, mel):
    with torch.no_grad():
        out = _set(_model(key, seed), fmt)(torch.from_numpy(np.array(mel)).to("cuda:0"))
    torch.cuda.synchronize()
    return out


def _check_case(fmt, key, name):
    z = _fixture(key)[name]
    out = _run(key, int(z["seed"]), fmt, z["mel"])
    assert out.dtype == torch.float32 and tuple(out.shape) == z["audio"].shape
    out = out.cpu().numpy()
    base = _base_linf(key)
    err, linf = rms_rel_err(out, z["audio"]), _linf(out, z["audio"])
    rec = {"format": fmt, "config": key, "case": name, "batch": int(z["mel"].shape[0]), "frames": int(z["mel"].shape[2]),
           "rel_rms": err, "linf": linf, "base_ref_fp32_vs_fp64_linf": base, "linf_over_base": linf / base}
    if fmt == "f32":
        rec.update(bound_rel_rms=WAVE_TOL, bound_linf=EDGE_LINF_FACTOR * base)
        checks = [(err, rec["bound_rel_rms"]), (linf, rec["bound_linf"])]
    else:
        want = _restated(fmt, key, name)
        r_err, r_linf = rms_rel_err(out, want), _linf(out, want)
        rec.update(vs_restatement_rel_rms=r_err, vs_restatement_linf=r_linf)
        if fmt == "f16":
            ref_rel, ref_linf = (float(v) for v in z["ref_half_vs_fp32"])
            rec.update(ref_half_vs_fp32_rel_rms=ref_rel, ref_half_vs_fp32_linf=ref_linf, rel_rms_over_ref=err / ref_rel,
                       linf_over_ref=linf / ref_linf, vs_restatement_linf_over_ref=r_linf / ref_linf,
                       bound_rel_rms=F16_RMS_FACTOR * ref_rel, bound_linf=F16_LINF_FACTOR * ref_linf)
        else:
            ref_linf = float(z["ref_fp32_vs_fp64"][1])                       # the case's own figure, as in test_hifigan_bf16x3.py
            rec.update(ref_fp32_vs_fp64_linf=ref_linf, linf_over_ref=linf / ref_linf, vs_restatement_linf_over_ref=r_linf / ref_linf,
                       bound_rel_rms=WAVE_TOL, bound_linf=BF16X3_LINF_FACTOR * ref_linf)
        checks = [(err, rec["bound_rel_rms"]), (linf, rec["bound_linf"]), (r_err, rec["bound_rel_rms"]), (r_linf, rec["bound_linf"])]
    _log(rec)
    assert np.isfinite(out).all()
    for got, bound in checks:
        assert got < bound, rec


@pytest.mark.gpu
@pytest.mark.parametrize("key,name", ALL_CASES)
def test_hifigan_edge_f32_matches_reference_golden(key, name):
    _check_case("f32", key, name)


@pytest.mark.gpu
@pytest.mark.parametrize("key,name", ALL_CASES)
def test_hifigan_edge_f16_matches_reference_golden(key, name):
    _check_case("f16", key, name)


@pytest.mark.gpu
@pytest.mark.parametrize("key,name", ALL_CASES)
def test_hifigan_edge_bf16x3_matches_reference_golden(key, name):
    _check_case("bf16x3", key, name)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("key", KEYS)
def test_hifigan_edge_batch_item_equals_single_call_bit_for_bit(key, fmt):
    """Item i of the B = 3 case equals the B = 1 call on the same mel bit for bit: the K order of a column's sum is a function of
    the layer and its K chunk only."""
    b, f, seed = next(c for c in ec.CASES[key] if c[0] == 3)
    z = _fixture(key)[ec.case_name(b, f)]
    full = _run(key, seed, fmt, z["mel"]).clone()
    assert torch.isfinite(full).all()
    for i in range(b):
        one = _run(key, seed, fmt, z["mel"][i:i + 1]).clone()
        assert torch.equal(full[i:i + 1], one), (key, fmt, i, _linf(full[i:i + 1].cpu().numpy(), one.cpu().numpy()))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_hifigan_edge_wide_block_shapes_on_r80(fmt):
    """r80 at B = 256 x 256 frames: conv_pre (80 rows, 128-column tiles) starts 1 x 2 x 256 = 512 workgroups and stays narrow while
    ups.0 (2 x 2 x 256 = 1024), ups.1 (1 x 10 x 256) and the 40-channel resblock convs (1 x 5 x 256 = 1280) take the wide shape;
    a single item is narrow throughout.  Items 0 and B - 1 equal their single-item calls bit for bit, and the single-item call is
    inside the format's bound against its restatement.  The case has no fixture of its own, so every bound is scaled from the
    largest figure over the config's fixtures: fp32 (the float64 restatement) EDGE_LINF_FACTOR x and bf16x3 BF16X3_LINF_FACTOR x the
    base, the largest ``ref_fp32_vs_fp64`` L-inf; f16 F16_RMS_FACTOR / F16_LINF_FACTOR x the largest ``ref_half_vs_fp32`` relative
    RMS / L-inf."""
    key, B, T = "r80", 256, 256
    cfg = ec.CONFIGS[key]
    layers = {l.name: l for l in ec.plan(cfg, 2 if fmt == "f16" else 4)}
    narrow = {n: ec.launch_shape(l, ec.columns(cfg, l, T), B)[2] < l.BN for n, l in layers.items()}
    assert narrow["conv_pre"] and ec.launch_shape(layers["conv_pre"], T, B)[3] == 512
    wide = ["ups.0", "ups.1"] + [n for n, l in layers.items() if l.M == 40]
    assert len(wide) == 8 and not any(narrow[n] for n in wide)
    assert ec.launch_shape(layers["ups.0"], T, B)[3] == ec.HG_NARROW_BELOW
    for n, l in layers.items():
        assert ec.launch_shape(l, ec.columns(cfg, l, T), 1)[2] == (l.BN // 2 if l.BM >= 64 else l.BN), n
    seed = ec.CASES[key][0][2]
    mel = synthetic.synthetic_mel(B, T, cfg["num_mels"], seed=256)
    full = _run(key, seed, fmt, mel)
    assert torch.isfinite(full).all()
    for i in (0, B - 1):
        one = _run(key, seed, fmt, mel[i:i + 1])
        assert torch.equal(full[i:i + 1], one), i
    one = _run(key, seed, fmt, mel[:1]).cpu().numpy()
    base = _base_linf(key)
    sd = _sd(key, seed)
    half_rel, half_linf = (max(float(z["ref_half_vs_fp32"][i]) for z in _fixture(key).values()) for i in (0, 1))
    if fmt == "f32":
        want, b_rms, b_linf = hr.generator_np(cfg, sd, mel[:1]), WAVE_TOL, EDGE_LINF_FACTOR * base
    elif fmt == "f16":
        want = h16.generator_np(cfg, sd, mel[:1])
        b_rms, b_linf = F16_RMS_FACTOR * half_rel, F16_LINF_FACTOR * half_linf
    else:
        want, b_rms, b_linf = h3.generator_np(cfg, sd, mel[:1]), WAVE_TOL, BF16X3_LINF_FACTOR * base
    err, linf = rms_rel_err(one, want), _linf(one, want)
    _log({"format": fmt, "config": key, "case": f"wide b{B}_f{T}, item 0 alone vs restatement", "rel_rms": err, "linf": linf,
          "linf_over_base": linf / base, "bound_rel_rms": b_rms, "bound_linf": b_linf})
    assert err < b_rms and linf < b_linf


# ---- the C ABI directly: own buffers, strided unaligned mel, poisoned workspace, guard zones ----
def _abi_setup(key, fmt, seed):
    """(config struct, packed blob on the device) through the pack and size queries of hifigan._ENTRY."""
    lib = _lib.lib()
    cfg = ec.CONFIGS[key]
    c = hg.c_config(cfg)
    packed_bytes, pack, _, _ = hg._ENTRY[fmt]
    # folded on the device, as Generator._pack folds them: the CPU's norm may round another way and the packed bits would move
    flat = torch.cat([t.reshape(-1) for wb in _model(key, seed).folded_weights() for t in wb]).contiguous()
    assert flat.is_cuda
    assert flat.numel() == lib.ctts_hifigan_weight_floats(ctypes.byref(c))
    blob = torch.zeros(_lib.nbytes(getattr(lib, packed_bytes), ctypes.byref(c), what=packed_bytes) // 4, dtype=torch.float32, device="cuda:0")
    _lib.check(getattr(lib, pack)(ctypes.byref(c), _lib.ptr(flat), flat.numel(), _lib.ptr(blob), _lib.stream(torch.device("cuda:0"))), pack)
    torch.cuda.synchronize()
    return c, blob


def _abi_forward(fmt, c, blob, mel, strided, ws_byte):
    """One forward through the C entry on buffers of this test's own.  ``mel``: numpy [B, num_mels, T].  ``strided``: rows
    ``T + 3`` apart behind a pointer one float off a 16-byte boundary, NaN everywhere between the rows; else the contiguous mel
    padded to a multiple of four columns that ``Generator.forward`` hands over.  The workspace has exactly the queried size
    and is filled with ``ws_byte``; 256 sentinel bytes follow it, and 256 lie on either side of the waveform.  Returns the
    waveform [B, 1, L] after asserting that every sentinel byte is intact."""
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    B, n_mel, T = mel.shape
    up = 1
    for i in range(c.n_ups):
        up *= c.upsample_rates[i]
    L = T * up
    x = torch.from_numpy(np.ascontiguousarray(mel)).to(dev)
    if strided:
        ld = T + 3
        buf = torch.full((4 + 1 + B * n_mel * ld,), float("nan"), dtype=torch.float32, device=dev)
        buf[5:].view(B, n_mel, ld)[:, :, :T] = x
        mel_ptr = buf.data_ptr() + 20
        assert buf.data_ptr() % 16 == 0 and mel_ptr % 16 == 4
    else:
        ld = (T + 3) // 4 * 4
        buf = torch.nn.functional.pad(x, (0, ld - T)).contiguous()
        mel_ptr = buf.data_ptr()
        assert mel_ptr % 16 == 0
    _, _, ws_query, fwd = hg._ENTRY[fmt]
    ws_bytes = _lib.nbytes(getattr(lib, ws_query), ctypes.byref(c), B, T, what=ws_query)
    ws = torch.full((ws_bytes + 256,), SENTINEL, dtype=torch.uint8, device=dev)
    ws[:ws_bytes] = ws_byte
    audio = torch.full((256 + B * L * 4 + 256,), SENTINEL, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 16 == 0 and audio.data_ptr() % 16 == 0
    _lib.check(getattr(lib, fwd)(ctypes.byref(c), _lib.ptr(blob), ctypes.c_void_p(mel_ptr), ld, ctypes.c_void_p(audio.data_ptr() + 256),
                                 B, T, _lib.ptr(ws), ws_bytes, _lib.stream(dev)), fwd)
    torch.cuda.synchronize()
    assert bool((ws[ws_bytes:] == SENTINEL).all()), "a store went past workspace_bytes"
    assert bool((audio[:256] == SENTINEL).all()), "a store went in front of the waveform"
    assert bool((audio[256 + B * L * 4:] == SENTINEL).all()), "a store went past the waveform"
    return audio[256:256 + B * L * 4].view(torch.float32).view(B, 1, L).clone()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("key,frames", [("r24", 43), ("r80", 65)])
def test_hifigan_edge_c_abi_strided_mel_poisoned_workspace_and_guards(key, frames, fmt):
    """ctts_hifigan_forward_f32 / _f16 / _bf16x3 on an odd frame count.  The call on the padded aligned mel with a zeroed
    workspace is what ``Generator.forward`` returns, bit for bit; so are the call with ``mel_ld = frames + 3`` behind an
    unaligned pointer with NaN in every float that is not a mel value (fp32: the scalar staging branch of hg_conv_kernel), and
    the call on a workspace of all-ones bytes (NaN in fp32 and in half): no pad column, pad channel or stale buffer is read
    into a result.  No store leaves the waveform or the workspace (asserted inside ``_abi_forward``)."""
    seed = ec.CASES[key][0][2]
    mel = synthetic.synthetic_mel(2, frames, ec.CONFIGS[key]["num_mels"], seed=900 + frames)
    assert frames % 2 == 1
    c, blob = _abi_setup(key, fmt, seed)
    base = _abi_forward(fmt, c, blob, mel, strided=False, ws_byte=0)
    assert torch.isfinite(base).all()
    assert torch.equal(base, _run(key, seed, fmt, mel)), "the C entry and Generator.forward differ"
    strided = _abi_forward(fmt, c, blob, mel, strided=True, ws_byte=0)
    assert torch.equal(strided, base), _linf(strided.cpu().numpy(), base.cpu().numpy())
    poisoned = _abi_forward(fmt, c, blob, mel, strided=False, ws_byte=0xFF)
    assert torch.equal(poisoned, base), _linf(poisoned.cpu().numpy(), base.cpu().numpy())
    both = _abi_forward(fmt, c, blob, mel, strided=True, ws_byte=0xFF)
    assert torch.equal(both, base), _linf(both.cpu().numpy(), base.cpu().numpy())
