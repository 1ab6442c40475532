"""Host side of the composed conditioning (no GPU): which configs have it, what it adds to the blob and takes from the workspace,
and that the entry points without `options` size exactly what they sized before."""
import ctypes as C
import os

from conftest import REPO
from cookietts_amd import WaveGlow, _lib, synthetic

NEW_SYMBOLS = ("ctts_waveglow_has_composed_cond", "ctts_waveglow_packed_bytes_opt", "ctts_waveglow_pack_cond_composed",
               "ctts_waveglow_workspace_bytes_opt", "ctts_waveglow_infer_spk_f32_opt", "ctts_wn_cond_composed_scratch_bytes",
               "ctts_wn_cond_composed_f32")


def _model(name):
    return WaveGlow(**synthetic.WAVEGLOW_CONFIGS[name])


def test_symbols_header_and_knob(hip_lib_path):
    lib = _lib.lib()
    hdr = open(os.path.join(REPO, "include", "cookietts_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s + "(" in hdr and s in _lib.SIGNATURES, s
    assert "#define CTTS_WG_OPT_COMPOSED_COND 1" in hdr and _lib.WG_OPT_COMPOSED_COND == 1
    assert "CTTS_F32_COND_CHAIN" in open(os.path.join(REPO, "cookietts_amd", "csrc", "tuning.h")).read() and "CTTS_F32_COND_CHAIN" in hdr


def test_which_models_ask_for_it(hip_lib_path):
    lib = _lib.lib()
    for name, has, asks in (("toy", 1, 1), ("full", 1, 1), ("toy_hop512_g16", 1, 1), ("toy_hop384_g12", 1, 1),
                            ("toy_simple", 1, 0), ("toy_simple_half", 1, 0),          # the shape allows it, the class never asks
                            ("toy_spk_rezero", 0, 0)):
        m = _model(name)
        c = m.c_config()
        assert lib.ctts_waveglow_has_composed_cond(C.byref(c)) == has, name
        assert m._options() == asks, name
    m = _model("toy")
    m._composed_cond = False
    assert m._options() == 0
    assert _model("toy").set_compute_dtype("bf16x3")._options() == 0                    # the 16-bit paths have their own cond GEMMs


def test_blob_and_workspace_sizes(hip_lib_path):
    lib = _lib.lib()
    c = _model("full").c_config()
    assert lib.ctts_waveglow_packed_bytes_opt(C.byref(c), 0) == lib.ctts_waveglow_packed_bytes(C.byref(c))
    grown = lib.ctts_waveglow_packed_bytes_opt(C.byref(c), 1) - lib.ctts_waveglow_packed_bytes(C.byref(c))
    n_flows, P, J, n_mel, K0 = 12, 32, 4, 80, 640
    # A [n_flows P][J n_mel][256] + bias [n_flows P][256] + the pack-time double scratch [n_flows][256][K0]
    assert grown == 4 * (n_flows * P * 256 * (J * n_mel + 1) + n_flows * 2 * 256 * K0)
    assert lib.ctts_waveglow_packed_bytes_opt(C.byref(c), 2) == 0 and b"options" in lib.ctts_last_error()
    for fn, fn_opt in ((lib.ctts_waveglow_workspace_bytes, lib.ctts_waveglow_workspace_bytes_opt),):
        chain = fn(C.byref(c), 8, 900)
        assert fn_opt(C.byref(c), 8, 900, 0) == chain
        # 900 frames: no spect [B][640][ld] and no h_tmp [B][12 * 256][ld], a padded mel [B][80][1032] instead
        ld = 28928 + 2 * 128                    # L = 900 * 32 = 28800 rounded up to a multiple of 256; pad 128 (8 layers)
        assert chain - fn_opt(C.byref(c), 8, 900, 1) == 4 * 8 * ((640 + 12 * 256) * ld - 80 * (8 * 128 + 8))
        # 9 frames fill a fraction of the GEMM's 128-frame tile: the chain issues fewer products, and keeps its buffers
        assert fn_opt(C.byref(c), 8, 9, 1) == fn(C.byref(c), 8, 9)
        assert fn_opt(C.byref(c), 8, 44, 1) == fn(C.byref(c), 8, 44) and fn_opt(C.byref(c), 8, 45, 1) < fn(C.byref(c), 8, 45)
    spk = _model("toy_spk_rezero").c_config()
    assert lib.ctts_waveglow_packed_bytes_opt(C.byref(spk), 1) == lib.ctts_waveglow_packed_bytes(C.byref(spk))
    assert lib.ctts_wn_cond_composed_scratch_bytes(C.byref(spk), 2, 9) == 0
    assert lib.ctts_wn_cond_composed_scratch_bytes(C.byref(c), 8, 900) == 4 * 8 * 80 * (8 * 128 + 8)
