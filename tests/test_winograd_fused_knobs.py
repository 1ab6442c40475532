"""The knobs of the one-launch Winograd layer: names, bits and the library's view of them (no GPU needed)."""
import os

from conftest import REPO
from cookietts_amd import _lib

NEW = ("CTTS_F32_WINOGRAD_FUSED_MIN", "CTTS_F32_WINOGRAD_NO_FUSED")


def test_new_knobs_have_bits_of_their_own_and_are_documented():
    bits = _lib.TUNING_BITS
    assert all(n in bits for n in NEW)
    assert len(set(bits.values())) == len(bits) and all(0 <= b <= 30 for b in bits.values())
    hdr = open(os.path.join(REPO, "include", "cookietts_hip.h")).read()
    tun = open(os.path.join(REPO, "cookietts_amd", "csrc", "tuning.h")).read()
    for n in NEW:
        assert f"{bits[n]} {n}" in hdr and n in tun, n


def test_library_reads_the_new_knobs(hip_lib_path, monkeypatch):
    for n in NEW + ("CTTS_F32_WINOGRAD_MIN", "CTTS_F32_WINOGRAD_PLAIN"):
        monkeypatch.delenv(n, raising=False)
    _lib.tuning_reload()
    try:
        assert not any(_lib.tuning_active(n) for n in NEW)
        monkeypatch.setenv("CTTS_F32_WINOGRAD_FUSED_MIN", "0")          # 0 = always: set, not "off"
        _lib.tuning_reload()
        assert _lib.tuning_active("CTTS_F32_WINOGRAD_FUSED_MIN") and not _lib.tuning_active("CTTS_F32_WINOGRAD_NO_FUSED")
        assert not _lib.tuning_active("CTTS_F32_WINOGRAD_MIN")          # the form's own threshold is another knob
        monkeypatch.setenv("CTTS_F32_WINOGRAD_NO_FUSED", "1")
        _lib.tuning_reload()
        assert all(_lib.tuning_active(n) for n in NEW)
    finally:
        monkeypatch.undo()
        _lib.tuning_reload()
