"""CPU: AMT-G's large frames behind config.yaml's ``amt_large_frames`` key — the new C symbols (header, both libraries, the binding) and their
null-handle answers, the key read at call time, the size check and its messages for S, L and G with the key on and off (2160x3840 for G is
refused when off and accepted when on; 2832x4320 is refused either way), the node's refusal before a checkpoint or an engine exists, and the
Python limits against the library's, and the stand-alone address check of the residual + PReLU large form
(tests/hostcheck/conv_large_res_prelu_addr.cpp, built with the undefined-behaviour sanitizer and run as a program).  ``ckpt.load_config`` is patched to turn keys on: the package's config.yaml leaves them off."""
import ctypes
import os
import subprocess

import pytest
import torch

import cfi_amd
from cfi_amd import _lib, amt, ckpt

NEW = ["vfi_amt_set_large_frames", "vfi_amt_large_max_padded_pixels", "vfi_amt_object_max_padded_pixels", "vfi_conv_allow_large_res_prelu"]
G_OFF, G_ON, SL = 6100805, 12201611, 2 ** 23 - 1


_REAL_CONFIG = ckpt.load_config      # the package's own config.yaml, whatever a test has patched in since


def config_with(**keys):
    def load():
        cfg = dict(_REAL_CONFIG())
        cfg.update(keys)
        return cfg
    return load


def _no_engine(*a, **k):
    raise AssertionError("the refusals must come before the checkpoint and the engine")


def test_new_symbols_header_libraries_binding(hip_lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "vfi_hip.h")) as fh:
        header = fh.read()
    product, test = ctypes.CDLL(_lib.LIB_PATH), ctypes.CDLL(_lib.TEST_LIB_PATH)
    for n in NEW:
        assert n + "(" in header and n in _lib.PROTOTYPES and getattr(hip_lib, n) is not None
        assert getattr(product, n) is not None and getattr(test, n) is not None
    assert _lib.PROTOTYPES["vfi_amt_set_large_frames"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    assert _lib.PROTOTYPES["vfi_amt_large_max_padded_pixels"] == (ctypes.c_int64, [ctypes.c_int])
    assert _lib.PROTOTYPES["vfi_amt_object_max_padded_pixels"] == (ctypes.c_int64, [ctypes.c_void_p])
    assert _lib.PROTOTYPES["vfi_conv_allow_large_res_prelu"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])


def test_the_amt_test_taps_are_in_the_test_build_only(hip_lib):
    """include/vfi_hip_test_amt.h: bound in the test build, absent from the product library (dlopen only, no call)"""
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "vfi_hip_test_amt.h")) as fh:
        declared = set(re.findall(r"\b(vfi_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)))
    assert declared == set(_lib.AMT_TEST_PROTOTYPES) == {"vfi_test_amt_add", "vfi_test_amt_warp"}
    product = ctypes.CDLL(_lib.LIB_PATH)
    for n in declared:
        assert getattr(hip_lib, n) is not None and not hasattr(product, n), n
    assert hip_lib.vfi_test_amt_add(None, 4, 4, 1, None, 0, None, 4, 2, 2, 4, 1, None) != 0 and "vfi_test_amt_add: bad arguments" in _lib.last_error()
    assert hip_lib.vfi_test_amt_warp(None, 4, None, 2, None, 4, 2, 2, 4, None) != 0 and "vfi_test_amt_warp: bad arguments" in _lib.last_error()


def test_null_handles(hip_lib):
    assert hip_lib.vfi_amt_set_large_frames(None, 1) != 0 and "vfi_amt_set_large_frames: null object" in _lib.last_error()
    assert hip_lib.vfi_amt_object_max_padded_pixels(None) == 0
    assert hip_lib.vfi_amt_large_max_padded_pixels(3) == 0 and hip_lib.vfi_amt_large_max_padded_pixels(-1) == 0
    assert hip_lib.vfi_conv_allow_large_res_prelu(None, 1) != 0 and "vfi_conv_allow_large_res_prelu: null handle" in _lib.last_error()


def test_the_python_limits_are_the_librarys(hip_lib):
    assert amt.LARGE_MAX_PADDED_PIXELS_G == (2 ** 32 - 1) // 352 == G_ON == hip_lib.vfi_amt_large_max_padded_pixels(2)
    assert amt.MAX_PADDED_PIXELS_G == (2 ** 31 - 1) // 352 == G_OFF      # the limit with the key off is what it was
    # AMT-S / AMT-L: the switch has nothing to raise
    assert amt.MAX_PADDED_PIXELS == SL == hip_lib.vfi_amt_large_max_padded_pixels(0) == hip_lib.vfi_amt_large_max_padded_pixels(1)


def test_key_absent_false_true_read_at_call_time(monkeypatch):
    assert "amt_large_frames" not in ckpt.load_config()                  # the package's own config.yaml: absent = off
    assert not amt.large_frames_enabled() and amt.max_padded_pixels("G") == G_OFF
    monkeypatch.setattr(ckpt, "load_config", config_with(amt_large_frames=False))
    assert not amt.large_frames_enabled() and amt.max_padded_pixels("G") == G_OFF
    monkeypatch.setattr(ckpt, "load_config", config_with(amt_large_frames=True))      # no reload, no new import: the next call sees it
    assert amt.large_frames_enabled() and amt.max_padded_pixels("G") == G_ON
    assert amt.max_padded_pixels("S") == amt.max_padded_pixels("L") == amt.max_padded_pixels(None) == SL
    monkeypatch.setattr(ckpt, "load_config", config_with(amt_large_frames=False))
    assert amt.max_padded_pixels("G") == G_OFF


def test_no_environment_variable_turns_it_on(monkeypatch):
    for name in ("AMT_LARGE_FRAMES", "VFI_AMT_LARGE_FRAMES", "amt_large_frames"):
        monkeypatch.setenv(name, "1")
    assert not amt.large_frames_enabled()


def test_check_frame_size_for_g(monkeypatch):
    assert amt.padded_size(2160, 3840) == (2160, 3840) and G_OFF < 2160 * 3840 == 8294400 <= G_ON
    assert amt.padded_size(2832, 4320) == (2832, 4320) and 2816 * 4320 == 12165120 <= G_ON < 2832 * 4320
    # key off: 4K is refused, and the message names the key that would help
    with pytest.raises(ValueError, match=r"AMT VFI: 2160x3840 frames \(padded 2160x3840\) are beyond the kernels' index arithmetic \(6100805 pixels for AMT-G\); "
                                         r"config.yaml's amt_large_frames: true raises it to 12201611"):
        amt.check_frame_size(2160, 3840, "G")
    # ... beyond the large limit it says that the key would not be enough
    with pytest.raises(ValueError, match=r"2832x4320.*\(6100805 pixels for AMT-G\) \(amt_large_frames would raise it to 12201611 only\)"):
        amt.check_frame_size(2832, 4320, "G")
    monkeypatch.setattr(ckpt, "load_config", config_with(amt_large_frames=True))
    amt.check_frame_size(2160, 3840, "G")
    amt.check_frame_size(2816, 4320, "G")
    amt.check_frame_size(1080, 1920, "G")
    with pytest.raises(ValueError, match=r"2832x4320.*index arithmetic \(12201611 pixels for AMT-G\) \(decoder1's 352-channel buffers"):
        amt.check_frame_size(2832, 4320, "G")
    # the caller's own reading of the key wins over the file's
    with pytest.raises(ValueError, match="amt_large_frames: true raises it"):
        amt.check_frame_size(2160, 3840, "G", large=False)
    with pytest.raises(ValueError, match="at least 128"):
        amt.check_frame_size(100, 300, "G")


@pytest.mark.parametrize("variant", ["S", "L", None])
@pytest.mark.parametrize("key", [False, True])
def test_check_frame_size_for_s_and_l_does_not_follow_the_key(monkeypatch, variant, key):
    monkeypatch.setattr(ckpt, "load_config", config_with(amt_large_frames=key))
    amt.check_frame_size(2160, 3840, variant)
    amt.check_frame_size(2048, 4080, variant)      # 8 355 840 <= 2^23 - 1
    assert 2048 * 4096 == SL + 1
    with pytest.raises(ValueError, match=r"padded 2048x4096\) are beyond the kernels' index arithmetic \(8388607 pixels\)$"):
        amt.check_frame_size(2048, 4096, variant)
    with pytest.raises(ValueError, match=r"\(8388607 pixels\)$"):
        amt.check_frame_size(2832, 4320, variant)


def test_the_node_refuses_before_any_engine_is_built(monkeypatch):
    monkeypatch.setattr(amt, "load_file_from_direct_url", _no_engine)
    monkeypatch.setattr(amt, "cached_engine", _no_engine)
    clip_4k = torch.zeros(1, 1, 1, 3).expand(2, 2160, 3840, 3)
    too_big = torch.zeros(1, 1, 1, 3).expand(2, 2832, 4320, 3)
    node = cfi_amd.amt.AMT_VFI()
    # amt_large_frames without amt_g changes nothing: the checkpoint is refused by name
    monkeypatch.setattr(ckpt, "load_config", config_with(amt_large_frames=True))
    with pytest.raises(NotImplementedError, match="amt-g.pth: AMT-G has a forward of its own"):
        node.vfi("amt-g.pth", clip_4k)
    # amt_g alone: 4K is refused before the checkpoint lookup, and the message names the key
    monkeypatch.setattr(ckpt, "load_config", config_with(amt_g=True))
    with pytest.raises(ValueError, match=r"for AMT-G\); config.yaml's amt_large_frames: true"):
        node.vfi("amt-g.pth", clip_4k)
    # both keys: 4K passes the size check (the next thing the node does is ask for the checkpoint), 2832x4320 does not
    monkeypatch.setattr(ckpt, "load_config", config_with(amt_g=True, amt_large_frames=True))
    with pytest.raises(AssertionError, match="before the checkpoint and the engine"):
        node.vfi("amt-g.pth", clip_4k)
    with pytest.raises(ValueError, match=r"2832x4320.*12201611 pixels for AMT-G"):
        node.vfi("amt-g.pth", too_big)
    # AMT-S / AMT-L take 4K with or without the key, as before
    for name in ("amt-s.pth", "amt-l.pth"):
        with pytest.raises(AssertionError, match="before the checkpoint and the engine"):
            node.vfi(name, clip_4k)
        with pytest.raises(ValueError, match=r"\(8388607 pixels\)$"):
            node.vfi(name, too_big)


def test_the_key_is_documented_in_the_config_file():
    path = os.path.join(os.path.dirname(os.path.abspath(amt.__file__)), "config.yaml")
    with open(path) as fh:
        text = fh.read()
    line = [ln for ln in text.splitlines() if ln.startswith("# amt_large_frames: true")]
    assert len(line) == 1 and "12 201 611" in line[0] and "6 100 805" in line[0] and "AMT-S and AMT-L" in line[0]


def test_res_prelu_address_check_program_under_ubsan(tmp_path):
    """The three per-region descriptors (input, output, residual) of both Winograd region shapes and the direct tiles' input descriptor on
    AMT-G's rb[4] at 1080x1920, at 1408x2160 and with a wider residual at an odd size (csrc/conv_large.h)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "conv_large_res_prelu_addr")
    src = os.path.join(root, "tests", "hostcheck", "conv_large_res_prelu_addr.cpp")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Xarch_host", "-fsanitize=undefined,signed-integer-overflow",
                           "-Xarch_host", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "conv_large_res_prelu_addr: ok" in r.stdout and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
