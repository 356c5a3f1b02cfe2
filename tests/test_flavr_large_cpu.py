"""CPU: FLAVR's large frames behind config.yaml's ``flavr_large_frames`` key — the new C symbols (header, both libraries, the binding) and
their null-handle answers, the key's three states read at call time, the limit arithmetic, the node's refusal before a checkpoint or an
engine exists, the key left unread for frames under the old limit, and the stand-alone address check of the transposed convolution's large
form (tests/hostcheck/deconv_large_addr.cpp, built with the undefined-behaviour sanitizer and run as a program).  ``ckpt.load_config`` is
patched to turn the key on: the package's config.yaml leaves it off."""
import contextlib
import ctypes
import os
import subprocess

import pytest
import torch

import cfi_amd
from cfi_amd import _lib, ckpt, flavr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vfi_flavr_set_large_frames", "vfi_flavr_max_padded_pixels", "vfi_flavr_large_max_padded_pixels", "vfi_flavr_object_max_padded_pixels"]
OLD, LARGE = 2097151, 8388607


def config_with(**keys):
    real = ckpt.load_config

    def load():
        cfg = dict(real())
        cfg.update(keys)
        return cfg
    return load


def _nothing_may_load(*a, **k):
    raise AssertionError("the refusal must come before the checkpoint, the engine and any upload")


def test_new_symbols_header_libraries_binding(hip_lib):
    with open(os.path.join(ROOT, "include", "vfi_hip.h")) as fh:
        header = fh.read()
    product, test = ctypes.CDLL(_lib.LIB_PATH), ctypes.CDLL(_lib.TEST_LIB_PATH)
    for n in NEW:
        assert n + "(" in header and n in _lib.PROTOTYPES and getattr(hip_lib, n) is not None
        assert getattr(product, n) is not None and getattr(test, n) is not None


def test_null_handles(hip_lib):
    assert hip_lib.vfi_flavr_set_large_frames(None, 1) != 0 and "vfi_flavr_set_large_frames: null object" in _lib.last_error()
    assert hip_lib.vfi_flavr_object_max_padded_pixels(None) == 0


def test_limit_arithmetic(hip_lib):
    """The widest tensor, the last up-convolution's [Hp, Wp, 4 * 64], sets both limits: below 2^31 - 1 bytes, and within the layer kernels' bound
    for one operand image with the permission"""
    assert flavr.FLOATS_PER_PADDED_PIXEL == 4 * 64
    assert flavr.MAX_PADDED_PIXELS == OLD == hip_lib.vfi_flavr_max_padded_pixels()
    assert OLD * 1024 < 2 ** 31 - 1 <= (OLD + 1) * 1024
    bound = hip_lib.vfi_conv_huge_max_floats()
    assert bound == 2 ** 31 - 1
    assert flavr.LARGE_MAX_PADDED_PIXELS == bound // 256 == LARGE == hip_lib.vfi_flavr_large_max_padded_pixels()
    pad = flavr.padded_size
    assert pad(1080, 1920) == (1088, 1920) and 1088 * 1920 <= OLD < 1104 * 1920      # 1080p fits the old limit, 1104x1920 is the first refused
    assert pad(1440, 2560) == (1440, 2560) and OLD < 1440 * 2560 <= LARGE
    assert pad(2160, 3840) == (2160, 3840) and 2160 * 3840 == 8294400 <= LARGE < 2176 * 3856
    assert pad(2161, 3841) == (2176, 3856)


def test_key_absent_false_true_read_at_call_time(monkeypatch):
    assert "flavr_large_frames" not in ckpt.load_config()                  # the package's own config.yaml: absent = off
    assert not flavr.large_frames_enabled() and flavr.max_padded_pixels() == OLD
    monkeypatch.setattr(ckpt, "load_config", config_with(flavr_large_frames=False))
    assert not flavr.large_frames_enabled() and flavr.max_padded_pixels() == OLD
    monkeypatch.setattr(ckpt, "load_config", config_with(flavr_large_frames=True))      # no reload, no new import: the next call sees it
    assert flavr.large_frames_enabled() and flavr.max_padded_pixels() == LARGE
    monkeypatch.setattr(ckpt, "load_config", config_with(flavr_large_frames=False))
    assert flavr.max_padded_pixels() == OLD


def test_no_environment_variable_turns_it_on(monkeypatch):
    for name in ("FLAVR_LARGE_FRAMES", "VFI_FLAVR_LARGE_FRAMES", "flavr_large_frames"):
        monkeypatch.setenv(name, "1")
    assert not flavr.large_frames_enabled()


def test_check_frame_size(monkeypatch):
    flavr.check_frame_size(1080, 1920)
    with pytest.raises(ValueError, match=r"FLAVR VFI: 1104x1920 frames \(padded 1104x1920\) are over the size limit of 2097151 padded pixels; "
                                         r"config.yaml's flavr_large_frames: true raises it to 8388607"):
        flavr.check_frame_size(1104, 1920)                                 # the key would have helped: it is named
    with pytest.raises(ValueError, match=r"2161x3841 frames \(padded 2176x3856\) are over the size limit of 2097151") as e:
        flavr.check_frame_size(2161, 3841)                                 # ... here it would not
    assert "true raises it" not in str(e.value)
    monkeypatch.setattr(ckpt, "load_config", config_with(flavr_large_frames=True))
    flavr.check_frame_size(1104, 1920)
    flavr.check_frame_size(2160, 3840)
    with pytest.raises(ValueError, match=r"padded 2176x3856\) are over the size limit of 8388607 padded pixels"):
        flavr.check_frame_size(2176, 3856)


def test_the_key_is_not_read_for_frames_under_the_old_limit(monkeypatch):
    monkeypatch.setattr(ckpt, "load_config", lambda: (_ for _ in ()).throw(AssertionError("config.yaml was read for a small frame")))
    flavr.check_frame_size(1080, 1920)
    flavr.check_frame_size(1088, 1920)
    with pytest.raises(AssertionError, match="was read"):
        flavr.check_frame_size(1104, 1920)


class StandIn:
    """An engine that records what the node asks of it"""

    device = torch.device("cpu")

    def __init__(self):
        self.windows = 0

    def forward(self, frames, out=None):
        self.windows += 1
        return ((frames[1] + frames[2]) / 2)[None, ..., :3]


def test_the_node_refuses_before_any_upload(monkeypatch):
    monkeypatch.setattr(flavr, "load_file_from_github_release", _nothing_may_load)
    monkeypatch.setattr(flavr, "cached_engine", _nothing_may_load)
    monkeypatch.setattr(flavr, "run_windows", _nothing_may_load)
    over_old = torch.zeros(1, 1, 1, 3).expand(4, 1104, 1920, 3)      # no memory behind it: the check reads the shape only
    over_large = torch.zeros(1, 1, 1, 3).expand(4, 2176, 3856, 3)
    with pytest.raises(ValueError, match="flavr_large_frames: true raises it to 8388607"):
        cfi_amd.flavr.FLAVR_VFI().vfi("FLAVR_2x.pth", over_old)
    monkeypatch.setattr(ckpt, "load_config", config_with(flavr_large_frames=True))
    with pytest.raises(ValueError, match=r"2176x3856.*size limit of 8388607"):
        cfi_amd.flavr.FLAVR_VFI().vfi("FLAVR_2x.pth", over_large)
    # with the key on the frame passes the check: the next thing the node does is ask for the checkpoint
    with pytest.raises(AssertionError, match="before the checkpoint"):
        cfi_amd.flavr.FLAVR_VFI().vfi("FLAVR_2x.pth", over_old)


def test_the_stand_in_engine_runs_a_clip_through_the_node(monkeypatch):
    eng = StandIn()
    monkeypatch.setattr(flavr, "load_file_from_github_release", lambda *a: "FLAVR_2x.pth")
    monkeypatch.setattr(flavr, "cached_engine", lambda kind, path, build: (eng, False))
    monkeypatch.setattr(flavr, "engine_call", lambda entry, shape: contextlib.nullcontext(entry[0]))
    monkeypatch.setattr(ckpt, "load_config", lambda: (_ for _ in ()).throw(AssertionError("config.yaml was read for a small frame")))
    frames = torch.rand(5, 32, 48, 3)
    (out,) = cfi_amd.flavr.FLAVR_VFI().vfi("FLAVR_2x.pth", frames)
    assert out.shape == (7, 32, 48, 3) and eng.windows == 2


def test_the_key_is_documented_in_the_config_file():
    with open(os.path.join(os.path.dirname(os.path.abspath(flavr.__file__)), "config.yaml")) as fh:
        text = fh.read()
    assert "# flavr_large_frames: true" in text and "8 388 607" in text and "2 097 151" in text


def test_deconv_address_check_program_under_ubsan(tmp_path):
    """The store-side helpers of csrc/conv_large.h (large_deconv_*) and the input rebase for every region of FLAVR's two transposed layers at
    2160x3840, at the large limit and on two small images"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "deconv_large_addr")
    src = os.path.join(ROOT, "tests", "hostcheck", "deconv_large_addr.cpp")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Xarch_host", "-fsanitize=undefined,signed-integer-overflow",
                           "-Xarch_host", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "deconv_large_addr: ok" in r.stdout and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
