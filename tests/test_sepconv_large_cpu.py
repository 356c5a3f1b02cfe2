"""CPU: Sepconv VFI's large frames behind config.yaml's ``sepconv_large_frames`` key — the new C symbols (header, both libraries, the
binding) and their null-handle answers, the key's states read at call time, the limit arithmetic, ``check_frame_size`` for every row of the
table in docs/design/sepconv.md "4K", the node's refusal before a checkpoint or an engine exists, the key left unread for frames the old
limit covers, and the stand-alone check of the band arithmetic (tests/hostcheck/sepconv_bands.cpp, built with the undefined-behaviour
sanitizer and run as a program).  ``ckpt.load_config`` is patched to turn the key on: the package's config.yaml leaves it off."""
import ctypes
import os
import subprocess

import pytest
import torch

import cfi_amd
from cfi_amd import _lib, ckpt, sepconv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vfi_sepconvnet_set_large_frames", "vfi_sepconvnet_max_pixels", "vfi_sepconvnet_large_max_pixels", "vfi_sepconvnet_object_max_pixels",
       "vfi_sepconv_pair_out_rows"]
WHOLE, OLD, LARGE = 2097151, 4194303, 8388607


def config_with(**keys):
    real = ckpt.load_config

    def load():
        cfg = dict(real())
        cfg.update(keys)
        return cfg
    return load


def _nothing_may_load(*a, **k):
    raise AssertionError("the refusal must come before the checkpoint, the engine and any upload")


def _config_must_not_be_read():
    raise AssertionError("config.yaml was read for a frame the old limit covers")


def test_new_symbols_header_libraries_binding(hip_lib):
    with open(os.path.join(ROOT, "include", "vfi_hip.h")) as fh:
        header = fh.read()
    product, test = ctypes.CDLL(_lib.LIB_PATH), ctypes.CDLL(_lib.TEST_LIB_PATH)
    for n in NEW:
        assert n + "(" in header and n in _lib.PROTOTYPES and getattr(hip_lib, n) is not None
        assert getattr(product, n) is not None and getattr(test, n) is not None


def test_null_handles(hip_lib):
    assert hip_lib.vfi_sepconvnet_set_large_frames(None, 1) != 0 and "vfi_sepconvnet_set_large_frames: null object" in _lib.last_error()
    assert hip_lib.vfi_sepconvnet_object_max_pixels(None) == 0


def test_the_band_option_exists_in_the_test_library_only(hip_lib):
    assert hip_lib.vfi_test_set_option(b"sepconv_band_rows", 0) == 0
    assert not hasattr(ctypes.CDLL(_lib.LIB_PATH), "vfi_test_set_option")


def test_limit_arithmetic(hip_lib):
    """[Hp, Wp, 256], the heads' first layer, below 2 GiB (plain layer forms) and below 4 GiB (the old limit); [Hp, Wp, 64], up2(row1), below
    2 GiB with the key on"""
    assert sepconv.HEAD1_FLOATS_PER_PIXEL == 4 * 64 and sepconv.UP2_FLOATS_PER_PIXEL == 64
    assert sepconv.WHOLE_FRAME_PIXELS == WHOLE and WHOLE * 1024 < 2 ** 31 - 1 <= (WHOLE + 1) * 1024
    assert sepconv.MAX_PADDED_PIXELS == OLD == hip_lib.vfi_sepconvnet_max_pixels() and OLD * 1024 < 2 ** 32 <= (OLD + 1) * 1024
    assert sepconv.LARGE_MAX_PADDED_PIXELS == LARGE == hip_lib.vfi_sepconvnet_large_max_pixels() and LARGE * 256 < 2 ** 31 - 1 <= (LARGE + 1) * 256
    assert sepconv.BAND_MAX_WIDTH == 131071 and 16 * 131071 <= WHOLE < 16 * 131072
    pad = sepconv.padded_size
    assert pad(1080, 1920) == (1080, 1920) and 1080 * 1920 <= WHOLE
    assert pad(1440, 2560) == (1440, 2560) and WHOLE < 1440 * 2560 <= OLD
    assert pad(2160, 3840) == (2160, 3840) and OLD < 2160 * 3840 == 8294400 <= LARGE
    assert pad(2160, 3842) == (2160, 3842) and 2160 * 3842 == 8298720 <= LARGE
    assert pad(2898, 2896) == (2898, 2896) and 2898 * 2896 == 8392608 > LARGE
    assert pad(101, 179) == (102, 180) and pad(25, 40) == (26, 40)


def test_key_absent_false_true_read_at_call_time(monkeypatch):
    assert "sepconv_large_frames" not in ckpt.load_config()                  # the package's own config.yaml: absent = off
    assert not sepconv.large_frames_enabled() and sepconv.max_padded_pixels() == OLD
    monkeypatch.setattr(ckpt, "load_config", config_with(sepconv_large_frames=False))
    assert not sepconv.large_frames_enabled() and sepconv.max_padded_pixels() == OLD
    monkeypatch.setattr(ckpt, "load_config", config_with(sepconv_large_frames=True))      # no reload, no new import: the next call sees it
    assert sepconv.large_frames_enabled() and sepconv.max_padded_pixels() == LARGE
    monkeypatch.setattr(ckpt, "load_config", config_with(sepconv_large_frames=False))
    assert sepconv.max_padded_pixels() == OLD


def test_no_environment_variable_turns_it_on(monkeypatch):
    for name in ("SEPCONV_LARGE_FRAMES", "VFI_SEPCONV_LARGE_FRAMES", "sepconv_large_frames"):
        monkeypatch.setenv(name, "1")
    assert not sepconv.large_frames_enabled()


def test_check_frame_size_key_off(monkeypatch):
    """off, <= 4 194 303: today's path, no new refusal; off, above: ValueError naming the key"""
    for h, w in ((1080, 1920), (1440, 2560), (2, 2), (2048, 2046), (2047, 2045)):      # the last two pad to 2048 x 2046 = 4 190 208
        sepconv.check_frame_size(h, w)
    with pytest.raises(ValueError, match=r"Sepconv VFI: 2048x2048 frames \(padded 2048x2048\) are over the size limit of 4194303 padded pixels; "
                                         r"config.yaml's sepconv_large_frames: true raises it to 8388607"):
        sepconv.check_frame_size(2048, 2048)                                 # 4 194 304: the first refused, and the key would have helped
    with pytest.raises(ValueError, match=r"Sepconv VFI: 2160x3840 frames \(padded 2160x3840\) are over the size limit of 4194303 padded pixels; "
                                         r"config.yaml's sepconv_large_frames: true raises it to 8388607"):
        sepconv.check_frame_size(2160, 3840)
    with pytest.raises(ValueError, match=r"2897x2895 frames \(padded 2898x2896\) are over the size limit of 4194303") as e:
        sepconv.check_frame_size(2897, 2895)                                 # ... here it would not
    assert "true raises it" not in str(e.value) and "would raise it to 8388607 only" in str(e.value)


def test_check_frame_size_key_on(monkeypatch):
    """on: whole-frame up to 2 097 151, bands up to 8 388 607, refused above with the reason"""
    monkeypatch.setattr(ckpt, "load_config", config_with(sepconv_large_frames=True))
    for h, w in ((1080, 1920), (1440, 2560), (2048, 2048), (2160, 3840), (2160, 3842), (2159, 3841), (2896, 2896)):
        sepconv.check_frame_size(h, w)
    with pytest.raises(ValueError, match=r"Sepconv VFI: 2898x2896 frames \(padded 2898x2896\) are over the size limit of 8388607 padded pixels "
                                         r"\(up2\(row1\), the \[Hp, Wp, 64\] fp32 tensor, must stay below 2 GiB\)"):
        sepconv.check_frame_size(2898, 2896)                                 # 8 392 608
    with pytest.raises(ValueError, match=r"too wide for the banded head stage: 131071 padded columns"):
        sepconv.check_frame_size(32, 131073)


def test_the_key_is_not_read_for_frames_the_old_limit_covers(monkeypatch):
    monkeypatch.setattr(ckpt, "load_config", _config_must_not_be_read)
    for h, w in ((1080, 1920), (1440, 2560), (2048, 2046), (2045, 2048), (1, 1)):
        assert sepconv.padded_size(h, w)[0] * sepconv.padded_size(h, w)[1] <= OLD
        sepconv.check_frame_size(h, w)
    with pytest.raises(AssertionError, match="was read"):
        sepconv.check_frame_size(2048, 2048)


def test_the_node_refuses_before_any_upload(monkeypatch):
    monkeypatch.setattr(sepconv, "load_file_from_github_release", _nothing_may_load)
    monkeypatch.setattr(sepconv, "cached_engine", _nothing_may_load)
    monkeypatch.setattr(sepconv, "run_plan", _nothing_may_load)
    uhd = torch.zeros(1, 1, 1, 3).expand(2, 2160, 3840, 3)      # no memory behind it: the check reads the shape only
    over_large = torch.zeros(1, 1, 1, 3).expand(2, 2898, 2896, 3)
    with pytest.raises(ValueError, match="sepconv_large_frames: true raises it to 8388607"):
        cfi_amd.sepconv.SepconvVFI().vfi("sepconv.pth", uhd)
    monkeypatch.setattr(ckpt, "load_config", config_with(sepconv_large_frames=True))
    with pytest.raises(ValueError, match=r"2898x2896.*size limit of 8388607"):
        cfi_amd.sepconv.SepconvVFI().vfi("sepconv.pth", over_large)
    # with the key on the 4K frame passes the check: the next thing the node does is ask for the checkpoint
    with pytest.raises(AssertionError, match="before the checkpoint"):
        cfi_amd.sepconv.SepconvVFI().vfi("sepconv.pth", uhd)


def test_small_frames_reach_the_checkpoint_without_the_key(monkeypatch):
    monkeypatch.setattr(ckpt, "load_config", _config_must_not_be_read)
    monkeypatch.setattr(sepconv, "load_file_from_github_release", _nothing_may_load)
    with pytest.raises(AssertionError, match="before the checkpoint"):
        cfi_amd.sepconv.SepconvVFI().vfi("sepconv.pth", torch.zeros(1, 1, 1, 3).expand(2, 1440, 2560, 3))


def test_the_key_is_documented_in_the_config_file():
    with open(os.path.join(os.path.dirname(os.path.abspath(sepconv.__file__)), "config.yaml")) as fh:
        text = fh.read()
    assert "# sepconv_large_frames: true" in text and "8 388 607" in text and "4 194 303" in text
    assert "\nsepconv_large_frames" not in text      # a commented line: absent by default


def test_band_arithmetic_program_under_ubsan(tmp_path):
    """csrc/sepconv_bands.h, the header csrc/sepconv_net.hip plans its bands with, for a sweep of frame sizes and every legal band height"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "sepconv_bands")
    src = os.path.join(ROOT, "tests", "hostcheck", "sepconv_bands.cpp")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Xarch_host", "-fsanitize=undefined,signed-integer-overflow",
                           "-Xarch_host", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sepconv_bands: ok" in r.stdout and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
