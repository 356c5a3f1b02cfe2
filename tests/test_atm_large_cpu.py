"""CPU: ATM's large frames behind config.yaml's ``atm_large_frames`` key — the new C symbols and their null-handle answers, the key read at call
time, the size check of both variants at 2160x3840 and at the first refused multiple-of-64 shape, the node's refusal before a checkpoint or an
engine exists, and the Python limits against the library's.  ``ckpt.load_config`` is patched to turn the key on: the package's config.yaml
leaves it off."""
import ctypes
import os

import pytest
import torch

import cfi_amd
from cfi_amd import _lib, atm, atm_spec, ckpt

NEW = ["vfi_atm_set_large_frames", "vfi_atm_large_max_padded_pixels"]
LITE, BASE = 13421772, 8388607


def config_with(**keys):
    real = ckpt.load_config

    def load():
        cfg = dict(real())
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


def test_null_handles(hip_lib):
    assert hip_lib.vfi_atm_set_large_frames(None, 1) != 0 and "vfi_atm_set_large_frames: null object" in _lib.last_error()
    assert hip_lib.vfi_atm_object_max_padded_pixels(None) == 0
    assert hip_lib.vfi_atm_large_max_padded_pixels(2) == 0 and hip_lib.vfi_atm_large_max_padded_pixels(-1) == 0


def test_the_python_limits_are_the_librarys(hip_lib):
    assert atm.LARGE_MAX_PADDED_PIXELS == (2 ** 32 - 1) // 320 == LITE == hip_lib.vfi_atm_large_max_padded_pixels(0)
    assert atm.LARGE_MAX_PADDED_PIXELS_BASE == (2 ** 32 - 1) // 512 == BASE == hip_lib.vfi_atm_large_max_padded_pixels(1)
    assert atm.MAX_PADDED_PIXELS == 6710886 == hip_lib.vfi_atm_max_padded_pixels()      # the limits with the key off are what they were
    assert atm.MAX_PADDED_PIXELS_BASE == 4194303


def test_key_absent_false_true_read_at_call_time(monkeypatch):
    assert "atm_large_frames" not in ckpt.load_config()                  # the package's own config.yaml: absent = off
    assert not atm_spec.atm_large_frames_enabled() and (atm.max_padded_pixels("lite"), atm.max_padded_pixels("base")) == (6710886, 4194303)
    monkeypatch.setattr(ckpt, "load_config", config_with(atm_large_frames=False))
    assert not atm_spec.atm_large_frames_enabled() and (atm.max_padded_pixels("lite"), atm.max_padded_pixels("base")) == (6710886, 4194303)
    monkeypatch.setattr(ckpt, "load_config", config_with(atm_large_frames=True))      # no reload, no new import: the next call sees it
    assert atm_spec.atm_large_frames_enabled() and (atm.max_padded_pixels("lite"), atm.max_padded_pixels("base")) == (LITE, BASE)
    monkeypatch.setattr(ckpt, "load_config", config_with(atm_large_frames=False))
    assert (atm.max_padded_pixels("lite"), atm.max_padded_pixels("base")) == (6710886, 4194303)


def test_no_environment_variable_turns_it_on(monkeypatch):
    for name in ("ATM_LARGE_FRAMES", "VFI_ATM_LARGE_FRAMES", "atm_large_frames"):
        monkeypatch.setenv(name, "1")
    assert not atm_spec.atm_large_frames_enabled()


@pytest.mark.parametrize("variant,old", [("lite", 6710886), ("base", 4194303)])
def test_check_frame_size_at_4k(monkeypatch, variant, old):
    assert atm.padded_size(2160, 3840) == (2176, 3840) and 2176 * 3840 == 8355840
    suffix = " for ATM-base" if variant == "base" else ""
    with pytest.raises(ValueError, match=r"ATM VFI: 2160x3840 frames \(padded 2176x3840\) are beyond the kernels' index arithmetic \(%d padded pixels%s\)" % (old, suffix)):
        atm.check_frame_size(2160, 3840, variant)                         # key off: the message it always had
    monkeypatch.setattr(ckpt, "load_config", config_with(atm_large_frames=True))
    atm.check_frame_size(2160, 3840, variant)
    atm.check_frame_size(1080, 1920, variant)


def test_the_first_refused_sizes_with_the_key_on(monkeypatch):
    monkeypatch.setattr(ckpt, "load_config", config_with(atm_large_frames=True))
    # lite: 13 421 772 padded pixels fit, 13 421 773 do not.  Shapes are multiples of 64: 2880x4608 = 13 271 040 fits, one more 64-row
    # band (2944x4608 = 13 565 952) is the first shape of that width that does not; 3264x4096 = 13 369 344 fits, 3328x4096 does not
    atm.check_frame_size(2880, 4608, "lite")
    atm.check_frame_size(3264, 4096, "lite")
    assert 2880 * 4608 <= LITE < LITE + 1 <= 2944 * 4608 and 3264 * 4096 <= LITE < 3328 * 4096
    with pytest.raises(ValueError, match=r"padded 2944x4608.*index arithmetic \(13421772 padded pixels\)"):
        atm.check_frame_size(2881, 4608, "lite")                          # pads to 2944
    with pytest.raises(ValueError, match="index arithmetic"):
        atm.check_frame_size(3328, 4096, "lite")
    # base: 8 388 607 fit, 8 388 608 = 2048x4096 exactly is the first that does not; 2176x3840 (4K) and 1984x4224 fit
    atm.check_frame_size(2176, 3840, "base")
    atm.check_frame_size(1984, 4224, "base")
    assert 2048 * 4096 == BASE + 1
    with pytest.raises(ValueError, match=r"padded 2048x4096.*index arithmetic \(8388607 padded pixels for ATM-base\)"):
        atm.check_frame_size(2048, 4096, "base")
    with pytest.raises(ValueError, match="index arithmetic"):
        atm.check_frame_size(2240, 3840, "base")                          # one 64-row band beyond 4K


def test_the_node_refuses_before_any_engine_is_built(monkeypatch):
    monkeypatch.setattr(atm, "load_file_from_github_release", _no_engine)
    monkeypatch.setattr(atm, "cached_engine", _no_engine)
    clip_4k = torch.zeros(1, 1, 1, 3).expand(2, 2160, 3840, 3)
    too_big = torch.zeros(1, 1, 1, 3).expand(2, 3328, 4096, 3)
    names = ("atm-vfi-lite.pt", "atm-vfi-base.pt")
    monkeypatch.setattr(ckpt, "load_config", config_with(atm_base=True, atm_ensemble=True))
    for name in names:                                                    # key off: 4K is refused by the node, as before
        with pytest.raises(ValueError, match="index arithmetic"):
            cfi_amd.atm.ATM_VFI().vfi(name, clip_4k, 10, 2, "On")
    monkeypatch.setattr(ckpt, "load_config", config_with(atm_base=True, atm_ensemble=True, atm_large_frames=True))
    for name in names:
        for gm in atm.GLOBAL_MOTION:                                      # all three global_motion choices
            with pytest.raises(ValueError, match=r"3328x4096.*index arithmetic"):
                cfi_amd.atm.ATM_VFI().vfi(name, too_big, 10, 2, gm)
            # 4K passes the size check with the key on: the next thing the node does is ask for the checkpoint
            with pytest.raises(AssertionError, match="before the checkpoint and the engine"):
                cfi_amd.atm.ATM_VFI().vfi(name, clip_4k, 10, 2, gm)


def test_the_key_is_documented_in_the_config_file():
    path = os.path.join(os.path.dirname(os.path.abspath(atm.__file__)), "config.yaml")
    with open(path) as fh:
        text = fh.read()
    assert "# atm_large_frames: true" in text and "13 421 772" in text and "8 388 607" in text
