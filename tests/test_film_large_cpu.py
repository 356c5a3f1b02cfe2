"""CPU: FILM at 4K — the new C symbols (header, both libraries, the Python binding), the frame-size limit and its derivation from the channel
tables, the node's refusal before anything is loaded or uploaded, the one-lane rule above the old limit, and the stand-alone address check
of the layers' LARGE forms (tests/hostcheck/conv_large_addr.cpp, built with the undefined-behaviour sanitizer and run as a program)."""
import contextlib
import ctypes
import os
import re
import subprocess

import pytest
import torch

import cfi_amd
from cfi_amd import _lib, film, lanes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_PRODUCT = ("vfi_conv_allow_huge", "vfi_conv_huge_max_floats", "vfi_film_max_pixels", "vfi_film_workspace_bytes")
NEW_TAPS = ("vfi_test_large_launches",)
OLD_LIMIT = 5162220      # (2^32 - 1) // (208 * 4): FILM's limit by reading before the layers took operands of 4 GiB and more


def _declared(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(vfi_[a-z0-9_]+)\s*\(", src))


def test_new_symbols_header_libraries_binding(hip_lib):
    assert set(NEW_PRODUCT) <= _declared("vfi_hip.h")
    assert set(NEW_TAPS) == _declared("vfi_hip_test_large.h")
    for n in NEW_PRODUCT:
        assert n in _lib.PROTOTYPES and getattr(hip_lib, n) is not None
    assert set(_lib.LARGE_TEST_PROTOTYPES) == set(NEW_TAPS) and getattr(hip_lib, NEW_TAPS[0]) is not None
    product, test = ctypes.CDLL(_lib.LIB_PATH), ctypes.CDLL(_lib.TEST_LIB_PATH)
    for n in NEW_PRODUCT:
        assert hasattr(product, n) and hasattr(test, n), n
    for n in NEW_TAPS:
        assert hasattr(test, n) and not hasattr(product, n), n


def test_pixel_limit_is_derived_from_the_channel_tables(hip_lib):
    """vfi_film_max_pixels = the layers' bound for one operand image / the floats per pixel of the widest tensor, al[0]: the aligned level 0
    [img 3 + pad 1 + features 64] x 2 + 4 flow channels, padded to 8s, plus the 64 channels of the fusion's up-sampling layer"""
    feat0 = 64
    cal0 = (2 * (4 + feat0) + 4 + 7) // 8 * 8
    assert cal0 == 144
    bound = hip_lib.vfi_conv_huge_max_floats()
    assert bound == 2 ** 31 - 1
    limit = hip_lib.vfi_film_max_pixels()
    assert limit == bound // (cal0 + 64) == 10324440 == film.max_pixels()
    assert 2160 * 3840 <= limit and 2160 * 4096 <= limit < 2176 * 4800
    assert OLD_LIMIT == (2 ** 32 - 1) // ((cal0 + 64) * 4) == film.LANE_PIXELS
    assert 2560 * 1440 <= OLD_LIMIT < 3200 * 1800


def test_null_handles(hip_lib):
    assert hip_lib.vfi_film_workspace_bytes(None) == 0
    assert hip_lib.vfi_conv_allow_huge(None, 1) != 0 and "null handle" in _lib.last_error()


def _nothing_may_load(*a, **k):
    raise AssertionError("the refusal must come before the checkpoint, the engine and any upload")


class StandIn:
    """An engine on the CPU that records its calls (nodeloop.run_plan's stand-in path)"""
    device = torch.device("cpu")

    def __init__(self):
        self.forwards = 0

    def forward(self, x0, x1, clamp=False):
        self.forwards += 1
        return (x0[..., :3] + x1[..., :3]) * 0.5

    def release_workspace(self):
        pass

    def close(self):
        pass


def test_the_node_refuses_2176x4800_before_any_upload(hip_lib, monkeypatch):
    monkeypatch.setattr(film, "load_file_from_github_release", _nothing_may_load)
    monkeypatch.setattr(film, "cached_engine", _nothing_may_load)
    monkeypatch.setattr(film, "run_plan", _nothing_may_load)
    too_big = torch.zeros(1, 1, 1, 3).expand(2, 2176, 4800, 3)      # no memory behind it: the check reads the shape only
    with pytest.raises(ValueError, match=r"FILM VFI: a 2176x4800 frame is over the size limit of FILM, 10324440 pixels"):
        cfi_amd.FILM_VFI().vfi("film_net_fp32.pt", too_big, 10, 2)
    with pytest.raises(ValueError, match="10324440 pixels"):
        film.check_frame_size(2176, 4800)
    film.check_frame_size(2160, 3840)
    film.check_frame_size(2160, 4096)
    film.check_frame_size(2520, 4097)      # 10 324 440 exactly
    # a frame inside the limit goes on: the next thing the node does is ask for the checkpoint
    with pytest.raises(AssertionError, match="before the checkpoint"):
        cfi_amd.FILM_VFI().vfi("film_net_fp32.pt", torch.zeros(1, 1, 1, 3).expand(2, 2160, 3840, 3), 10, 2)


def test_the_stand_in_engine_runs_a_clip_through_the_node(hip_lib, monkeypatch):
    """... and with a stand-in engine the node's path is whole: the size check passes, the lane set is built for the frame size"""
    eng = StandIn()
    monkeypatch.setattr(film, "load_file_from_github_release", lambda *a: "film_net_fp32.pt")
    monkeypatch.setattr(film, "cached_engine", lambda kind, path, build: (eng, False))
    monkeypatch.setattr(film, "engine_call", lambda entry, shape: contextlib.nullcontext(entry[0]))
    frames = torch.rand(3, 64, 96, 3)
    (out,) = cfi_amd.FILM_VFI().vfi("film_net_fp32.pt", frames, 10, 2)
    assert out.shape == (5, 64, 96, 3) and eng.forwards == 2
    assert torch.equal(out[0::2], frames)


def test_lane_rule(monkeypatch):
    monkeypatch.delenv("VFI_PAIR_LANES", raising=False)
    default = lanes.DEFAULT_LANES["film"]
    assert default == 2
    for h, w in ((64, 96), (1080, 1920), (1440, 2560), (1536, 3328)):
        assert h * w <= OLD_LIMIT and film.lanes_for_frame(h, w) == default
    assert film.lanes_for_frame(1, OLD_LIMIT) == default and film.lanes_for_frame(1, OLD_LIMIT + 1) == 1
    for h, w in ((1800, 3200), (2160, 3840), (2160, 4096)):
        assert film.lanes_for_frame(h, w) == 1
    ls = film.film_lane_set(StandIn)
    assert ls.k == default and ls.pairs_per_lane == lanes.PAIRS_PER_LANE["film"]
    film.limit_lanes(ls, 2160, 3840)
    assert ls.k == 1 and lanes.lanes_of(ls, 100)[1] == 1
    film.limit_lanes(ls, 1080, 1920)      # the same cached set on a later 1080p call: its lanes are back
    assert ls.k == default and lanes.lanes_of(ls, 100)[1] == default
    monkeypatch.setenv("VFI_PAIR_LANES", "3")      # the override still rules below the mark, and never opens lanes above it
    assert film.lanes_for_frame(1080, 1920) == 3 and film.lanes_for_frame(2160, 3840) == 1
    assert lanes.DEFAULT_LANES == {"m2m": 3, "film": 2, "gmfss": 3, "ifunet": 3, "ifrnet": 2}      # nobody else's lanes moved


def test_film_engine_still_reports_no_workspace_bytes():
    assert not hasattr(film.FilmEngine, "workspace_bytes") and hasattr(film.FilmEngine, "workspace_now")


def test_address_check_program_under_ubsan(tmp_path):
    """The shared address helpers of csrc/conv_large.h for every tile and region of FILM's three 4K layers, at the bound and just over it"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "conv_large_addr")
    src = os.path.join(ROOT, "tests", "hostcheck", "conv_large_addr.cpp")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Xarch_host", "-fsanitize=undefined,signed-integer-overflow",
                           "-Xarch_host", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "conv_large_addr: ok" in r.stdout and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
