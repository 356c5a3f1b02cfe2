"""CPU: XVFI's large frames behind config.yaml's ``xvfi_large_frames`` key — the key's three states read at call time, the size check of both
configurations at 2160x3840 and at the first refused size, the node's refusal before a checkpoint or an engine exists, and the constant.
``ckpt.load_config`` is patched to turn the key on: the package's config.yaml leaves it off."""
import pytest
import torch

import cfi_amd
import xvfi_restated as xr
from cfi_amd import ckpt, xvfi, xvfi_spec


def config_with(value):
    real = ckpt.load_config

    def load():
        cfg = dict(real())
        cfg["xvfi_large_frames"] = value
        return cfg
    return load


def _no_engine(*a, **k):
    raise AssertionError("the refusals must come before the checkpoint and the engine")


def test_the_constant():
    assert xvfi.LARGE_MAX_PADDED_PIXELS == (2 ** 32 - 1) // 320 == 13421772
    assert xvfi.FLOATS_PER_PADDED_PIXEL * 4 == 320
    assert xvfi.MAX_PADDED_PIXELS == (2 ** 31 - 1) // 320 == 6710886      # the limit with the key off is what it was


def test_key_absent_false_true_read_at_call_time(monkeypatch):
    assert "xvfi_large_frames" not in ckpt.load_config()                  # the package's own config.yaml: absent = off
    assert not xvfi.large_frames_enabled() and xvfi.max_padded_pixels() == 6710886
    monkeypatch.setattr(ckpt, "load_config", config_with(False))
    assert not xvfi.large_frames_enabled() and xvfi.max_padded_pixels() == 6710886
    monkeypatch.setattr(ckpt, "load_config", config_with(True))          # no reload, no new import: the next call sees it
    assert xvfi.large_frames_enabled() and xvfi.max_padded_pixels() == 13421772
    monkeypatch.setattr(ckpt, "load_config", config_with(False))
    assert not xvfi.large_frames_enabled() and xvfi.max_padded_pixels() == 6710886


@pytest.mark.parametrize("ckpt_name,padded", [(xr.V, (2160, 3840)), (xr.X, (2560, 4096))])
def test_check_frame_size_at_4k(monkeypatch, ckpt_name, padded):
    cfg = xvfi_spec.config_of(ckpt_name)
    assert xvfi_spec.padded_size(2160, 3840, cfg) == padded
    assert padded[0] * padded[1] > xvfi.MAX_PADDED_PIXELS
    with pytest.raises(ValueError, match=r"2160x3840 frames \(padded %dx%d\) are beyond the kernels' index arithmetic \(6710886 padded pixels\)" % padded):
        xvfi.check_frame_size(2160, 3840, cfg)                            # key off: as before
    monkeypatch.setattr(ckpt, "load_config", config_with(True))
    xvfi.check_frame_size(2160, 3840, cfg)
    xvfi.check_frame_size(1080, 1920, cfg)


def test_the_first_refused_sizes_with_the_key_on(monkeypatch):
    monkeypatch.setattr(ckpt, "load_config", config_with(True))
    x4k, vimeo = xvfi_spec.config_of(xr.X), xvfi_spec.config_of(xr.V)
    # X4K pads to multiples of 512: 2560x4608 and 3072x4096 still fit, the first size beyond the limit is 3072x4608
    xvfi.check_frame_size(2560, 4608, x4k)
    xvfi.check_frame_size(3072, 4096, x4k)
    assert xvfi_spec.padded_size(2561, 4097, x4k) == (3072, 4608) and 3072 * 4608 > xvfi.LARGE_MAX_PADDED_PIXELS
    with pytest.raises(ValueError, match=r"padded 3072x4608.*index arithmetic \(13421772 padded pixels\)"):
        xvfi.check_frame_size(2561, 4097, x4k)
    with pytest.raises(ValueError, match="index arithmetic"):
        xvfi.check_frame_size(3072, 4608, x4k)
    # Vimeo pads to multiples of 16: the limit itself is the boundary
    xvfi.check_frame_size(3200, 4192, vimeo)                              # 13 414 400 pixels
    assert 3216 * 4176 > xvfi.LARGE_MAX_PADDED_PIXELS
    with pytest.raises(ValueError, match="index arithmetic"):
        xvfi.check_frame_size(3216, 4176, vimeo)                          # 13 430 016


def test_the_node_refuses_before_any_engine_is_built(monkeypatch):
    monkeypatch.setattr(xvfi, "load_file_from_github_release", _no_engine)
    monkeypatch.setattr(xvfi, "cached_engine", _no_engine)
    clip_4k = torch.zeros(1, 1, 1, 3).expand(2, 2160, 3840, 3)
    too_big = torch.zeros(1, 1, 1, 3).expand(2, 3072, 4608, 3)
    for name in (xr.V, xr.X):                                             # key off: 4K is refused by the node, as before
        with pytest.raises(ValueError, match="index arithmetic"):
            cfi_amd.XVFI().vfi(name, clip_4k, 1, 2)
    monkeypatch.setattr(ckpt, "load_config", config_with(True))
    for name in (xr.V, xr.X):
        with pytest.raises(ValueError, match=r"3072x4608.*index arithmetic \(13421772 padded pixels\)"):
            cfi_amd.XVFI().vfi(name, too_big, 1, 2)
        # 4K passes the size check with the key on: the next thing the node does is ask for the checkpoint
        with pytest.raises(AssertionError, match="before the checkpoint and the engine"):
            cfi_amd.XVFI().vfi(name, clip_4k, 1, 2)


def test_the_key_is_documented_in_the_config_file():
    import os

    path = os.path.join(os.path.dirname(os.path.abspath(xvfi.__file__)), "config.yaml")
    with open(path) as fh:
        text = fh.read()
    assert "# xvfi_large_frames: true" in text and "13 421 772" in text
