"""FILM on 2160x3840 frames: the object's entry guard and limit, its layers' permission for operands of 4 GiB and more (csrc/film_net.hip,
docs/design/film.md "4K"), and the node's one-lane rule.

1. Forced through the net: with large_image_bytes = 1 every layer with a LARGE form takes it; 64x96 and the reference golden case give the
   bits of the unforced forward, and the golden within 1e-3.
2. 2160x3840, one pair: shape, finite, the same pair twice and two streams against one bit for bit, the LARGE launches are exactly the
   seven the design note lists, the workspace is the design note's figure.
3. 1440x2560 and 1536x3328, just under the limit the object had before: finite and repeatable.
4. Limits: a frame one row under vfi_film_max_pixels() runs, 2176x4800 is refused before any allocation.
5. The node on a three-frame 4K clip: five frames, sources bit for bit, new frames = engine.forward on the pairs, one lane.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from cfi_amd import synth

pytestmark = pytest.mark.gpu

LARGE_DEFAULT = 2 ** 31 - 1
GEN2, WINO = 2, 3
# docs/design/film.md, "4K": device bytes of the workspace after one 2160x3840 forward with two streams
WORKSPACE_4K = 69_254_794_560
# ... and the layers that take a LARGE form there, as (Hin, Win, in_cs, Cout): pred[0][0] and pred[1][0] once per flow direction on tw[k][0] /
# tw[k][1], the fusion's second convolution of levels 2, 1, 0 on al[2], al[1], al[0]
LARGE_4K = sorted([(2160, 3840, 132, 32)] * 2 + [(1080, 1920, 388, 64)] * 2 + [(540, 960, 1168, 256), (1080, 1920, 528, 128), (2160, 3840, 208, 64)])


@pytest.fixture(scope="module")
def lib(hip_lib):
    return hip_lib


@pytest.fixture(scope="module")
def sd():
    return synth.film_synth_state_dict(1234)


@pytest.fixture(scope="module")
def engine(lib, sd):
    from cfi_amd.film import FilmEngine

    eng = FilmEngine(sd)
    yield eng
    eng.close()
    torch.cuda.empty_cache()


def _large_launches(lib):
    log = (C.c_int32 * (6 * 256))()
    n = lib.vfi_test_large_launches(log, 256)
    return [tuple(log[6 * i:6 * i + 6]) for i in range(n)]


def test_forced_through_the_net(lib, engine, golden_dir):
    g = np.load(os.path.join(golden_dir, "film_net.npz"))
    gfr, gout = torch.from_numpy(g["frames"]), torch.from_numpy(g["out"])[0]
    small = synth.smooth_frames(2, 64, 96, seed=5, shift=2.0)
    try:
        for fr, want in ((small, None), (gfr, gout)):
            x0, x1 = fr[0].cuda().contiguous(), fr[1].cuda().contiguous()
            assert lib.vfi_test_set_option(b"large_image_bytes", LARGE_DEFAULT) == 0
            _large_launches(lib)
            plain = engine.forward(x0, x1).cpu()
            assert _large_launches(lib) == []
            assert lib.vfi_test_set_option(b"large_image_bytes", 1) == 0
            forced = engine.forward(x0, x1).cpu()
            n_forced = len(_large_launches(lib))
            print(f"{tuple(fr.shape[1:3])}: {n_forced} launches took a LARGE form when forced")
            assert n_forced > 0
            assert torch.equal(forced.view(torch.int32), plain.view(torch.int32))
            if want is not None:
                assert (forced - want).abs().max().item() <= 1e-3
    finally:
        lib.vfi_test_set_option(b"large_image_bytes", LARGE_DEFAULT)


def test_4k_pair(lib, engine):
    fr = synth.smooth_frames(2, 2160, 3840, seed=3, shift=4.0)
    x0, x1 = fr[0].cuda().contiguous(), fr[1].cuda().contiguous()
    try:
        _large_launches(lib)
        a = engine.forward(x0, x1)
        torch.cuda.synchronize()
        launches = _large_launches(lib)
        ws = engine.workspace_now()
        print(f"FILM 2160x3840: workspace {ws} bytes; LARGE launches {launches}")
        assert a.shape == (2160, 3840, 3) and bool(torch.isfinite(a).all())
        assert all(e[0] in (GEN2, WINO) for e in launches)
        assert sorted((e[1], e[2], e[3], e[5]) for e in launches) == LARGE_4K
        assert abs(ws - WORKSPACE_4K) <= WORKSPACE_4K // 100, ws
        b = engine.forward(x0, x1)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the same pair twice"
        assert lib.vfi_test_set_option(b"film_side", 0) == 0
        c = engine.forward(x0, x1)
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), "one stream against two"
    finally:
        lib.vfi_test_set_option(b"film_side", 1)
        engine.release_workspace()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("h,w", [(1440, 2560), (1536, 3328)])
def test_just_under_the_old_limit(lib, engine, h, w):
    assert h * w <= 5162220
    fr = synth.smooth_frames(2, h, w, seed=h, shift=3.0)
    x0, x1 = fr[0].cuda().contiguous(), fr[1].cuda().contiguous()
    try:
        _large_launches(lib)
        a = engine.forward(x0, x1)
        b = engine.forward(x0, x1)
        launches = _large_launches(lib)
        print(f"FILM {h}x{w}: workspace {engine.workspace_now()} bytes; LARGE launches per forward {launches[:len(launches) // 2]}")
        assert bool(torch.isfinite(a).all()) and torch.equal(a.view(torch.int32), b.view(torch.int32))
        # below 4 GiB per operand: whatever takes a LARGE form here took it before the permission existed
        assert all(e[1] * e[2] * e[3] * 4 <= 2 ** 32 - 1 for e in launches)
    finally:
        engine.release_workspace()
        torch.cuda.empty_cache()


def test_limits(lib, engine):
    from cfi_amd import _lib

    limit = lib.vfi_film_max_pixels()
    assert limit == lib.vfi_conv_huge_max_floats() // 208
    h, w = limit // 4096, 4096      # one row (and a bit) under the limit
    assert h == 2520 and (h + 1) * w > limit
    x = torch.rand(h, w, 3, device="cuda")
    try:
        out = engine.forward(x, x)
        assert out.shape == (h, w, 3) and bool(torch.isfinite(out).all())
    finally:
        engine.release_workspace()
        del x
        torch.cuda.empty_cache()
    # over the limit: refused before any allocation or launch.  Buffers of the claimed size, as for the layers' refusals
    H, W = 2176, 4800
    assert H * W > limit
    big, out = torch.zeros(H, W, 3, device="cuda"), torch.zeros(H, W, 3, device="cuda")
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    rc = lib.vfi_film_forward(engine.handle, big.data_ptr(), big.data_ptr(), 3, H, W, out.data_ptr(), 0, _lib.stream_ptr())
    msg = _lib.last_error()
    torch.cuda.synchronize()
    assert rc != 0 and "2176x4800" in msg and "FILM" in msg and f"{limit} pixels" in msg and "level 0" in msg, msg
    assert torch.cuda.mem_get_info()[0] == free0 and engine.workspace_now() == 0
    assert float(out.abs().max()) == 0.0
    with pytest.raises(RuntimeError, match="over the size limit of FILM"):
        engine.forward(big, big)


def test_node_on_a_4k_clip(lib, sd, tmp_path, monkeypatch):
    import cfi_amd.film as FM
    from cfi_amd import ckpt
    from cfi_amd.film import FilmEngine

    monkeypatch.delenv("VFI_PAIR_LANES", raising=False)
    pth = tmp_path / "film_net_fp32.pt"
    torch.save(sd, pth)
    monkeypatch.setattr(FM, "load_file_from_github_release", lambda model_type, ckpt_name: str(pth))
    frames = synth.smooth_frames(3, 2160, 3840, seed=6, shift=4.0)
    ckpt.clear_engine_cache()
    try:
        (out,) = FM.FILM_VFI().vfi("film_net_fp32.pt", frames, multiplier=2)
        assert out.shape == (5, 2160, 3840, 3)
        assert torch.equal(out[0::2], frames[..., :3]), "source frames pass through bit for bit"
        lanes = ckpt._engine_cache[FM.MODEL_TYPE][1]
        assert lanes.k == 1 and len(lanes.engines) == 1 and lanes.k_built == 2, "one lane above 5 162 220 pixels"
    finally:
        ckpt.clear_engine_cache()
        torch.cuda.empty_cache()
    eng = FilmEngine(sd)
    try:
        for p in (0, 1):
            want = eng.forward(frames[p].cuda().contiguous(), frames[p + 1].cuda().contiguous(), clamp=True).cpu()
            assert torch.equal(out[2 * p + 1].view(torch.int32), want.view(torch.int32)), f"new frame of pair {p}"
    finally:
        eng.close()
        torch.cuda.empty_cache()
