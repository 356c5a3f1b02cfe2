"""FLAVR on frames up to 8 388 607 padded pixels (config.yaml's ``flavr_large_frames``), on the device.

1. Forced, through the net: with the switch on and the test option large_image_bytes at 1 byte every layer of the forward that has a
   large-image form takes it (the log of LARGE launches, vfi_test_large_launches); every golden case of tests/golden/flavr_net.npz comes out
   bit-identical to the un-forced run.  At the golden sizes (up to 112x192 padded) the transposed layers' inputs are at most 56x96, under
   the 128x128 from which a transposed layer takes the Winograd form at all, so they run the grouped direct tile forced or not — sending
   them to the large Winograd form would change their summation order and break the bit-identity this test is about.  The large transposed
   form is therefore asserted through the net at 512x512, the smallest square frame at which both dec[2] (128x128 input) and dec[4]
   (256x256) take it, again bit-identical to the un-forced run.
2. 1104x1920, the first frame over the old limit (2 119 680 padded pixels, the frame of test_gpu_flavr's refusal test): served with the key
   on, every pixel within 1e-3 of the float32 restatement; refused as before with it off.  The restatement runs once for this file.
3. 2160x3840 with the switch on: finite, the same window twice bit-identical, the workspace of docs/design/flavr.md (51 759 157 264 bytes).
4. 2176x3856, over the large limit: refused before any launch.
5. The node: a 4-frame 1104x1920 clip with the key patched on; with it off the node raises, naming the key.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cain_restated
import flavr_restated
from gpu_util import describe_diff
from test_flavr_spec_cpu import NET_CASES, window
from test_gpu_flavr import SEED, TOL, _forward, _smooth_window, engines, lib      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
NAN = float("nan")
LARGE_DEFAULT = 2 ** 31 - 1
GEN2, WINO = 2, 3
OLD, LARGE = 2097151, 8388607
WORKSPACE_4K = 4 * (1560 * 2160 * 3840 + 4 + 1024 * 512 + 1024)      # docs/design/flavr.md "4K": 1560 floats per padded pixel + the scratch block


def _large_log(hip_lib):
    buf = (C.c_int32 * (6 * 256))()
    n = hip_lib.vfi_test_large_launches(buf, 256)
    return [tuple(buf[6 * i:6 * i + 6]) for i in range(min(n, 256))]


def _config(**keys):
    from cfi_amd import ckpt

    real = ckpt.load_config
    return lambda: dict(real(), **keys)


def _forced_equals_plain(hip_lib, engine, fr, what):
    """-> (output, the log of LARGE launches of the forced run); asserts the forced run's bits are the un-forced run's"""
    engine._call("set_large_frames", 0)
    _large_log(hip_lib)
    want = _forward(engine, fr)
    assert _large_log(hip_lib) == [], what + ": a large form ran without the mark"
    engine._call("set_large_frames", 1)
    assert hip_lib.vfi_test_set_option(b"large_image_bytes", 1) == 0
    try:
        got = _forward(engine, fr)
        log = _large_log(hip_lib)
    finally:
        hip_lib.vfi_test_set_option(b"large_image_bytes", LARGE_DEFAULT)
        engine._call("set_large_frames", 0)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), what + ": the large path differs from the default path"
    return got, log


@pytest.mark.parametrize("name", sorted(NET_CASES))
def test_golden_cases_forced_large(name, hip_lib, engines, golden_dir):
    n_outputs, h, w, stride, fseed = NET_CASES[name]
    engine, _ = engines(n_outputs)
    gd = np.load(os.path.join(golden_dir, "flavr_net.npz"))
    got, log = _forced_equals_plain(hip_lib, engine, window(h, w, fseed), name)
    d, sums_ok = cain_restated.compare(got, gd, name + "_", stride, TOL)
    assert d <= TOL and sums_ok, (name, d, sums_ok)
    hp, wp = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    keyed = {(e[1], e[2], e[3], e[4], e[5]) for e in log}
    print(name, "large launches", sorted(keyed))
    # feature_fuse (1x1 on fin, second-generation direct kernel) is among the large launches whatever tile the 3x3 layers get at this size
    assert (hp, wp, 256, 256, 64) in keyed, (name, sorted(keyed))
    # ... the transposed layers are not: under 128x128 input pixels they stay on the grouped direct tile, forced or not (see the module text)
    transposed = {(WINO, hp // 8, wp // 8, 3072, 1536, 512), (WINO, hp // 4, wp // 4, 1536, 768, 256), (WINO, hp // 2, wp // 2, 768, 384, 256)}
    assert not transposed & set(log), (name, log)


def test_512x512_forced_reaches_the_large_transposed_form(hip_lib, engines):
    engine, _ = engines(1)
    _, log = _forced_equals_plain(hip_lib, engine, _smooth_window(512, 512, 11), "512x512")
    # (family, Hin, Win, in_cs, Cin_p, Cout of the 3x3 form = 4 x 64): dec[4] on (dx_0 | x_0) and dec[2] on (dx_2 | x_2), four time slices each
    assert log.count((WINO, 256, 256, 768, 384, 256)) == 4 and log.count((WINO, 128, 128, 1536, 768, 256)) == 4, log


# ---- just over the old limit -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def over_old():
    """The 1104x1920 window and its float32 restatement, made once"""
    from cfi_amd.flavr_spec import seeded_state_dict

    fr = _smooth_window(1104, 1920, 6)
    before = torch.get_num_threads()
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    try:
        with torch.no_grad():
            want = flavr_restated.flavr_forward(seeded_state_dict(SEED, 1), fr)[0].permute(1, 2, 0).contiguous()
    finally:
        torch.set_num_threads(before)
    return fr, want


def test_1104x1920_is_served_with_the_key_and_refused_without(monkeypatch, hip_lib, engines, over_old):
    from cfi_amd import ckpt

    engine, _ = engines(1)
    fr, want = over_old
    assert engine.max_padded_pixels() == OLD == hip_lib.vfi_flavr_max_padded_pixels()
    dev = [f[0].permute(1, 2, 0).contiguous().cuda() for f in fr]
    with pytest.raises(RuntimeError, match="size limit"):      # key off: refused as before
        engine.forward(dev)
    with monkeypatch.context() as mp:
        mp.setattr(ckpt, "load_config", _config(flavr_large_frames=True))
        _large_log(hip_lib)
        got = engine.forward(dev)[0].cpu()
        log = _large_log(hip_lib)
        assert engine.max_padded_pixels() == LARGE == hip_lib.vfi_flavr_large_max_padded_pixels()
    print("1104x1920 workspace bytes", engine.workspace_bytes(), "max |d|", (got - want).abs().max().item(), "large launches", sorted(set(log)))
    assert torch.isfinite(got).all()
    assert (got - want).abs().max().item() <= TOL, describe_diff(got, want, "1104x1920")
    # the one tensor over 2 GiB is fin [1104, 1920, 256]: dec[4] writes it (large transposed form), feature_fuse reads it (direct 1x1, large)
    assert log.count((WINO, 552, 960, 768, 384, 256)) == 4 and (GEN2, 1104, 1920, 256, 256, 64) in log and len(log) == 5, log
    assert engine.workspace_bytes() == 4 * (1560 * 1104 * 1920 + 4 + 1024 * 512 + 1024)
    with pytest.raises(RuntimeError, match="size limit"):      # the key is read again: off, the same frame is refused again
        engine.forward(dev)
    assert engine.max_padded_pixels() == OLD
    engine.release_workspace()


def test_node_serves_a_clip_over_the_old_limit_with_the_key(monkeypatch, tmp_path, hip_lib, over_old):
    from cfi_amd import ckpt, flavr
    from cfi_amd.flavr_spec import seeded_state_dict

    fr, want = over_old
    frames = torch.cat([f[0].permute(1, 2, 0)[None] for f in fr]).contiguous()      # [4, 1104, 1920, 3]
    path = str(tmp_path / "FLAVR_2x.pth")
    torch.save({"state_dict": {"module." + k: v for k, v in seeded_state_dict(SEED, 1).items()}}, path)
    monkeypatch.setattr(flavr, "load_file_from_github_release", lambda model_type, name: path)
    ckpt.clear_engine_cache()
    node = flavr.FLAVR_VFI()
    try:
        with pytest.raises(ValueError, match="flavr_large_frames: true raises it to 8388607"):
            node.vfi("FLAVR_2x.pth", frames)
        monkeypatch.setattr(ckpt, "load_config", _config(flavr_large_frames=True))
        out = node.vfi("FLAVR_2x.pth", frames)[0]
        assert out.shape == (5, 1104, 1920, 3)
        assert torch.equal(out[[0, 1, 3, 4]], frames), "original frames not bit-equal"
        assert (out[2] - want).abs().max().item() <= TOL, describe_diff(out[2], want, "node 1104x1920")
    finally:
        ckpt.clear_engine_cache()


# ---- 4K and beyond ---------------------------------------------------------------------------------------------------------------------------

def test_4k_smoke(monkeypatch, hip_lib, engines):
    from cfi_amd import ckpt

    engine, _ = engines(1)
    monkeypatch.setattr(ckpt, "load_config", _config(flavr_large_frames=True))      # the engine reads the key for a frame over the old limit
    try:
        g = torch.Generator(device="cuda").manual_seed(4)
        dev = [torch.rand(2160, 3840, 3, device="cuda", generator=g) for _ in range(4)]
        a = engine.forward(dev).clone()
        assert engine.workspace_bytes() == WORKSPACE_4K == 51759157264
        b = engine.forward(dev)
        torch.cuda.synchronize()
        assert a.shape == (1, 2160, 3840, 3) and torch.isfinite(a).all()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the same window twice differs"
    finally:
        engine.release_workspace()
        engine._call("set_large_frames", 0)


def test_over_the_large_limit_is_refused_before_any_launch(lib, engines):
    from cfi_amd import _lib

    engine, _ = engines(1)
    engine._call("set_large_frames", 1)
    try:
        small = [torch.rand(32, 32, 3, device="cuda")] * 4
        engine.forward(small)
        before = engine.workspace_bytes()
        H, W = 2176, 3856                                       # 8 390 656 padded pixels: fin would hold over 2^31 - 1 floats
        f = torch.rand(H, W, 3, device="cuda")
        out = torch.full((1, H, W, 3), NAN, device="cuda")
        p = (C.c_void_p * 4)(*[f.data_ptr()] * 4)
        rc = lib.vfi_flavr_forward(engine.handle, p, 1, 3, H, W, out.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc != 0 and "size limit" in _lib.last_error() and "8388607" in _lib.last_error() and "2^31 - 1 floats" in _lib.last_error(), _lib.last_error()
        assert torch.isnan(out).all(), "something was written"
        assert engine.workspace_bytes() == before, "the workspace was touched"
        assert torch.isfinite(engine.forward(small)).all()      # the engine is still usable
    finally:
        engine._call("set_large_frames", 0)
