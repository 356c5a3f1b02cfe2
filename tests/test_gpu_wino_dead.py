"""-m gpu: the Winograd kernel's dead-plane forms (csrc/conv_wino.hip, option wino_dead) give the bits of the all-16-planes loop.

A transposed-convolution layer's transform weights have whole zero plane rows / columns per 32-channel N block; with wino_dead = 1 (the
default) the K loop of such a block leaves those MFMAs, their B-fragment reads and their share of the input transform out.  An
accumulator that is never touched stays the +0 it was cleared to, which is what fma(x, +-0, +0) gives for every finite x — so the two
settings must agree in every bit, and each must be the transposed convolution (float64 torch, 2e-5 * max(1, |want|), the bound of
tests/test_gpu_ops.py::_deconv_case).

Shapes: regions are 16x8 pixels per wave.  vfi_deconv4x4_ps2 (LO = 24: the forms row 3 | column 0 | row 0 of the Gray order, SHUF 1
epilogue) at 9x17 and 5x7 (partial regions in both directions, 8 and 24 chunks) and at 8x16 with Cin 8 (one chunk per item, fully
interior).  Layer objects (SHUF 2, per-channel PReLU = epilogue MODE 1) with LO = 16 (row 3 | row 0) and LO = 32 at 9x17 — where the
object's selection rule sends them to the grouped direct kernel (it takes the Winograd form from 128 x 128 input pixels and 192 work
items), so the comparison holds there without reaching the new code — and therefore also at the smallest ragged sizes that DO reach it,
131x177 (LO = 16) and 129x133 (LO = 32); which kernel ran is read back, not guessed.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from gpu_util import describe_diff, hptr, nhwc, ptr

pytestmark = pytest.mark.gpu

WINO = 3      # vfi_test_last_conv_launch: kernel family


@pytest.fixture(scope="module")
def lib(hip_lib):
    from cfi_amd import _lib

    assert torch.cuda.is_available()
    _lib.check(hip_lib.vfi_init(0), "vfi_init")
    return hip_lib


def _ck(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


def _last(lib):
    rec = (C.c_int32 * 8)()
    assert lib.vfi_test_last_conv_launch(rec, 8) == 8
    return list(rec)


def _inputs(n, cin, h, w, seed):
    """[-1, 1) with exact zeros sprinkled in (one value in eight)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, cin, h, w, generator=g) * 2 - 1
    return x * (torch.rand(x.shape, generator=g) >= 0.125)


def _both(lib, run):
    """run() under wino_dead = 0 and 1 -> the two outputs (host) and the two launch records"""
    outs = []
    try:
        for dead in (0, 1):
            assert lib.vfi_test_set_option(b"wino_dead", dead) == 0
            before = _last(lib)[7]
            out = run()
            torch.cuda.synchronize()
            rec = _last(lib)
            assert rec[7] == before + 1, f"{rec[7] - before} convolution launches for one call"
            outs.append((out.cpu(), rec))
    finally:
        lib.vfi_test_set_option(b"wino_dead", 1)
    return outs


def _assert_bound(got, want, what):
    assert not torch.isnan(got).any(), what
    tol = 2e-5 * max(1.0, want.abs().max().item())
    err = (got.double() - want).abs().max().item()
    print(f"  {what}: max err {err:.3e}, bound {tol:.3e}")
    assert err <= tol, describe_diff(got.double(), want, what)


@pytest.mark.parametrize("cin,h,w", [(64, 9, 17), (192, 5, 7), (8, 8, 16)])
def test_deconv_ps2_same_bits(lib, cin, h, w):
    n, lo = 2, 24
    x = _inputs(n, cin, h, w, cin + h)
    g = torch.Generator().manual_seed(cin)
    wt = (torch.rand(cin, lo, 4, 4, generator=g) * 2 - 1) / (cin * 4) ** 0.5
    b = torch.rand(lo, generator=g) - 0.5
    want = nhwc(F.pixel_shuffle(F.conv_transpose2d(x.double(), wt.double(), b.double(), 2, 1), 2))
    xd = nhwc(x).cuda()

    def run():
        out = torch.full(want.shape, float("nan"), device="cuda")
        _ck(lib.vfi_deconv4x4_ps2(ptr(xd), hptr(wt), hptr(b), ptr(out), n, h, w, cin, lo, None), "vfi_deconv4x4_ps2")
        return out

    (ref, rec0), (got, rec1) = _both(lib, run)
    for rec in (rec0, rec1):
        assert rec[0] == WINO and rec[1] == 8 and rec[2] == 0 and rec[3] == 1, rec      # Winograd, 16x8 regions, hot epilogue, SHUF 1
    assert (x == 0).sum() > 0
    _assert_bound(ref, want, f"deconv+ps {cin}@{h}x{w} wino_dead=0")
    _assert_bound(got, want, f"deconv+ps {cin}@{h}x{w} wino_dead=1")
    assert torch.equal(got, ref), describe_diff(got, ref, "wino_dead 1 vs 0")


@pytest.mark.parametrize("lo,h,w,reaches", [(16, 9, 17, False), (32, 9, 17, False), (16, 131, 177, True), (32, 129, 133, True)])
def test_layer_object_prelu_same_bits(lib, lo, h, w, reaches):
    n, cin = 2, 8
    x = _inputs(n, cin, h, w, lo + h)
    g = torch.Generator().manual_seed(lo)
    wt = (torch.rand(cin, lo, 4, 4, generator=g) * 2 - 1) / (cin * 4) ** 0.5
    b = torch.rand(lo, generator=g) - 0.5
    slopes = torch.rand(lo, generator=g) * 1.5 - 0.5      # per-channel PReLU slopes of either sign
    want = nhwc(F.prelu(F.conv_transpose2d(x.double(), wt.double(), b.double(), 2, 1), slopes.double()))
    xd = nhwc(x).cuda()
    hnd = lib.vfi_conv_create_ex(1, wt.data_ptr(), b.data_ptr(), lo, cin, 4, 2, 0, None, cin, slopes.data_ptr())
    assert hnd, "vfi_conv_create_ex failed"

    def run():
        out = torch.full(want.shape, float("nan"), device="cuda")
        _ck(lib.vfi_conv_forward_ex(hnd, ptr(xd), cin, h, w, ptr(out), lo, n, 3, 0.0, 0.0, 0.0, None, 0, None), "vfi_conv_forward_ex")
        return out

    try:
        (ref, rec0), (got, rec1) = _both(lib, run)
    finally:
        lib.vfi_conv_destroy(hnd)
    for rec in (rec0, rec1):
        # the Winograd kernel's transposed form with the per-channel PReLU epilogue (MODE 1, SHUF 2) where the object takes it
        assert (rec[0] == WINO) == reaches and (not reaches or (rec[1] == 8 and rec[2] == 1 and rec[3] == 2)), rec
    _assert_bound(ref, want, f"deconv+prelu LO {lo} @{h}x{w} wino_dead=0")
    _assert_bound(got, want, f"deconv+prelu LO {lo} @{h}x{w} wino_dead=1")
    assert torch.equal(got, ref), describe_diff(got, ref, "wino_dead 1 vs 0")
