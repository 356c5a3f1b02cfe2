"""Layer objects on images of 2 GiB and more (below 4 GiB): the LARGE instantiations of the second-generation direct kernel and of the
Winograd kernel (csrc/conv_mfma2.hip, conv_wino.hip), which rebase their buffer descriptors per tile / per region.

1. Forced, small.  The test option large_image_bytes = 1 makes every image "large", so small shapes run the LARGE code.  Same arithmetic
   in the same order, only the addressing differs: the result must equal the default path's bit for bit.  Data is small integers (every
   fp32 sum exact in any order), so both must also equal a float64 convolution on the host bit for bit.  The launch record says that the
   LARGE instantiation really ran (form 3 of the direct kernel, store 3 of the Winograd kernel).  NaN surroundings catch a stray access.
2. Real, over 2 GiB.  Small-integer data made on the device.  Bands of output rows (first, last, around the rows whose byte offset crosses
   2^31 in the input and in the output) are compared bit for bit with a float64 convolution of the cropped input on the host.  The chosen
   route has no seams of its own (every tile / region has its own descriptor), so EVERY row is checked besides: the image is cut into two
   overlapping halves below 2 GiB, the plain path runs on each, and rows away from the cut must equal the large call's bit for bit.

Exactness of the data: x in [-3, 3], weights in [-2, 2] (3x3 stride 1: 4 * [-1, 1], so that the Winograd transform G g G^T is integral),
bias and residual small integers: every partial sum is an integer below 2^24 in any order, in both kernels.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float("nan")
GEN1, GEN2, WINO = 1, 2, 3
LARGE_DEFAULT = 2 ** 31 - 1
TWO31 = 2 ** 31


def _ck(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


def _rec(lib):
    r = (C.c_int32 * 8)()
    assert lib.vfi_test_last_conv_launch(r, 8) == 8
    return list(r)


def _ints(g, shape, lo, hi, mul=1):
    return (torch.randint(lo, hi + 1, shape, generator=g) * mul).float()


def conv_f64(x, w, b, k, stride, top=True, bottom=True):
    """x [N,H,W,C], w OIHW, b: Conv2d(k, stride, pad = 1 for k 3 / 4, 0 for k 1) in float64, NHWC.  top / bottom False: the band's first /
    last row is not the image's, so no padding row is added there (the band carries the halo itself)."""
    p = 0 if k == 1 else 1
    xc = F.pad(x.double().permute(0, 3, 1, 2), (p, p, p if top else 0, p if bottom else 0))
    return F.conv2d(xc, w.double(), b.double(), stride=stride).permute(0, 2, 3, 1)


def epilogue(v, act, slope, res):
    if res is not None:
        v = v + res.double()
    return torch.where(v > 0, v, v * slope) if act == 1 else v


def is_large(rec):
    return (rec[0] == GEN2 and rec[2] == 3) or (rec[0] == WINO and rec[3] == 3)


# ---- 1. forced, small -----------------------------------------------------------------------------------------------------------------------

EPILOGUES = [(0, 0.0, False), (1, 0.0, False), (1, 0.25, False), (0, 0.0, True), (1, 0.0, True), (1, 0.25, True)]      # none, ReLU, leaky; residual


def _small_case(lib, k, stride, cin, cphys, cout, n, h, w, algo, family, variant=None, seed=0):
    g = torch.Generator().manual_seed(7000 + seed)
    wino_data = k == 3 and stride == 1
    wt = _ints(g, (cout, cin, k, k), -1, 1, 4) if wino_data else _ints(g, (cout, cin, k, k), -2, 2)
    b = _ints(g, (cout,), -3, 3)
    x = _ints(g, (n, h, w, cin), -3, 3)
    ho, wo = -(-h // stride), -(-w // stride)
    r = _ints(g, (n, ho, wo, cout), -4, 4)
    pre = conv_f64(x, wt, b, k, stride)
    assert float(pre.abs().max()) + 4 < 2 ** 24
    handle = lib.vfi_conv_create_ex(0, wt.data_ptr(), b.data_ptr(), cout, cin, k, stride, 0, None, cphys, None)
    assert handle, "vfi_conv_create_ex failed"
    name = f"conv{k}x{k}s{stride}_{cphys}to{cout}".encode()
    try:
        in_cs, out_cs, res_cs, off_i, off_o, off_r = 8 + cphys + 4, 3 + cout + 5, 2 + cout + 4, 8, 3, 2
        xin = torch.full((w + n * h * w + w, in_cs), NAN)
        win = torch.full((n * h * w, cphys), 12345.0)      # window positions beyond cin: finite, their weights are zero
        win[:, :cin] = x.reshape(-1, cin)
        xin[w:w + n * h * w, off_i:off_i + cphys] = win
        xd = xin.cuda()
        rin = torch.full((1 + n * ho * wo + 1, res_cs), NAN)
        rin[1:-1, off_r:off_r + cout] = r.reshape(-1, cout)
        rd = rin.cuda()
        lib.vfi_test_conv_algo(algo)
        if variant is not None:
            lib.vfi_test_variant_override(name + b"=" + str(variant).encode())
        for act, slope, res in EPILOGUES:
            want = epilogue(pre, act, slope, r if res else None).float()
            outs = []
            for mark in (LARGE_DEFAULT, 1):
                assert lib.vfi_test_set_option(b"large_image_bytes", mark) == 0
                out = torch.full((1 + n * ho * wo + 2, out_cs), NAN, device="cuda")
                _ck(lib.vfi_conv_forward_ex(handle, xd.data_ptr() + 4 * (w * in_cs + off_i), in_cs, h, w, out.data_ptr() + 4 * (out_cs + off_o), out_cs, n, act, slope,
                                            0.0, 0.0, rd.data_ptr() + 4 * (res_cs + off_r) if res else None, res_cs if res else 0, None), "forward_ex")
                torch.cuda.synchronize()
                rec = _rec(lib)
                what = f"{name.decode()} n{n} {h}x{w} algo {algo} act {act}/{slope} res {res} mark {mark}: launch {rec}"
                assert rec[0] == family, what
                assert variant is None or rec[1] == variant, what
                assert is_large(rec) == (mark == 1), what
                got = out.cpu()
                assert torch.isnan(got[0]).all() and torch.isnan(got[-2:]).all(), what + ": wrote a guard pixel"
                body = got[1:-2]
                assert torch.isnan(body[:, :off_o]).all() and torch.isnan(body[:, off_o + cout:]).all(), what + ": wrote a guard channel"
                val = body[:, off_o:off_o + cout].reshape(n, ho, wo, cout)
                assert not torch.isnan(val).any(), what + ": an output is NaN (unwritten, or a NaN was read)"
                assert torch.equal(val, want), what + f": {int((val != want).sum())} values differ from the float64 convolution"
                outs.append(val)
            assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    finally:
        lib.vfi_test_set_option(b"large_image_bytes", LARGE_DEFAULT)
        lib.vfi_test_variant_override(b"")
        lib.vfi_test_conv_algo(0)
        lib.vfi_conv_destroy(handle)


@pytest.mark.parametrize("algo,family", [(1, GEN2), (2, WINO)])
@pytest.mark.parametrize("h,w", [(2, 2), (5, 7), (18, 34), (40, 72)])
def test_forced_3x3_stride1(hip_lib, h, w, algo, family):
    _small_case(hip_lib, 3, 1, 132, 136, 64, 2, h, w, algo, family, seed=h)


@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("h,w", [(2, 2), (4, 6), (18, 34)])
def test_forced_stride2(hip_lib, k, h, w):
    _small_case(hip_lib, k, 2, 132, 136, 64, 2, h, w, 0, GEN2, seed=10 * k + h)


def test_forced_1x1(hip_lib):
    _small_case(hip_lib, 1, 1, 132, 136, 64, 2, 5, 7, 0, GEN2, seed=3)


# every tile of the direct kernel that has a LARGE instantiation, forced by trace name: (k, stride, Cin, window, Cout, variant)
LARGE_TILES = [(3, 1, 132, 136, 64, 32), (3, 1, 132, 136, 64, 34), (3, 1, 132, 136, 96, 35), (3, 1, 132, 136, 32, 45), (3, 1, 132, 136, 32, 61),
               (3, 2, 132, 136, 64, 39), (3, 2, 132, 136, 96, 41),
               (4, 2, 30, 32, 64, 46), (4, 2, 30, 32, 64, 47), (4, 2, 30, 32, 32, 51),
               (1, 1, 132, 136, 64, 48), (1, 1, 132, 136, 64, 49), (1, 1, 132, 136, 32, 50), (1, 1, 124, 128, 64, 55), (1, 1, 124, 128, 128, 56)]


@pytest.mark.parametrize("k,stride,cin,cphys,cout,variant", LARGE_TILES, ids=lambda v: str(v))
def test_forced_every_large_tile(hip_lib, k, stride, cin, cphys, cout, variant):
    _small_case(hip_lib, k, stride, cin, cphys, cout, 2, 18, 34, 1, GEN2, variant=variant, seed=variant)


# ---- 2. real, over 2 GiB ----------------------------------------------------------------------------------------------------------------------

def _bands(rows, crossings):
    """Output row ranges to compare on the host: the first 8, the last 8, and 8 rows on each side of every crossing row"""
    out = [(0, min(8, rows)), (max(rows - 8, 0), rows)]
    for c in crossings:
        if 0 <= c < rows:
            out.append((max(c - 8, 0), min(c + 9, rows)))
    return out


def _band_ref(xd, cin, wt, b, k, stride, r0, r1, act, slope):
    """Rows [r0, r1) of the layer's output from the cropped input, float64 on the host"""
    H = xd.shape[1]
    lo = r0 * stride - (0 if k == 1 else 1)
    hi = (r1 - 1) * stride + (k - 1 if k != 1 else 0) - (0 if k == 1 else 1) + 1      # one past the last input row the band reads
    top, bottom = lo < 0, hi > H
    crop = xd[:, max(lo, 0):min(hi, H), :, :cin].cpu()
    v = conv_f64(crop, wt, b, k, stride, top=top, bottom=bottom)
    assert v.shape[1] == r1 - r0, (v.shape, r0, r1)
    return epilogue(v, act, slope, None).float()


def _large_case(lib, k, stride, cin, cout, H, W, in_cs, out_cs, act, slope, algo, expect, seed, halves=True):
    """-> nothing; asserts.  expect: (family, large?) of the launch record."""
    g = torch.Generator().manual_seed(9000 + seed)
    wino_data = k == 3 and stride == 1
    wt = _ints(g, (cout, cin, k, k), -1, 1, 4) if wino_data else _ints(g, (cout, cin, k, k), -2, 2)
    b = _ints(g, (cout,), -3, 3)
    torch.manual_seed(seed)
    xd = torch.randint(-3, 4, (1, H, W, in_cs), device="cuda", dtype=torch.int8).float()      # every channel of the window's tensor: small integers
    ho, wo = H // stride, W // stride
    out = torch.full((1, ho, wo, out_cs), NAN, device="cuda")
    in_bytes, out_bytes = H * W * in_cs * 4, ho * wo * out_cs * 4
    handle = lib.vfi_conv_create_ex(0, wt.data_ptr(), b.data_ptr(), cout, cin, k, stride, 0, None, cin, None)
    assert handle
    try:
        lib.vfi_test_conv_algo(algo)
        _ck(lib.vfi_conv_forward_ex(handle, xd.data_ptr(), in_cs, H, W, out.data_ptr(), out_cs, 1, act, slope, 0.0, 0.0, None, 0, None), "forward_ex (large)")
        torch.cuda.synchronize()
        rec = _rec(lib)
        what = f"conv{k}x{k}s{stride} {cin}->{cout} {H}x{W} in_cs {in_cs} ({in_bytes} bytes) out_cs {out_cs} ({out_bytes} bytes) algo {algo}: launch {rec}"
        print(what)
        assert (rec[0], is_large(rec)) == expect, what
        # bands on the host
        cross = [(TWO31 // (W * in_cs * 4)) // stride]
        if out_bytes >= TWO31:
            cross.append(TWO31 // (wo * out_cs * 4))
        for r0, r1 in _bands(ho, cross):
            got = out[0, r0:r1].cpu()
            want = _band_ref(xd, cin, wt, b, k, stride, r0, r1, act, slope)
            assert torch.isnan(got[..., cout:]).all(), what + f": rows {r0}..{r1}: a channel beside the output window was written"
            assert torch.equal(got[..., :cout], want[0]), what + f": rows {r0}..{r1}: {int((got[..., :cout] != want[0]).sum())} values differ from the float64 convolution"
        # every row: the plain path on two overlapping halves below 2 GiB
        if halves:
            rows_half = ((LARGE_DEFAULT - 1) // (W * in_cs * 4)) // 2 * 2
            rows_half = min(rows_half, H // 2 + 40)
            assert 2 * rows_half - 16 >= H and rows_half * W * in_cs * 4 < LARGE_DEFAULT
            for first in (0, H - rows_half):
                sub = torch.full((1, rows_half // stride, wo, out_cs), NAN, device="cuda")
                _ck(lib.vfi_conv_forward_ex(handle, xd.data_ptr() + 4 * first * W * in_cs, in_cs, rows_half, W, sub.data_ptr(), out_cs, 1, act, slope, 0.0, 0.0, None, 0,
                                            None), "forward_ex (half)")
                torch.cuda.synchronize()
                assert not is_large(_rec(lib))
                # rows of the half whose taps stay inside it: all but the row at the cut
                a0, a1 = (0, rows_half // stride - 2) if first == 0 else (2, rows_half // stride)
                o0 = first // stride
                same = torch.equal(out[0, o0 + a0:o0 + a1, :, :cout].view(torch.int32), sub[0, a0:a1, :, :cout].view(torch.int32))
                assert same, what + f": rows {o0 + a0}..{o0 + a1} differ from the plain path on the sub-image that starts at row {first}"
                del sub
    finally:
        lib.vfi_test_conv_algo(0)
        lib.vfi_conv_destroy(handle)


@pytest.mark.parametrize("algo,expect", [(1, (GEN2, True)), (2, (WINO, True))])
def test_large_case_a_3x3_stride1(hip_lib, oracle_threads, algo, expect):
    """[1, 2176, 3840] with in_cs = out_cs = 80: every operand 2 673 868 800 bytes"""
    assert 2176 * 3840 * 80 * 4 == 2673868800
    _large_case(hip_lib, 3, 1, 16, 32, 2176, 3840, 80, 80, 1, 0.0, algo, expect, seed=1)


@pytest.mark.parametrize("cout,expect", [(32, (GEN1, False)), (64, (GEN2, True))])
def test_large_case_b_3x3_stride2(hip_lib, oracle_threads, cout, expect):
    """The same input, stride 2.  Cout 32 takes the first-generation tile s2_m1n1, as it always did: that kernel indexes floats, not bytes,
    had no 2 GiB guard and has no LARGE form; Cout 64 (XVFI's rec_ext_ds) takes the second-generation kernel, which refused this image."""
    _large_case(hip_lib, 3, 2, 16, cout, 2176, 3840, 80, 80, 1, 0.0, 0, expect, seed=2)


def test_large_case_c_4x4_stride2(hip_lib, oracle_threads):
    """The RefineUNet's first layer at scale 2: Cin 80 on [1, 2160, 3840]; input and space-to-depth image both over 2 GiB"""
    assert 2160 * 3840 * 80 * 4 > TWO31 and 1081 * 1921 * 320 * 4 > TWO31
    _large_case(hip_lib, 4, 2, 80, 64, 2160, 3840, 80, 64, 1, 0.0, 0, (GEN2, True), seed=3)


def test_large_case_d_near_the_top_and_the_refusal(hip_lib, oracle_threads):
    """[1, 2560, 4096] with in_cs = out_cs = 100: 4 194 304 000 bytes, 100 MB below 4 GiB; with a stride of 104 the image is over 4 GiB and
    the call is refused with the message it always had."""
    from cfi_amd import _lib

    assert 2560 * 4096 * 100 * 4 == 4194304000 and 2560 * 4096 * 104 * 4 == 4362076160
    _large_case(hip_lib, 3, 1, 16, 32, 2560, 4096, 100, 100, 1, 0.25, 0, (WINO, True), seed=4)
    torch.cuda.empty_cache()
    wt, b = torch.zeros(32, 16, 3, 3), torch.zeros(32)
    handle = hip_lib.vfi_conv_create_ex(0, wt.data_ptr(), b.data_ptr(), 32, 16, 3, 1, 0, None, 16, None)
    assert handle
    # buffers of the size the call claims: a refusal touches nothing, and a call that is not refused stays inside them
    xin, out = torch.zeros(2560 * 4096 * 104, device="cuda"), torch.zeros(2560 * 4096 * 104, device="cuda")
    try:
        for algo in (0, 1, 2):
            hip_lib.vfi_test_conv_algo(algo)
            rc = hip_lib.vfi_conv_forward_ex(handle, xin.data_ptr(), 104, 2560, 4096, out.data_ptr(), 104, 1, 1, 0.25, 0.0, 0.0, None, 0, None)
            assert rc != 0 and "image larger than 2 GiB" in _lib.last_error(), (algo, rc, _lib.last_error())
    finally:
        hip_lib.vfi_test_conv_algo(0)
        hip_lib.vfi_conv_destroy(handle)


def test_forms_without_a_large_instantiation_stay_refused(hip_lib):
    """Above 2 GiB the extended feature set of the second-generation kernel (here: sigmoid, replicate padding at stride 1 and 2) keeps its
    refusal, on either algorithm."""
    from cfi_amd import _lib

    # buffers of the size the call claims: a refusal touches nothing, and a call that is not refused stays inside them
    xin, out = torch.zeros(2176 * 3840 * 80, device="cuda"), torch.zeros(2176 * 3840 * 80, device="cuda")
    bias = torch.zeros(64)
    for k, stride, pad, act in ((3, 1, 0, 4), (3, 1, 1, 1), (3, 2, 1, 0)):
        wt = torch.zeros(64, 16, k, k)
        handle = hip_lib.vfi_conv_create_ex(0, wt.data_ptr(), bias.data_ptr(), 64, 16, k, stride, pad, None, 16, None)
        assert handle
        try:
            for algo in (0, 1, 2):
                hip_lib.vfi_test_conv_algo(algo)
                rc = hip_lib.vfi_conv_forward_ex(handle, xin.data_ptr(), 80, 2176, 3840, out.data_ptr(), 80, 1, act, 0.0, 0.0, 0.0, None, 0, None)
                assert rc != 0 and "larger than 2 GiB" in _lib.last_error(), (k, stride, pad, act, algo, rc, _lib.last_error())
        finally:
            hip_lib.vfi_test_conv_algo(0)
            hip_lib.vfi_conv_destroy(handle)
