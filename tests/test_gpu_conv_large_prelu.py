"""Layer objects with a per-channel PReLU epilogue (act 3) on images of 2 GiB and more (below 4 GiB): the LARGE instantiations that ATM's
full-resolution layers take — the Winograd kernel's hot PReLU epilogue (MODE 1, 16x8 regions) and the second-generation direct kernel's
3x3 stride-1, 3x3 stride-2 and 1x1 tiles with act 3 as their only extended feature (csrc/conv_wino.hip, conv_mfma2.hip).

1. Forced, small.  The test option large_image_bytes = 1 makes every image "large".  Each new instantiation is compared with its plain twin
   bit for bit over the WHOLE output buffer, NaN guard pixels and guard channels included, and both with a float64 convolution of
   small-integer data, which is exact in fp32.  The launch record must name the LARGE form under the option (on the code before these
   forms existed it names the plain one).  Shapes: 37x45 (odd, no multiple of a tile or region, several workgroups with N = 2) and 16x24;
   the layer shapes are ATM's: Cin 76 in an 80-float pixel, an output window at offset 64 of a 128-float pixel, stride 2 out of such a window,
   1x1; slopes of both signs and zero.
2. At size, one call per layer shape of the table in docs/design/atm.md ("4K"), ATM-base's and ATM-lite's at 2176x3840.  Small-integer data
   made on the device.  Bands of output rows (first, last, around the rows whose byte offset crosses 2^31 in the input and in the output)
   are compared bit for bit with a float64 convolution of the cropped input on the host; every row is compared with the plain path on
   overlapping sub-images below 2 GiB (rows away from the cuts).
3. Refusals kept above 2 GiB: sigmoid, replicate padding, residual + PReLU.

Exactness of the data: x in [-3, 3], weights in [-2, 2] (3x3 stride 1: 4 * [-1, 1], so that the Winograd transform G g G^T is integral), bias
small integers: every partial sum is an integer far below 2^24 in any order (at most 9 * 128 * 3 * 4 + 3 = 13 827).  The slopes are taken
from {-2, -1, -0.5, 0, 0.25, 0.5, 1, 2}: v * slope is exact as well.
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
SLOPES = [-2.0, -1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 2.0]


def _ck(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


def _rec(lib):
    r = (C.c_int32 * 8)()
    assert lib.vfi_test_last_conv_launch(r, 8) == 8
    return list(r)


def _ints(g, shape, lo, hi, mul=1):
    return (torch.randint(lo, hi + 1, shape, generator=g) * mul).float()


def _slopes(g, cout):
    """Every slope of SLOPES in turn, shuffled: both signs and zero occur from 8 channels on"""
    s = torch.tensor([SLOPES[i % len(SLOPES)] for i in range(cout)])
    return s[torch.randperm(cout, generator=g)].contiguous()


def conv_f64(x, w, b, k, stride, top=True, bottom=True):
    """x [N,H,W,C], w OIHW, b: Conv2d(k, stride, pad = 1 for k 3, 0 for k 1) in float64, NHWC.  top / bottom False: the band's first / last
    row is not the image's, so no padding row is added there (the band carries the halo itself)."""
    p = 0 if k == 1 else 1
    xc = F.pad(x.double().permute(0, 3, 1, 2), (p, p, p if top else 0, p if bottom else 0))
    return F.conv2d(xc, w.double(), b.double(), stride=stride).permute(0, 2, 3, 1)


def epilogue(v, act, slopes):
    return torch.where(v > 0, v, v * slopes.double()) if act == 3 else v


def is_large(rec):
    return (rec[0] == GEN2 and rec[2] == 3) or (rec[0] == WINO and rec[3] == 3)


# ---- 1. forced, small -----------------------------------------------------------------------------------------------------------------------

def _small_case(lib, k, stride, cin, cphys, in_cs, off_i, cout, out_cs, off_o, n, h, w, algo, family, variant=None, wino_mode=None, seed=0):
    g = torch.Generator().manual_seed(11000 + seed)
    wino_data = k == 3 and stride == 1
    wt = _ints(g, (cout, cin, k, k), -1, 1, 4) if wino_data else _ints(g, (cout, cin, k, k), -2, 2)
    b = _ints(g, (cout,), -3, 3)
    sl = _slopes(g, cout)
    x = _ints(g, (n, h, w, cin), -3, 3)
    ho, wo = -(-h // stride), -(-w // stride)
    pre = conv_f64(x, wt, b, k, stride)
    assert float(pre.abs().max()) * 2 < 2 ** 24
    want = epilogue(pre, 3, sl).float()
    assert (want < 0).any() and (want > 0).any()
    handle = lib.vfi_conv_create_ex(0, wt.data_ptr(), b.data_ptr(), cout, cin, k, stride, 0, None, cphys, sl.data_ptr())
    assert handle, "vfi_conv_create_ex failed"
    name = f"conv{k}x{k}s{stride}_{cphys}to{cout}".encode()
    try:
        if stride == 2 and (h % 2 or w % 2):
            _ck(lib.vfi_conv_accept_odd(handle, 1), "accept_odd")
        assert off_i + cphys <= in_cs and off_o + cout <= out_cs
        xin = torch.full((w + n * h * w + w, in_cs), NAN)
        win = torch.full((n * h * w, cphys), 12345.0)      # window positions beyond cin: finite, their weights are zero
        win[:, :cin] = x.reshape(-1, cin)
        xin[w:w + n * h * w, off_i:off_i + cphys] = win
        xd = xin.cuda()
        lib.vfi_test_conv_algo(algo)
        if variant is not None:
            lib.vfi_test_variant_override(name + b"=" + str(variant).encode())
        outs, recs = [], []
        for mark in (LARGE_DEFAULT, 1):
            assert lib.vfi_test_set_option(b"large_image_bytes", mark) == 0
            out = torch.full((1 + n * ho * wo + 2, out_cs), NAN, device="cuda")
            _ck(lib.vfi_conv_forward_ex(handle, xd.data_ptr() + 4 * (w * in_cs + off_i), in_cs, h, w, out.data_ptr() + 4 * (out_cs + off_o), out_cs, n, 3, 0.0,
                                        0.0, 0.0, None, 0, None), "forward_ex")
            torch.cuda.synchronize()
            rec = _rec(lib)
            what = f"{name.decode()} n{n} {h}x{w} in {off_i}+{cphys}/{in_cs} out {off_o}+{cout}/{out_cs} algo {algo} mark {mark}: launch {rec}"
            assert rec[0] == family, what
            assert variant is None or rec[1] == variant, what
            assert wino_mode is None or rec[2] == wino_mode, what
            assert is_large(rec) == (mark == 1), what + ": the LARGE form is taken under large_image_bytes = 1, and only then"
            got = out.cpu()
            assert torch.isnan(got[0]).all() and torch.isnan(got[-2:]).all(), what + ": wrote a guard pixel"
            body = got[1:-2]
            assert torch.isnan(body[:, :off_o]).all() and torch.isnan(body[:, off_o + cout:]).all(), what + ": wrote a guard channel"
            val = body[:, off_o:off_o + cout].reshape(n, ho, wo, cout)
            assert not torch.isnan(val).any(), what + ": an output is NaN (unwritten, or a NaN was read)"
            assert torch.equal(val, want), what + f": {int((val != want).sum())} values differ from the float64 convolution"
            outs.append(got)
            recs.append(rec)
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "the LARGE form and its plain twin differ in some bit of the buffer"
        return recs
    finally:
        lib.vfi_test_set_option(b"large_image_bytes", LARGE_DEFAULT)
        lib.vfi_test_variant_override(b"")
        lib.vfi_test_conv_algo(0)
        lib.vfi_conv_destroy(handle)


SHAPES = [(37, 45), (16, 24)]


@pytest.mark.parametrize("algo,family,mode", [(1, GEN2, None), (2, WINO, 1)])
@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("h,w", SHAPES)
def test_forced_proj_cin76_of_80_into_a_window_at_64_of_128(hip_lib, h, w, cout, algo, family, mode):
    """ATM's proj: 3x3 + PReLU, 76 channels in an 80-float pixel, written into the window at +64 of the 128-float concat pixel.  Both kernels.
    (32 output channels on the direct kernel: tile d1_m2n1, 45, which such a layer gets at full resolution, is forced by name — at these
    small sizes the automatic choice is a first-generation tile, which indexes floats and has no LARGE form.)"""
    variant = 45 if (algo == 1 and cout == 32) else None
    _small_case(hip_lib, 3, 1, 76, 80, 80, 0, cout, 128, 64, 2, h, w, algo, family, variant=variant, wino_mode=mode, seed=h + cout + algo)


@pytest.mark.parametrize("h,w", SHAPES)
def test_forced_stride2_out_of_a_window_at_64_of_128(hip_lib, h, w):
    """ATM-base's down1: 3x3 stride 2 + PReLU reading the window at +64 of the 128-float pixel; tile d2_m1n2 (39), which has a LARGE form"""
    _small_case(hip_lib, 3, 2, 64, 64, 128, 64, 64, 256, 0, 2, h, w, 0, GEN2, seed=200 + h)


@pytest.mark.parametrize("h,w", SHAPES)
def test_forced_1x1(hip_lib, h, w):
    """The transposed convolutions' 1x1 form: 4 * Cout taps + PReLU"""
    _small_case(hip_lib, 1, 1, 117, 120, 120, 0, 244, 248, 0, 2, h, w, 0, GEN2, seed=300 + h)


def test_forced_stride2_tile_choice(hip_lib):
    """A stride-2 act 3 layer is handed a tile that has a LARGE form: 39 for 64 output channels, 41 for 96"""
    for cout, tile in ((64, 39), (96, 41)):
        _small_case(hip_lib, 3, 2, 64, 64, 128, 64, cout, 128, 8, 2, 16, 24, 0, GEN2, seed=400 + cout)
        # (the record's variant id is checked by forcing nothing: the automatic choice must already be the tile)
        g = torch.Generator().manual_seed(1)
        wt, b, sl = _ints(g, (cout, 64, 3, 3), -2, 2), _ints(g, (cout,), -3, 3), _slopes(g, cout)
        handle = hip_lib.vfi_conv_create_ex(0, wt.data_ptr(), b.data_ptr(), cout, 64, 3, 2, 0, None, 64, sl.data_ptr())
        assert handle
        try:
            assert hip_lib.vfi_test_set_option(b"large_image_bytes", 1) == 0
            x, out = torch.zeros(16 * 24 * 128, device="cuda"), torch.zeros(8 * 12 * cout, device="cuda")
            _ck(hip_lib.vfi_conv_forward_ex(handle, x.data_ptr() + 256, 128, 16, 24, out.data_ptr(), cout, 1, 3, 0.0, 0.0, 0.0, None, 0, None), "forward_ex")
            torch.cuda.synchronize()
            rec = _rec(hip_lib)
            assert rec[0] == GEN2 and rec[1] == tile and rec[2] == 3, rec
        finally:
            hip_lib.vfi_test_set_option(b"large_image_bytes", LARGE_DEFAULT)
            hip_lib.vfi_conv_destroy(handle)


# every tile of the direct kernel that has a LARGE x PReLU instantiation, forced by trace name: (k, stride, Cin, window, Cout, variant)
PRELU_TILES = [(3, 1, 132, 136, 64, 32), (3, 1, 132, 136, 64, 34), (3, 1, 132, 136, 96, 35), (3, 1, 132, 136, 32, 45), (3, 1, 132, 136, 32, 61),
               (3, 2, 132, 136, 64, 39), (3, 2, 132, 136, 96, 41),
               (1, 1, 132, 136, 64, 48), (1, 1, 132, 136, 64, 49), (1, 1, 132, 136, 32, 50), (1, 1, 124, 128, 64, 55), (1, 1, 124, 128, 128, 56)]


@pytest.mark.parametrize("k,stride,cin,cphys,cout,variant", PRELU_TILES, ids=lambda v: str(v))
def test_forced_every_large_prelu_tile(hip_lib, k, stride, cin, cphys, cout, variant):
    _small_case(hip_lib, k, stride, cin, cphys, cphys + 12, 8, cout, cout + 8, 3, 2, 37, 45, 1, GEN2, variant=variant, seed=variant)


@pytest.mark.parametrize("cout,variant", [(32, 61), (64, 34)])
def test_forced_split_k_is_the_plain_twins(hip_lib, cout, variant):
    """Few tiles and a long K loop: the launch is cut along K, and the cut sets the summation order.  The LARGE form has other register
    counts than its plain twin (tile d1_m1n1: 4 resident workgroups against 3) and must still cut where the twin cuts.  The data is exact
    in any order, so the launch records are compared: the same number of slices, more than one."""
    plain, large = _small_case(hip_lib, 3, 1, 288, 288, 288, 0, cout, cout, 0, 1, 16, 24, 1, GEN2, variant=variant, seed=500 + variant)
    assert plain[4] > 1 and plain[4] == large[4], (plain, large)


# ---- 2. at size -------------------------------------------------------------------------------------------------------------------------------

def _bands(rows, crossings):
    """Output row ranges to compare on the host: the first 8, the last 8, and 8 rows on each side of every crossing row"""
    out = [(0, min(8, rows)), (max(rows - 8, 0), rows)]
    for c in crossings:
        if 0 <= c < rows:
            out.append((max(c - 8, 0), min(c + 9, rows)))
    return out


def _band_ref(xd, off_i, cin, wt, b, sl, k, stride, r0, r1, act):
    """Rows [r0, r1) of the layer's output from the cropped input, float64 on the host"""
    H = xd.shape[1]
    p = 0 if k == 1 else 1
    lo = r0 * stride - p
    hi = (r1 - 1) * stride + (k - 1) - p + 1      # one past the last input row the band reads
    top, bottom = lo < 0, hi > H
    crop = xd[:, max(lo, 0):min(hi, H), :, off_i:off_i + cin].cpu()
    v = conv_f64(crop, wt, b, k, stride, top=top, bottom=bottom)
    assert v.shape[1] == r1 - r0, (v.shape, r0, r1)
    return epilogue(v, act, sl).float()


def _at_size(lib, k, stride, cin, cout, H, W, in_cs, off_i, out_cs, off_o, act, algo, expect, seed):
    """-> nothing; asserts.  expect: (family, large?) of the launch record."""
    g = torch.Generator().manual_seed(13000 + seed)
    wino_data = k == 3 and stride == 1
    wt = _ints(g, (cout, cin, k, k), -1, 1, 4) if wino_data else _ints(g, (cout, cin, k, k), -2, 2)
    b = _ints(g, (cout,), -3, 3)
    sl = _slopes(g, cout)
    torch.manual_seed(seed)
    xd = torch.randint(-3, 4, (1, H, W, in_cs), device="cuda", dtype=torch.int8).float()      # every channel of the pixel: small integers
    ho, wo = H // stride, W // stride
    out = torch.full((1, ho, wo, out_cs), NAN, device="cuda")
    in_bytes, out_bytes = H * W * in_cs * 4, ho * wo * out_cs * 4
    handle = lib.vfi_conv_create_ex(0, wt.data_ptr(), b.data_ptr(), cout, cin, k, stride, 0, None, (cin + 7) // 8 * 8, sl.data_ptr())
    assert handle
    try:
        lib.vfi_test_conv_algo(algo)
        _ck(lib.vfi_conv_forward_ex(handle, xd.data_ptr() + 4 * off_i, in_cs, H, W, out.data_ptr() + 4 * off_o, out_cs, 1, act, 0.0, 0.0, 0.0, None, 0, None),
            "forward_ex (at size)")
        torch.cuda.synchronize()
        rec = _rec(lib)
        what = (f"conv{k}x{k}s{stride} {cin}->{cout} act {act} {H}x{W} in {off_i}+/{in_cs} ({in_bytes} bytes) out {off_o}+/{out_cs} ({out_bytes} bytes) "
                f"algo {algo}: launch {rec}")
        print(what)
        assert (rec[0], is_large(rec)) == expect, what
        # bands on the host
        cross = []
        if in_bytes >= TWO31:
            cross.append((TWO31 // (W * in_cs * 4)) // stride)
        if out_bytes >= TWO31:
            cross.append(TWO31 // (wo * out_cs * 4))
        assert cross, "no operand reaches 2^31 bytes: not a case for this test"
        for r0, r1 in _bands(ho, cross):
            got = out[0, r0:r1].cpu()
            want = _band_ref(xd, off_i, cin, wt, b, sl, k, stride, r0, r1, act)
            assert torch.isnan(got[..., :off_o]).all() and torch.isnan(got[..., off_o + cout:]).all(), what + f": rows {r0}..{r1}: a channel beside the output window was written"
            diff = int((got[..., off_o:off_o + cout] != want[0]).sum())
            assert diff == 0, what + f": rows {r0}..{r1}: {diff} values differ from the float64 convolution"
        # every row: the plain path on overlapping sub-images whose operands stay below 2 GiB
        row_bytes = max(W * in_cs * 4, (wo * out_cs * 4 + stride - 1) // stride)
        rows_sub = ((LARGE_DEFAULT - 1) // row_bytes) // 4 * 4
        n_sub = -(-(H - 16) // (rows_sub - 16))
        starts = [min(i * (rows_sub - 16), H - rows_sub) // 2 * 2 for i in range(n_sub)]
        assert starts[0] == 0 and starts[-1] + rows_sub == H and all(b_ - a_ <= rows_sub - 16 for a_, b_ in zip(starts, starts[1:])), (starts, rows_sub, H)
        for first in starts:
            sub = torch.full((1, rows_sub // stride, wo, out_cs), NAN, device="cuda")
            _ck(lib.vfi_conv_forward_ex(handle, xd.data_ptr() + 4 * (first * W * in_cs + off_i), in_cs, rows_sub, W, sub.data_ptr() + 4 * off_o, out_cs, 1, act, 0.0,
                                        0.0, 0.0, None, 0, None), "forward_ex (sub-image)")
            torch.cuda.synchronize()
            assert not is_large(_rec(lib)), what + ": the sub-image took a LARGE form"
            # rows of the sub-image whose taps stay inside it: all but two at a cut
            a0 = 0 if first == 0 else 2
            a1 = rows_sub // stride - (0 if first + rows_sub == H else 2)
            o0 = first // stride
            same = torch.equal(out[0, o0 + a0:o0 + a1, :, off_o:off_o + cout].view(torch.int32), sub[0, a0:a1, :, off_o:off_o + cout].view(torch.int32))
            assert same, what + f": rows {o0 + a0}..{o0 + a1} differ from the plain path on the sub-image that starts at row {first}"
            del sub
    finally:
        lib.vfi_test_conv_algo(0)
        lib.vfi_conv_destroy(handle)
        del xd, out
        torch.cuda.empty_cache()


HP, WP = 2176, 3840      # 2160x3840 padded to multiples of 64


def test_at_size_proj_lite(hip_lib, oracle_threads):
    """ref_in (80 floats, 2.67 GB) -> rf_c6's window at +32 of 64 floats: Winograd MODE 1, LARGE"""
    assert HP * WP * 80 * 4 == 2673868800
    _at_size(hip_lib, 3, 1, 76, 32, HP, WP, 80, 0, 64, 32, 3, 0, (WINO, True), seed=1)


def test_at_size_proj_base(hip_lib, oracle_threads):
    """ref_in (120 floats, 4.01 GB) -> rf_c6's window at +64 of 128 floats (4.28 GB): both operands cross 2^31"""
    assert HP * WP * 120 * 4 == 4010803200 and HP * WP * 128 * 4 == 4278190080
    _at_size(hip_lib, 3, 1, 116, 64, HP, WP, 120, 0, 128, 64, 3, 0, (WINO, True), seed=2)


def test_at_size_proj_base_direct_kernel(hip_lib, oracle_threads):
    """The same layer on the direct kernel's LARGE x PReLU form (algorithm choice 1)"""
    _at_size(hip_lib, 3, 1, 116, 64, HP, WP, 120, 0, 128, 64, 3, 1, (GEN2, True), seed=3)


def test_at_size_down1_base(hip_lib, oracle_threads):
    """rf_c6's window at +64 of 128 floats (4.28 GB) -> rf_c2 (256 floats at half resolution): 3x3 stride 2 + PReLU, tile 39"""
    _at_size(hip_lib, 3, 2, 64, 64, HP, WP, 128, 64, 256, 0, 3, 0, (GEN2, True), seed=4)


def test_at_size_rh0_base(hip_lib, oracle_threads):
    """rf_c6 (128 floats, 4.28 GB) -> rf_h (64 floats)"""
    _at_size(hip_lib, 3, 1, 128, 64, HP, WP, 128, 0, 64, 0, 3, 0, (WINO, True), seed=5)


def test_at_size_up2_c1_base(hip_lib, oracle_threads):
    """up_d2 -> up_c2 (104 floats, 3.48 GB each), 101 channels + PReLU"""
    assert HP * WP * 104 * 4 == 3476029440
    _at_size(hip_lib, 3, 1, 101, 101, HP, WP, 104, 0, 104, 0, 3, 0, (WINO, True), seed=6)


def test_at_size_up2_c2_base(hip_lib, oracle_threads):
    """up_c2 (104 floats) -> ref_in (120 floats, 4.01 GB), no activation: the LARGE form that existed, on ATM's shape"""
    _at_size(hip_lib, 3, 1, 101, 101, HP, WP, 104, 0, 120, 0, 0, 0, (WINO, True), seed=7)


def test_at_size_up2_de_base(hip_lib, oracle_threads):
    """up_pre2 (200 floats at half resolution, 1.67 GB) -> the level-2 taps (408 floats, 3.41 GB): 1x1 + PReLU with a small input and a large
    output.  The direct kernel stores through 64-bit addresses in every form, so this launch keeps the plain form it always had."""
    assert (HP // 2) * (WP // 2) * 408 * 4 == 3409182720
    _at_size(hip_lib, 1, 1, 197, 404, HP // 2, WP // 2, 200, 0, 408, 0, 3, 0, (GEN2, False), seed=8)


def test_at_size_1x1_prelu_large_input(hip_lib, oracle_threads):
    """No ATM layer has it, the form exists: 1x1 + PReLU reading a 4.28 GB image"""
    _at_size(hip_lib, 1, 1, 128, 32, HP, WP, 128, 0, 32, 0, 3, 0, (GEN2, True), seed=9)


# ---- 3. refusals kept ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_kept_above_2_gib(hip_lib):
    """Sigmoid, replicate padding and residual + PReLU have no LARGE form: above 2 GiB each keeps the refusal it always had, on either algorithm."""
    from cfi_amd import _lib

    # buffers of the size the call claims: a refusal touches nothing, and a call that is not refused stays inside them
    xin, out = torch.zeros(HP * WP * 80, device="cuda"), torch.zeros(HP * WP * 80, device="cuda")
    bias, sl = torch.zeros(64), torch.full((64,), 0.25)
    for pad, act, res in ((0, 4, False), (1, 3, False), (0, 3, True)):
        wt = torch.zeros(64, 16, 3, 3)
        handle = hip_lib.vfi_conv_create_ex(0, wt.data_ptr(), bias.data_ptr(), 64, 16, 3, 1, pad, None, 16, sl.data_ptr())
        assert handle
        try:
            for algo in (0, 1, 2):
                hip_lib.vfi_test_conv_algo(algo)
                rc = hip_lib.vfi_conv_forward_ex(handle, xin.data_ptr(), 80, HP, WP, out.data_ptr(), 80, 1, act, 0.0, 0.0, 0.0, out.data_ptr() if res else None,
                                                 80 if res else 0, None)
                assert rc != 0 and "larger than 2 GiB" in _lib.last_error(), (pad, act, res, algo, rc, _lib.last_error())
        finally:
            hip_lib.vfi_test_conv_algo(0)
            hip_lib.vfi_conv_destroy(handle)
