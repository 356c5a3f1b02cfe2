"""The large form of a layer object's transposed convolution: conv_wino_kernel<8, 0, 2, 0, LARGE> (csrc/conv_wino.hip), ConvTranspose2d(4, 2, 1)
as one 3x3 Winograd layer whose four parity groups are interleaved into [2 Hin, 2 Win] through per-region buffer descriptors.

1. Forced, small.  large_image_bytes = 1 makes every image "large": the smallest inputs the Winograd transposed form takes at all (128x128,
   and 131x133 for partial regions) run the large form and must equal the plain twin bit for bit over the whole buffer, NaN guards
   included, and a float64 transposed convolution bit for bit.  The launch record names the form (store 5 under the mark, store 2 without),
   and the permission vfi_conv_allow_huge alone changes no launch.
2. Real size.  FLAVR's dec[2] and dec[4] at 2160x3840 (docs/design/flavr.md), one time slice each: bands of output rows around every
   multiple of 2^31 bytes of the input and of the output against float64 on the host; every output row against the plain path on
   overlapping sub-images below 2 GiB (interior rows: a sub-image's zero border is not the image's).
3. Refusals: dec[4] without the permission, per-channel PReLU above the mark, an output over 2^31 - 1 floats with the permission.

Exactness of the data (the scheme of tests/test_gpu_conv_large.py): x in [-3, 3], weights 4 * [-1, 1] (so that G g G^T of the 3x3 embedding
is integral), integer bias: every partial sum in any order is an integer below 768 * 4 * 12 + 3 < 2^24.  LeakyReLU 0.2 rounds once, the
same product in every form and in float64 -> float32.
"""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_large import LARGE_DEFAULT, NAN, TWO31, WINO, _ck, _ints, _rec

pytestmark = pytest.mark.gpu

STORE_PLAIN, STORE_LARGE = 2, 5      # the launch record's store field: SHUF 2, and its large form (docs/design/conv_coverage.md)


def deconv_f64(x, w, b):
    """x [N,H,W,Cin], w [Cin,Cout,4,4]: ConvTranspose2d(4, 2, 1) in float64 -> [N,2H,2W,Cout]"""
    return F.conv_transpose2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=2, padding=1).permute(0, 2, 3, 1)


def lrelu(v, act, slope):
    """float64 v (integers); the slope is the kernel's float32 one, so v * slope is exact in float64 and rounds to float32 once, as v * slope does there"""
    return torch.where(v > 0, v, v * float(torch.tensor(slope, dtype=torch.float32))) if act == 1 else v


def _weights(g, cin, cout):
    return _ints(g, (cin, cout, 4, 4), -1, 1, 4), _ints(g, (cout,), -3, 3)


# ---- 1. forced, small -----------------------------------------------------------------------------------------------------------------------

# (h, w, cin, input layout (floats per pixel, window offset), cout, output layout (floats per pixel, window offset), n, act, slope)
# input layouts: a window at offset 8 of a wider pixel; FLAVR's [., ., 6, C] with the window at slice t = 2 (C = cin) and, for cin 24,
# the real three-slice window of C = 8 at slice 1.  Output layouts: offset 64 of a 384-float pixel (e2[1], slice 0 + 1), offset 64 t of a
# 256-float pixel (fin, t = 2).
SMALL = [
    (128, 128, 8, (8 + 8 + 4, 8), 24, (384, 64), 1, 0, 0.0),
    (128, 128, 16, (6 * 16, 32), 64, (256, 128), 2, 1, 0.2),
    (131, 133, 8, (6 * 8, 16), 64, (384, 64), 2, 0, 0.0),
    (131, 133, 16, (8 + 16 + 4, 8), 24, (256, 128), 1, 1, 0.2),
    (131, 133, 24, (6 * 8, 8), 64, (256, 128), 1, 0, 0.0),
    (128, 128, 16, (8 + 16 + 4, 8), 24, (384, 64), 2, 1, 0.2),
    (131, 133, 8, (8 + 8 + 4, 8), 24, (256, 128), 2, 0, 0.0),
    (128, 128, 8, (6 * 8, 16), 64, (384, 64), 1, 1, 0.2),
]


@pytest.mark.parametrize("h,w,cin,inl,cout,outl,n,act,slope", SMALL, ids=lambda v: str(v).replace(" ", ""))
def test_forced_large_form_is_the_plain_twin(hip_lib, h, w, cin, inl, cout, outl, n, act, slope):
    lib = hip_lib
    g = torch.Generator().manual_seed(100 * h + cin + cout + n)
    wt, b = _weights(g, cin, cout)
    x = _ints(g, (n, h, w, cin), -3, 3)
    want = lrelu(deconv_f64(x, wt, b), act, slope).float()
    assert float(want.abs().max()) < 2 ** 24
    (in_cs, off_i), (out_cs, off_o) = inl, outl
    handle = lib.vfi_conv_create_ex(1, wt.data_ptr(), b.data_ptr(), cout, cin, 4, 2, 0, None, cin, None)
    assert handle, "vfi_conv_create_ex failed"
    try:
        xin = torch.full((w + n * h * w + w, in_cs), NAN)
        xin[w:w + n * h * w, off_i:off_i + cin] = x.reshape(-1, cin)
        xd = xin.cuda()
        npix = n * 4 * h * w
        runs = []
        for mark, huge in ((LARGE_DEFAULT, 0), (LARGE_DEFAULT, 1), (1, 0), (1, 1)):
            assert lib.vfi_test_set_option(b"large_image_bytes", mark) == 0
            assert lib.vfi_conv_allow_huge(handle, huge) == 0
            out = torch.full((2 + npix + 3, out_cs), NAN, device="cuda")
            _ck(lib.vfi_conv_forward_ex(handle, xd.data_ptr() + 4 * (w * in_cs + off_i), in_cs, h, w, out.data_ptr() + 4 * (2 * out_cs + off_o), out_cs, n, act, slope,
                                        0.0, 0.0, None, 0, None), "forward_ex")
            torch.cuda.synchronize()
            rec = _rec(lib)
            what = f"deconv {cin}->{cout} n{n} {h}x{w} in {inl} out {outl} act {act}/{slope} mark {mark} huge {huge}: launch {rec}"
            assert rec[0] == WINO and rec[1] == 8 and rec[2] == 0, what
            assert rec[3] == (STORE_LARGE if mark == 1 else STORE_PLAIN), what      # the permission alone changes no launch
            got = out.cpu()
            assert torch.isnan(got[:2]).all() and torch.isnan(got[-3:]).all(), what + ": wrote a guard pixel"
            body = got[2:-3]
            assert torch.isnan(body[:, :off_o]).all() and torch.isnan(body[:, off_o + cout:]).all(), what + ": wrote a guard channel"
            val = body[:, off_o:off_o + cout].reshape(n, 2 * h, 2 * w, cout)
            assert not torch.isnan(val).any(), what + ": an output is NaN (unwritten, or a NaN was read)"
            assert torch.equal(val, want), what + f": {int((val != want).sum())} values differ from the float64 transposed convolution"
            runs.append((rec, got.view(torch.int32)))
        for rec, bits in runs[1:]:
            assert torch.equal(bits, runs[0][1]), "the whole buffer differs from the plain form's"
        assert runs[0][0][:7] == runs[1][0][:7] and runs[2][0][:7] == runs[3][0][:7], "the permission changed a launch"
    finally:
        lib.vfi_test_set_option(b"large_image_bytes", LARGE_DEFAULT)
        lib.vfi_conv_destroy(handle)


# ---- 2. real size ---------------------------------------------------------------------------------------------------------------------------

def _bands(rows, crossings, half=4):
    out = [(0, min(2 * half, rows)), (max(rows - 2 * half, 0), rows)]
    for c in crossings:
        if 0 <= c < rows:
            out.append((max(c - half, 0), min(c + half, rows)))
    return out


def _band_ref(xd, off_i, cin, wt, b, r0, r1, act, slope):
    """Output rows [r0, r1) in float64 on the host from the cropped input: output row r reads input rows (r + 1) // 2 - 1 and (r + 1) // 2"""
    H = xd.shape[1]
    lo, hi = max((r0 - 1) // 2, 0), min(r1 // 2 + 1, H)
    crop = xd[:, lo:hi, :, off_i:off_i + cin].cpu()
    v = deconv_f64(crop, wt, b)[:, r0 - 2 * lo:r1 - 2 * lo]
    assert v.shape[1] == r1 - r0
    return lrelu(v, act, slope).float()


def _real_case(lib, H, W, in_cs, off_i, cin, cout, out_cs, off_o, sub_rows, huge, seed):
    g = torch.Generator().manual_seed(9100 + seed)
    wt, b = _weights(g, cin, cout)
    act, slope = 0, 0.0      # FLAVR's
    torch.manual_seed(seed)
    xd = torch.randint(-3, 4, (1, H, W, in_cs), device="cuda", dtype=torch.int8).float()
    out = torch.full((1, 2 * H, 2 * W, out_cs), NAN, device="cuda")
    in_bytes, out_bytes = H * W * in_cs * 4, 4 * H * W * out_cs * 4
    assert max(in_bytes, out_bytes) >= TWO31 and (huge == (max(in_bytes, out_bytes) >= 2 * TWO31))
    handle = lib.vfi_conv_create_ex(1, wt.data_ptr(), b.data_ptr(), cout, cin, 4, 2, 0, None, cin, None)
    assert handle
    try:
        assert lib.vfi_conv_allow_huge(handle, int(huge)) == 0
        _ck(lib.vfi_conv_forward_ex(handle, xd.data_ptr() + 4 * off_i, in_cs, H, W, out.data_ptr() + 4 * off_o, out_cs, 1, act, slope, 0.0, 0.0, None, 0, None),
            "forward_ex (large)")
        torch.cuda.synchronize()
        rec = _rec(lib)
        what = f"deconv {cin}->{cout} {H}x{W} in_cs {in_cs} ({in_bytes} bytes) out_cs {out_cs} ({out_bytes} bytes): launch {rec}"
        print(what)
        assert rec[0] == WINO and rec[2] == 0 and rec[3] == STORE_LARGE, what
        # NaN everywhere outside the output window
        assert torch.isnan(out[..., :off_o]).all() and torch.isnan(out[..., off_o + cout:]).all(), what + ": a channel beside the output window was written"
        assert not torch.isnan(out[..., off_o:off_o + cout]).any(), what + ": an output is NaN"
        # bands around every multiple of 2^31 bytes of the input (as output rows) and of the output
        cross = [2 * (k * TWO31 // (W * in_cs * 4)) for k in range(1, in_bytes // TWO31 + 1)]
        cross += [k * TWO31 // (2 * W * out_cs * 4) for k in range(1, out_bytes // TWO31 + 1)]
        for r0, r1 in _bands(2 * H, cross):
            got = out[0, r0:r1, :, off_o:off_o + cout].cpu()
            want = _band_ref(xd, off_i, cin, wt, b, r0, r1, act, slope)
            assert torch.equal(got, want[0]), what + f": rows {r0}..{r1}: {int((got != want[0]).sum())} values differ from the float64 transposed convolution"
        # every row: the plain path on overlapping sub-images below 2 GiB; a sub-image's first and last output rows see its zero border
        assert sub_rows * W * in_cs * 4 < LARGE_DEFAULT and 4 * sub_rows * W * out_cs * 4 < LARGE_DEFAULT
        assert lib.vfi_conv_allow_huge(handle, 0) == 0
        step, first, covered = sub_rows - 8, 0, 0
        while covered < 2 * H:
            first = min(first, H - sub_rows)
            sub = torch.full((1, 2 * sub_rows, 2 * W, out_cs), NAN, device="cuda")
            _ck(lib.vfi_conv_forward_ex(handle, xd.data_ptr() + 4 * (first * W * in_cs + off_i), in_cs, sub_rows, W, sub.data_ptr() + 4 * off_o, out_cs, 1, act, slope,
                                        0.0, 0.0, None, 0, None), "forward_ex (sub-image)")
            torch.cuda.synchronize()
            assert _rec(lib)[3] == STORE_PLAIN
            a0 = 0 if first == 0 else 2
            a1 = 2 * sub_rows if first + sub_rows == H else 2 * sub_rows - 2
            assert 2 * first + a0 <= covered, "the sub-images leave a gap"
            same = torch.equal(out[0, 2 * first + a0:2 * first + a1, :, off_o:off_o + cout].view(torch.int32), sub[0, a0:a1, :, off_o:off_o + cout].view(torch.int32))
            assert same, what + f": rows {2 * first + a0}..{2 * first + a1} differ from the plain path on the sub-image that starts at input row {first}"
            covered = 2 * first + a1
            first += step
            del sub
    finally:
        lib.vfi_conv_destroy(handle)


def test_real_size_flavr_dec2(hip_lib, oracle_threads):
    """dec[2] at 2160x3840: 540x960 input, the window of 768 at slice 1 of a [6, 256] pixel (3.19 GB), 64 channels at offset 64 (1 + 1) of the
    384-float pixel of the 1080x1920 output (3.19 GB): the large form on its own"""
    assert 540 * 960 * 1536 * 4 == 3185049600 and 1080 * 1920 * 384 * 4 == 3185049600
    _real_case(hip_lib, 540, 960, 1536, 256, 768, 64, 384, 128, 300, False, seed=2)


def test_real_size_flavr_dec4(hip_lib, oracle_threads):
    """dec[4] at 2160x3840: 1080x1920 input, the window of 384 at slice 1 of a [6, 128] pixel (6.37 GB), 64 channels at offset 64 of the
    256-float pixel of the 2160x3840 output (2 123 366 400 floats, 8.49 GB): only with the permission"""
    assert 1080 * 1920 * 768 * 4 == 6370099200 and 2160 * 3840 * 256 == 2123366400
    _real_case(hip_lib, 1080, 1920, 768, 128, 384, 64, 256, 64, 256, True, seed=4)


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------------

def _refused(lib, handle, xin, in_cs, H, W, out, out_cs, act, text):
    from cfi_amd import _lib

    rc = lib.vfi_conv_forward_ex(handle, xin.data_ptr(), in_cs, H, W, out.data_ptr(), out_cs, 1, act, 0.0, 0.0, 0.0, None, 0, None)
    torch.cuda.synchronize()
    assert rc != 0 and text in _lib.last_error(), (rc, _lib.last_error())
    assert float(out.abs().max()) == 0.0, "a refused call wrote its output"


def test_refusals_above_the_mark(hip_lib):
    """Buffers of the size each call claims: a refusal touches nothing, and a call that is not refused stays inside them"""
    from cfi_amd import _lib

    lib = hip_lib
    # dec[4]'s call without the permission: operands of 6.37 and 8.49 GB
    wt, b = torch.zeros(384, 64, 4, 4), torch.zeros(64)
    handle = lib.vfi_conv_create_ex(1, wt.data_ptr(), b.data_ptr(), 64, 384, 4, 2, 0, None, 384, None)
    assert handle
    try:
        xin, out = torch.zeros(1080 * 1920 * 768, device="cuda"), torch.zeros(2160 * 3840 * 256, device="cuda")
        _refused(lib, handle, xin, 768, 1080, 1920, out, 256, 0, "image larger than 2 GiB")
        assert "vfi_conv_allow_huge" in _lib.last_error()
        # the permission is a switch: on and off again, the call is refused again
        assert lib.vfi_conv_allow_huge(handle, 1) == 0 and lib.vfi_conv_allow_huge(handle, 0) == 0
        _refused(lib, handle, xin, 768, 1080, 1920, out, 256, 0, "image larger than 2 GiB")
        del xin, out
    finally:
        lib.vfi_conv_destroy(handle)
    torch.cuda.empty_cache()
    # per-channel PReLU above the mark (dec[2]'s operands, a window of 760): no large form, the grouped direct tile's refusal (tile 43) as
    # before, permission or not.  (A window that is a multiple of 16 channels goes to the first-generation tile 13, which indexes floats,
    # never had a 2 GiB guard and serves such an input as it always did: docs/design/conv_coverage.md.)
    wt, b, pr = torch.zeros(760, 64, 4, 4), torch.zeros(64), torch.full((64,), 0.25)
    handle = lib.vfi_conv_create_ex(1, wt.data_ptr(), b.data_ptr(), 64, 760, 4, 2, 0, None, 760, pr.data_ptr())
    assert handle
    try:
        xin, out = torch.zeros(540 * 960 * 1536, device="cuda"), torch.zeros(1080 * 1920 * 384, device="cuda")
        for huge in (0, 1):
            assert lib.vfi_conv_allow_huge(handle, huge) == 0
            _refused(lib, handle, xin, 1536, 540, 960, out, 384, 3, "image larger than 2 GiB")
        del xin, out
    finally:
        lib.vfi_conv_destroy(handle)
    torch.cuda.empty_cache()
    # an output over 2^31 - 1 floats with the permission on: 2160 x 3840 pixels of 260 floats
    assert 2160 * 3840 * 260 > 2 ** 31 - 1
    wt, b = torch.zeros(8, 64, 4, 4), torch.zeros(64)
    handle = lib.vfi_conv_create_ex(1, wt.data_ptr(), b.data_ptr(), 64, 8, 4, 2, 0, None, 8, None)
    assert handle
    try:
        assert lib.vfi_conv_allow_huge(handle, 1) == 0
        xin, out = torch.zeros(1080 * 1920 * 8, device="cuda"), torch.zeros(2160 * 3840 * 260, device="cuda")
        _refused(lib, handle, xin, 8, 1080, 1920, out, 260, 0, "image larger than 2 GiB")
        assert "2^31 - 1 floats" in _lib.last_error()
    finally:
        lib.vfi_conv_destroy(handle)
