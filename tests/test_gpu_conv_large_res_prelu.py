"""Conv2d 3x3 stride 1 + residual + per-channel PReLU (act 3 with a residual) on images of 2 GiB and more: the LARGE forms behind the layer
object's permission vfi_conv_allow_large_res_prelu — the Winograd kernel's MODE 13 with 16x8 and 32x4 regions, and the second-generation
direct kernel's 3x3 stride-1 tiles (csrc/conv_wino.hip, conv_mfma2.hip).  The layer is the last one of AMT-G's ResBlock, prelu(conv5(x3) + r0).

1. Forced, small.  The test option large_image_bytes = 1 makes every image "large"; with the permission on, each form is compared with its
   plain twin bit for bit over the WHOLE output buffer, NaN guard pixels and guard channels included, and both with the float64 convolution
   plus residual, then PReLU, of small-integer data (exact in fp32).  The launch record must name the LARGE form (on the code before these
   forms existed it names the plain one).  Shapes 37x45 (odd, no multiple of a tile or region, several workgroups) and 16x24, N = 2.  Layers:
   AMT-G's rb[4] — 252 logical input channels mapped into a 352-float pixel as the ResBlock lays it out, 252 outputs into a 256-float
   pixel, the residual read from another 256-float pixel — and a small one, Cin 16, Cout 20, every operand a window at an offset inside a
   wider pixel, res_cs != out_cs.
2. Permission off: the same forced call takes the plain form it always took, and the record says so.  Above 2 GiB it is refused with
   "larger than 2 GiB" (3, before the permission is given; tests/test_gpu_conv_large_prelu.py pins the same for an ordinary object).
3. At size: rb[4] at 1080x1920, the half-resolution map of a 2160x3840 frame: a 2 919 628 800-byte input, data made on the device, one call
   per algorithm.  Bands of output rows (the first, the last, the rows around the one where the input's byte offset crosses 2^31) are compared
   bit for bit with float64 on the cropped input; every row is compared with the plain path on overlapping sub-images below 2 GiB.
   Once more per algorithm with the output and the residual in 264-float pixels (2 189 721 600 bytes each): the bands then include the rows
   around THEIR 2^31-byte row.

Exactness: x and the residual in [-3, 3], weights 4 * [-1, 1] (so that the Winograd transform G g G^T is integral), bias in [-3, 3]: every
partial sum is an integer of at most 9 * 252 * 3 * 4 + 3 + 3 = 27 222, far below 2^24 in any order; slopes from test_gpu_conv_large_prelu's
SLOPES, whose products with such integers are exact as well.  The helpers (data, float64 convolution, the launch record's reading) are that
file's, imported: it is an existing test file and stays as it is.
"""
import ctypes as C

import pytest
import torch

from test_gpu_conv_large_prelu import GEN2, LARGE_DEFAULT, NAN, TWO31, WINO, _ck, _ints, _rec, _slopes, conv_f64, epilogue, is_large

pytestmark = pytest.mark.gpu

# AMT-G's decoder1 ResBlock (csrc/amt_net.hip: run_decoder): c = 252 main channels, the last `skip` = 84 of them live behind the main ones
C_RB, SKIP = 252, 84
OFF = (C_RB + 7) // 8 * 8 + 8            # 264: where the side channels sit in the x1 / x3 pixel
XCS = OFF + (SKIP + 7) // 8 * 8          # 352 floats per pixel
RB_MAP = [i if i < C_RB - SKIP else OFF + i - (C_RB - SKIP) for i in range(C_RB)]

# (algorithm choice of vfi_test_conv_algo, family, Winograd region or None)
ALGOS = [(2, WINO, 8), (3, WINO, 16), (1, GEN2, None)]


def _layer(lib, g, cin, cout, cphys, chan_map):
    wt = _ints(g, (cout, cin, 3, 3), -1, 1, 4)
    b = _ints(g, (cout,), -3, 3)
    sl = _slopes(g, cout)
    cm = (C.c_int * len(chan_map))(*chan_map) if chan_map is not None else None
    handle = lib.vfi_conv_create_ex(0, wt.data_ptr(), b.data_ptr(), cout, cin, 3, 1, 0, cm, cphys, sl.data_ptr())
    assert handle, "vfi_conv_create_ex failed"
    return handle, wt, b, sl


def _forced(lib, cin, cphys, chan_map, in_cs, off_i, cout, out_cs, off_o, res_cs, off_r, n, h, w, algo, family, region, permission, variant=None, seed=0):
    """-> the two launch records (default mark, mark 1).  Everything else is asserted."""
    g = torch.Generator().manual_seed(17000 + seed)
    handle, wt, b, sl = _layer(lib, g, cin, cout, cphys, chan_map)
    name = f"conv3x3s1_{cphys}to{cout}".encode()
    try:
        assert off_i + cphys <= in_cs and off_o + cout <= out_cs and off_r + cout <= res_cs
        win = _ints(g, (n, h, w, cphys), -3, 3)      # every float of the window: small integers (unmapped positions have zero weights)
        x = win[..., chan_map] if chan_map is not None else win[..., :cin]
        res = _ints(g, (n, h, w, cout), -3, 3)
        pre = conv_f64(x, wt, b, 3, 1) + res.double()
        assert float(pre.abs().max()) * 2 < 2 ** 24
        want = epilogue(pre, 3, sl).float()
        assert (want < 0).any() and (want > 0).any()
        xin = torch.full((w + n * h * w + w, in_cs), NAN)
        xin[w:w + n * h * w, off_i:off_i + cphys] = win.reshape(-1, cphys)
        rin = torch.full((1 + n * h * w + 2, res_cs), NAN)
        rin[1:-2, off_r:off_r + cout] = res.reshape(-1, cout)
        xd, rd = xin.cuda(), rin.cuda()
        _ck(lib.vfi_conv_allow_large_res_prelu(handle, int(permission)), "allow_large_res_prelu")
        lib.vfi_test_conv_algo(algo)
        if variant is not None:
            lib.vfi_test_variant_override(name + b"=" + str(variant).encode())
        outs, recs = [], []
        for mark in (LARGE_DEFAULT, 1):
            assert lib.vfi_test_set_option(b"large_image_bytes", mark) == 0
            out = torch.full((1 + n * h * w + 2, out_cs), NAN, device="cuda")
            _ck(lib.vfi_conv_forward_ex(handle, xd.data_ptr() + 4 * (w * in_cs + off_i), in_cs, h, w, out.data_ptr() + 4 * (out_cs + off_o), out_cs, n, 3, 0.0,
                                        0.0, 0.0, rd.data_ptr() + 4 * (res_cs + off_r), res_cs, None), "forward_ex")
            torch.cuda.synchronize()
            rec = _rec(lib)
            what = (f"{name.decode()} n{n} {h}x{w} in {off_i}+{cphys}/{in_cs} out {off_o}+{cout}/{out_cs} res {off_r}+/{res_cs} algo {algo} permission {permission} "
                    f"mark {mark}: launch {rec}")
            if family is not None:
                assert rec[0] == family, what
            if rec[0] == WINO:
                assert rec[2] == 13 and (region is None or rec[1] == region), what + ": MODE 13 with the region shape asked for"
            assert variant is None or rec[0] != GEN2 or rec[1] == variant, what
            assert is_large(rec) == (mark == 1 and permission), what + ": the LARGE form is taken under large_image_bytes = 1 with the permission, and only then"
            got = out.cpu()
            assert torch.isnan(got[0]).all() and torch.isnan(got[-2:]).all(), what + ": wrote a guard pixel"
            body = got[1:-2]
            assert torch.isnan(body[:, :off_o]).all() and torch.isnan(body[:, off_o + cout:]).all(), what + ": wrote a guard channel"
            val = body[:, off_o:off_o + cout].reshape(n, h, w, cout)
            assert not torch.isnan(val).any(), what + ": an output is NaN (unwritten, or a NaN was read)"
            assert torch.equal(val, want), what + f": {int((val != want).sum())} values differ from float64"
            outs.append(got)
            recs.append(rec)
        # (without the permission the forced mark moves a Winograd launch to the direct kernel, as it always did: two kernels agree in value, and
        # may differ in the sign of a zero)
        if recs[0][0] == recs[1][0]:
            assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "the two marks differ in some bit of the buffer"
        return recs
    finally:
        lib.vfi_test_set_option(b"large_image_bytes", LARGE_DEFAULT)
        lib.vfi_test_variant_override(b"")
        lib.vfi_test_conv_algo(0)
        lib.vfi_conv_destroy(handle)


SHAPES = [(37, 45), (16, 24)]


# ---- 1. forced, small, permission on ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo,family,region", ALGOS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_forced_amt_g_rb4(hip_lib, h, w, algo, family, region):
    """252 mapped channels of a 352-float pixel -> 252 of 256, + the residual's 252 of 256.  The direct kernel's automatic tile at these
    sizes is d1_m1n1 (61), which has the form; at size it is d1_m1n2 (34), forced here by name as well (below)."""
    _forced(hip_lib, C_RB, XCS, RB_MAP, XCS, 0, C_RB, 256, 0, 256, 0, 2, h, w, algo, family, region, True, seed=h + algo)


def test_forced_amt_g_rb4_tile_34(hip_lib):
    _forced(hip_lib, C_RB, XCS, RB_MAP, XCS, 0, C_RB, 256, 0, 256, 0, 2, 37, 45, 1, GEN2, None, True, variant=34, seed=34)


@pytest.mark.parametrize("algo,family,region", ALGOS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_forced_small_layer_windows_everywhere(hip_lib, h, w, algo, family, region):
    """Cin 16 at +4 of a 24-float pixel, Cout 20 at +3 of 28, the residual at +5 of 40.  (32 padded output channels on the direct kernel:
    tile d1_m2n1, 45, forced by name — the automatic choice at these sizes is a first-generation tile, which has one form only.)"""
    _forced(hip_lib, 16, 16, None, 24, 4, 20, 28, 3, 40, 5, 2, h, w, algo, family, region, True, variant=45 if algo == 1 else None, seed=100 + h + algo)


@pytest.mark.parametrize("variant,cout", [(32, 64), (34, 64), (35, 96), (45, 32), (61, 32)])
def test_forced_every_direct_tile_with_the_form(hip_lib, variant, cout):
    _forced(hip_lib, 132, 136, None, 148, 8, cout, cout + 8, 3, cout + 16, 4, 2, 37, 45, 1, GEN2, None, True, variant=variant, seed=200 + variant)


def test_forced_split_k_is_the_plain_twins(hip_lib):
    """Few tiles and a long K loop: the launch is cut along K and the reduce kernel adds the residual; the LARGE form cuts where its twin cuts"""
    plain, large = _forced(hip_lib, 288, 288, None, 288, 0, 32, 32, 0, 40, 8, 1, 16, 24, 1, GEN2, None, True, variant=61, seed=300)
    assert plain[4] > 1 and plain[4] == large[4], (plain, large)


# ---- 2. permission off --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_permission_off_keeps_the_plain_form(hip_lib, algo):
    """An ordinary layer object under the forced mark: no LARGE launch, whatever the algorithm choice (the Winograd kernel is not eligible for
    a large input it has no permitted form for, so the direct kernel's plain form serves it, as before), and the same values."""
    recs = _forced(hip_lib, C_RB, XCS, RB_MAP, XCS, 0, C_RB, 256, 0, 256, 0, 2, 16, 24, algo, None, None, False, seed=400 + algo)
    assert recs[1][0] == GEN2 and not is_large(recs[1]), recs
    # and the permission can be taken back
    g = torch.Generator().manual_seed(5)
    handle, *_ = _layer(hip_lib, g, 16, 32, 16, None)
    try:
        assert hip_lib.vfi_conv_allow_large_res_prelu(handle, 1) == 0 and hip_lib.vfi_conv_allow_large_res_prelu(handle, 0) == 0
        assert hip_lib.vfi_conv_allow_large_res_prelu(None, 1) != 0
    finally:
        hip_lib.vfi_conv_destroy(handle)


# ---- 3. at size -----------------------------------------------------------------------------------------------------------------------------------

H2, W2 = 1080, 1920      # the half-resolution map of 2160x3840
WIDE = 264               # a pixel stride at which the output and the residual hold 2 189 721 600 bytes there: over 2^31 as well


@pytest.fixture(scope="module")
def rb4_at_size(hip_lib):
    """The layer, its 2.92 GB input and two residuals (256- and 264-float pixels) on the device, and conv + bias in float64 for the bands,
    made once for every case: the first and last rows, the rows around the input's 2^31-byte row and around the wide operands' one"""
    assert H2 * W2 * XCS * 4 == 2919628800 and H2 * W2 * 256 * 4 < TWO31 <= H2 * W2 * WIDE * 4 == 2189721600
    g = torch.Generator().manual_seed(19000)
    handle, wt, b, sl = _layer(hip_lib, g, C_RB, C_RB, XCS, RB_MAP)
    torch.manual_seed(19)
    xd = torch.randint(-3, 4, (1, H2, W2, XCS), device="cuda", dtype=torch.int8).float()
    rds = {cs: torch.randint(-3, 4, (1, H2, W2, cs), device="cuda", dtype=torch.int8).float() for cs in (256, WIDE)}
    cross_in = TWO31 // (W2 * XCS * 4)       # the input row in which byte 2^31 lies
    cross_wide = TWO31 // (W2 * WIDE * 4)    # ... and the row of a 264-float operand
    assert 4 < cross_in < cross_wide - 9 and cross_wide + 5 < H2 - 2
    bands = [(0, 2), (H2 - 2, H2), (cross_in - 4, cross_in + 5), (cross_wide - 4, cross_wide + 5)]
    pres = []
    for r0, r1 in bands:
        lo, hi = r0 - 1, r1 + 1
        crop = xd[:, max(lo, 0):min(hi, H2)].cpu()[..., RB_MAP]
        v = conv_f64(crop, wt, b, 3, 1, top=lo < 0, bottom=hi > H2)
        assert v.shape[1] == r1 - r0 and (float(v.abs().max()) + 3) * 2 < 2 ** 24
        pres.append(v)
    yield dict(handle=handle, xd=xd, rds=rds, bands=bands, pres=pres, sl=sl)
    hip_lib.vfi_conv_destroy(handle)
    del xd, rds
    torch.cuda.empty_cache()


@pytest.mark.parametrize("algo,family,region", ALGOS)
@pytest.mark.parametrize("ocs", [256, WIDE], ids=["rb4", "wide_output_and_residual"])
def test_at_size_rb4(hip_lib, rb4_at_size, ocs, algo, family, region, oracle_threads):
    """ocs 256: AMT-G's own call, only the input over 2 GiB.  ocs 264: the same layer writing into, and adding a residual from, pixels of
    264 floats, so that the output's and the residual's per-region descriptors (Winograd) and 64-bit addresses (direct kernel) are compared
    with float64 around THEIR 2^31-byte row as well, and in the rows behind it."""
    from cfi_amd import _lib

    u = rb4_at_size
    handle, xd, rd = u["handle"], u["xd"], u["rds"][ocs]
    out = torch.full((1, H2, W2, ocs), NAN, device="cuda")

    def call(first, rows, dst):
        return hip_lib.vfi_conv_forward_ex(handle, xd.data_ptr() + 4 * first * W2 * XCS, XCS, rows, W2, dst.data_ptr(), ocs, 1, 3, 0.0, 0.0, 0.0,
                                           rd.data_ptr() + 4 * first * W2 * ocs, ocs, None)

    try:
        hip_lib.vfi_test_conv_algo(algo)
        _ck(hip_lib.vfi_conv_allow_large_res_prelu(handle, 0), "permission off")
        rc = call(0, H2, out)
        assert rc != 0 and "larger than 2 GiB" in _lib.last_error(), (rc, _lib.last_error())
        _ck(hip_lib.vfi_conv_allow_large_res_prelu(handle, 1), "permission on")
        _ck(call(0, H2, out), "forward_ex (at size)")
        torch.cuda.synchronize()
        rec = _rec(hip_lib)
        what = f"rb[4] {H2}x{W2} out / res stride {ocs} algo {algo}: launch {rec}"
        print(what)
        assert rec[0] == family and is_large(rec) and (region is None or (rec[1] == region and rec[2] == 13)), what
        assert bool(torch.isnan(out[..., C_RB:]).all()), what + ": a channel beside the 252 was written"
        for (r0, r1), pre in zip(u["bands"], u["pres"]):
            want = epilogue(pre + rd[:, r0:r1, :, :C_RB].cpu().double(), 3, u["sl"]).float()
            diff = int((out[0, r0:r1, :, :C_RB].cpu() != want[0]).sum())
            assert diff == 0, what + f": rows {r0}..{r1}: {diff} values differ from float64"
        # every row: the plain path on overlapping sub-images below 2 GiB
        rows_sub = ((LARGE_DEFAULT - 1) // (W2 * XCS * 4)) // 4 * 4
        n_sub = -(-(H2 - 16) // (rows_sub - 16))
        starts = [min(i * (rows_sub - 16), H2 - rows_sub) // 2 * 2 for i in range(n_sub)]
        assert starts[0] == 0 and starts[-1] + rows_sub == H2 and all(b_ - a_ <= rows_sub - 16 for a_, b_ in zip(starts, starts[1:])), (starts, rows_sub)
        for first in starts:
            sub = torch.full((1, rows_sub, W2, ocs), NAN, device="cuda")
            _ck(call(first, rows_sub, sub), "forward_ex (sub-image)")
            torch.cuda.synchronize()
            srec = _rec(hip_lib)
            assert srec[0] == family and not is_large(srec), what + f": the sub-image's launch {srec}"
            a0 = 0 if first == 0 else 2
            a1 = rows_sub - (0 if first + rows_sub == H2 else 2)
            same = torch.equal(out[0, first + a0:first + a1, :, :C_RB].view(torch.int32), sub[0, a0:a1, :, :C_RB].view(torch.int32))
            assert same, what + f": rows {first + a0}..{first + a1} differ from the plain path on the sub-image that starts at row {first}"
            del sub
    finally:
        hip_lib.vfi_test_conv_algo(0)
        del out
        torch.cuda.empty_cache()
