"""Layer objects on operand images of 4 GiB and more: the per-object permission vfi_conv_allow_huge and the LARGE kernel forms behind it
(csrc/conv_large.h, conv_mfma2.hip, conv_wino.hip).  Companion of test_gpu_conv_large.py (2 GiB up to 4 GiB), whose data scheme, float64
reference and launch-record helpers are used here: small integers, every fp32 sum exact in any order.

1. Forced, small: large_image_bytes = 1 with the permission on against the plain form, bit for bit, at that file's forcing shapes and at
   FILM's `pred` window (128 channels at offset 4 of a 132-float pixel).
2. Real size, FILM's three layers as they occur at 2160x3840, under both algorithms: bands of rows against float64 on the host, every
   row against the plain path on overlapping sub-images below 2 GiB, NaN beside the output window, the launch record.
3. The same calls without the permission are refused with the message they always had and write nothing.
4. An image over the stated bound (2^31 - 1 floats) is refused with the permission on.
"""
import ctypes as C

import pytest
import torch

import test_gpu_conv_large as base
from test_gpu_conv_large import GEN2, LARGE_DEFAULT, NAN, TWO31, WINO, _ck, _ints, _rec, conv_f64, epilogue, is_large

pytestmark = pytest.mark.gpu


def _create(lib, wt, b, cout, cin, cphys, chan_map=None, huge=True):
    cm = (C.c_int * cin)(*chan_map) if chan_map is not None else None
    handle = lib.vfi_conv_create_ex(0, wt.data_ptr(), b.data_ptr(), cout, cin, 3, 1, 0, cm, cphys, None)
    assert handle, "vfi_conv_create_ex failed"
    if huge:
        assert lib.vfi_conv_allow_huge(handle, 1) == 0
    return handle


# ---- 1. forced, small ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo,family", [(1, GEN2), (2, WINO)])
@pytest.mark.parametrize("h,w,cin,cphys,in_cs,off_i,cout", [(2, 2, 132, 136, 148, 8, 64), (5, 7, 132, 136, 148, 8, 64), (18, 34, 132, 136, 148, 8, 64),
                                                            (40, 72, 132, 136, 148, 8, 64), (18, 34, 128, 128, 132, 4, 32), (40, 72, 128, 128, 132, 4, 32)])
def test_forced_with_permission_equals_plain(hip_lib, h, w, cin, cphys, in_cs, off_i, cout, algo, family):
    lib, n = hip_lib, 2
    g = torch.Generator().manual_seed(8100 + h + cin)
    wt, b = _ints(g, (cout, cin, 3, 3), -1, 1, 4), _ints(g, (cout,), -3, 3)
    x = _ints(g, (n, h, w, cin), -3, 3)
    r = _ints(g, (n, h, w, cout), -4, 4)
    pre = conv_f64(x, wt, b, 3, 1)
    out_cs, off_o, res_cs, off_r = 3 + cout + 5, 3, 2 + cout + 4, 2
    xin = torch.full((w + n * h * w + w, in_cs), NAN)
    win = torch.full((n * h * w, cphys), 12345.0)
    win[:, :cin] = x.reshape(-1, cin)
    xin[w:w + n * h * w, off_i:off_i + cphys] = win
    xd = xin.cuda()
    rin = torch.full((1 + n * h * w + 1, res_cs), NAN)
    rin[1:-1, off_r:off_r + cout] = r.reshape(-1, cout)
    rd = rin.cuda()
    handles = {huge: _create(lib, wt, b, cout, cin, cphys, huge=huge) for huge in (False, True)}
    try:
        lib.vfi_test_conv_algo(algo)
        if cout == 32:      # a small image with 32 output channels takes a first-generation tile, which has no LARGE form (and never refused an
            # image): the second-generation 16x16x32 tile d1_m2n1 that FILM's pred[0][0] takes at full size, by trace name
            lib.vfi_test_variant_override(f"conv3x3s1_{cphys}to{cout}=45".encode())
        for act, slope, res in base.EPILOGUES:
            want = epilogue(pre, act, slope, r if res else None).float()
            outs = []
            for huge, mark in ((False, LARGE_DEFAULT), (True, LARGE_DEFAULT), (True, 1)):
                assert lib.vfi_test_set_option(b"large_image_bytes", mark) == 0
                out = torch.full((1 + n * h * w + 2, out_cs), NAN, device="cuda")
                _ck(lib.vfi_conv_forward_ex(handles[huge], xd.data_ptr() + 4 * (w * in_cs + off_i), in_cs, h, w, out.data_ptr() + 4 * (out_cs + off_o), out_cs, n, act,
                                            slope, 0.0, 0.0, rd.data_ptr() + 4 * (res_cs + off_r) if res else None, res_cs if res else 0, None), "forward_ex")
                torch.cuda.synchronize()
                rec = _rec(lib)
                what = f"{h}x{w} cin {cin} at {off_i} of {in_cs} algo {algo} act {act}/{slope} res {res} huge {huge} mark {mark}: launch {rec}"
                assert rec[0] == family and is_large(rec) == (mark == 1), what
                outs.append((rec, out.cpu()))
            plain_rec, plain = outs[0]
            body = plain[1:-2, off_o:off_o + cout].reshape(n, h, w, cout)
            assert torch.equal(body, want), what
            for rec, got in outs[1:]:
                # NaN guards compare equal as bits: the whole buffer, guard pixels and guard channels included
                assert torch.equal(got.view(torch.int32), plain.view(torch.int32)), what
            assert outs[1][0][:7] == plain_rec[:7], "the permission alone changed a launch: %s -> %s" % (plain_rec, outs[1][0])
    finally:
        lib.vfi_test_set_option(b"large_image_bytes", LARGE_DEFAULT)
        lib.vfi_test_variant_override(b"")
        lib.vfi_test_conv_algo(0)
        for hd in handles.values():
            lib.vfi_conv_destroy(hd)
        torch.cuda.empty_cache()


# ---- 2. real size: FILM's three layers at 2160x3840 -----------------------------------------------------------------------------------------

def _film_map(F=64, nf=64):
    """film_net.hip's aligned_map(F) + the fusion slot: 2 * (3 + F) + 4 + nf logical channels on cal + nf physical ones"""
    m = []
    for half in range(2):
        m += [half * (4 + F) + c for c in range(3)] + [half * (4 + F) + 4 + c for c in range(F)]
    m += [2 * (4 + F) + c for c in range(4)]
    cal = (2 * (4 + F) + 4 + 7) // 8 * 8
    return m + [cal + c for c in range(nf)], cal + nf


MAP208, CS208 = _film_map()
#        name             H     W     in_cs  off  cin  cphys  chan_map  cout
LAYERS = {"pred_132": (2160, 3840, 132, 4, 128, 128, None, 32),
          "fuse_208": (2160, 3840, CS208, 0, len(MAP208), CS208, MAP208, 64),
          "fuse_528": (1080, 1920, 528, 0, 528, 528, None, 128)}
_cache = {}      # per layer: weights, input seed and the float64 bands, shared by the two algorithms


def _layer_data(name):
    if name not in _cache:
        H, W, in_cs, off, cin, cphys, cmap, cout = LAYERS[name]
        g = torch.Generator().manual_seed(9100 + in_cs)
        _cache[name] = {"wt": _ints(g, (cout, cin, 3, 3), -1, 1, 4), "b": _ints(g, (cout,), -3, 3), "bands": {}}
    return _cache[name]


def _bands(rows, crossings, half=4):
    out = [(0, min(2 * half, rows)), (max(rows - 2 * half, 0), rows)]
    for c in crossings:
        out.append((max(c - half, 0), min(c + half + 1, rows)))
    return out


@pytest.mark.parametrize("algo,family", [(1, GEN2), (2, WINO)])
@pytest.mark.parametrize("name", list(LAYERS))
def test_real_size_film_layers(hip_lib, oracle_threads, name, algo, family):
    lib = hip_lib
    H, W, in_cs, off, cin, cphys, cmap, cout = LAYERS[name]
    in_bytes = H * W * in_cs * 4
    assert in_bytes > 2 ** 32 and H * W * in_cs <= lib.vfi_conv_huge_max_floats()
    d = _layer_data(name)
    wt, b = d["wt"], d["b"]
    torch.manual_seed(in_cs)
    xd = torch.randint(-3, 4, (1, H, W, in_cs), device="cuda", dtype=torch.int8).float()      # every float of every pixel: small integers
    out_cs = cout + 8
    out = torch.full((1, H, W, out_cs), NAN, device="cuda")
    logical = (lambda t: t[..., MAP208]) if cmap is not None else (lambda t: t[..., off:off + cin])
    handle = _create(lib, wt, b, cout, cin, cphys, cmap)
    try:
        lib.vfi_test_conv_algo(algo)
        lib.vfi_test_large_launches(None, 0)
        _ck(lib.vfi_conv_forward_ex(handle, xd.data_ptr() + 4 * off, in_cs, H, W, out.data_ptr(), out_cs, 1, 1, 0.25, 0.0, 0.0, None, 0, None), "forward_ex (huge)")
        torch.cuda.synchronize()
        rec = _rec(lib)
        log = (C.c_int32 * 12)()
        what = f"{name}: {cin}->{cout} on {H}x{W}x{in_cs} ({in_bytes} bytes) algo {algo}: launch {rec}"
        print(what)
        assert rec[0] == family and is_large(rec), what
        assert lib.vfi_test_large_launches(log, 2) == 1 and list(log[:6]) == [family, H, W, in_cs, cphys, cout], what
        row_bytes = W * in_cs * 4
        crossings = [k * TWO31 // row_bytes for k in range(1, in_bytes // TWO31 + 1)]
        assert len(crossings) == in_bytes // TWO31 >= 2
        for r0, r1 in _bands(H, crossings):
            if (r0, r1) not in d["bands"]:
                lo, hi = max(r0 - 1, 0), min(r1 + 1, H)
                crop = logical(xd[:, lo:hi]).cpu()
                v = conv_f64(crop, wt, b, 3, 1, top=r0 == 0, bottom=r1 == H)
                assert v.shape[1] == r1 - r0 and float(v.abs().max()) < 2 ** 24
                d["bands"][(r0, r1)] = epilogue(v, 1, 0.25, None).float()[0]
            got = out[0, r0:r1].cpu()
            want = d["bands"][(r0, r1)]
            assert torch.isnan(got[..., cout:]).all(), what + f": rows {r0}..{r1}: a channel beside the output window was written"
            assert torch.equal(got[..., :cout], want), what + f": rows {r0}..{r1}: {int((got[..., :cout] != want).sum())} values differ from float64"
        assert torch.isnan(out[..., cout:]).all(), what + ": a channel beside the output window was written"
        # every row: the plain path on overlapping sub-images below 2 GiB
        rows_sub = (LARGE_DEFAULT - 1 - 4 * off) // row_bytes // 2 * 2
        step = rows_sub - 16
        starts = list(range(0, H - rows_sub, step)) + [H - rows_sub]
        covered = 0
        for first in starts:
            sub = torch.full((1, rows_sub, W, out_cs), NAN, device="cuda")
            _ck(lib.vfi_conv_forward_ex(handle, xd.data_ptr() + 4 * (first * W * in_cs + off), in_cs, rows_sub, W, sub.data_ptr(), out_cs, 1, 1, 0.25, 0.0, 0.0, None, 0,
                                        None), "forward_ex (sub-image)")
            torch.cuda.synchronize()
            srec = _rec(lib)
            assert srec[0] == family and not is_large(srec), (what, srec)
            a0, a1 = (0 if first == 0 else 2), (rows_sub if first + rows_sub == H else rows_sub - 2)      # all rows but those at a cut
            assert first + a0 <= covered, "the sub-images leave a gap"
            same = torch.equal(out[0, first + a0:first + a1, :, :cout].view(torch.int32), sub[0, a0:a1, :, :cout].view(torch.int32))
            assert same, what + f": rows {first + a0}..{first + a1} differ from the plain path on the sub-image that starts at row {first}"
            covered = first + a1
            del sub
        assert covered == H
        assert lib.vfi_test_large_launches(log, 2) == 0
    finally:
        lib.vfi_test_conv_algo(0)
        lib.vfi_conv_destroy(handle)
        del xd, out
        torch.cuda.empty_cache()


# ---- 3. / 4. refusals -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(LAYERS))
def test_without_the_permission_refused_and_nothing_touched(hip_lib, name):
    from cfi_amd import _lib

    H, W, in_cs, off, cin, cphys, cmap, cout = LAYERS[name]
    wt, b = torch.ones(cout, cin, 3, 3), torch.ones(cout)
    # buffers of the size the call claims: a refusal touches nothing, and a call that is not refused stays inside them
    xin, out = torch.ones(H * W * in_cs, device="cuda"), torch.zeros(H * W * cout, device="cuda")
    handle = _create(hip_lib, wt, b, cout, cin, cphys, cmap, huge=False)
    try:
        for algo in (0, 1, 2):
            hip_lib.vfi_test_conv_algo(algo)
            rc = hip_lib.vfi_conv_forward_ex(handle, xin.data_ptr() + 4 * off, in_cs, H, W, out.data_ptr(), cout, 1, 1, 0.25, 0.0, 0.0, None, 0, None)
            assert rc != 0 and "image larger than 2 GiB" in _lib.last_error(), (name, algo, rc, _lib.last_error())
        torch.cuda.synchronize()
        assert float(out.abs().max()) == 0.0, "a refused call wrote its output"
        # the permission is a switch: on, the call runs; off again, it is refused again
        assert hip_lib.vfi_conv_allow_huge(handle, 1) == 0 and hip_lib.vfi_conv_allow_huge(handle, 0) == 0
        rc = hip_lib.vfi_conv_forward_ex(handle, xin.data_ptr() + 4 * off, in_cs, H, W, out.data_ptr(), cout, 1, 1, 0.25, 0.0, 0.0, None, 0, None)
        assert rc != 0 and "image larger than 2 GiB" in _lib.last_error()
    finally:
        hip_lib.vfi_test_conv_algo(0)
        hip_lib.vfi_conv_destroy(handle)
        del xin, out
        torch.cuda.empty_cache()


def test_above_the_bound_refused_with_the_permission(hip_lib):
    """2521 x 4096 x 208 floats = 2 147 876 864 > 2^31 - 1: the image's float count no longer fits the kernels' int"""
    from cfi_amd import _lib

    H, W, cs, cout = 2521, 4096, 208, 64
    assert H * W * cs > hip_lib.vfi_conv_huge_max_floats() >= (H - 1) * W * cs
    wt, b = torch.ones(cout, cs, 3, 3), torch.ones(cout)
    xin, out = torch.ones(H * W * cs, device="cuda"), torch.zeros(H * W * cout, device="cuda")
    handle = _create(hip_lib, wt, b, cout, cs, cs)
    try:
        for algo in (0, 1, 2):
            hip_lib.vfi_test_conv_algo(algo)
            rc = hip_lib.vfi_conv_forward_ex(handle, xin.data_ptr(), cs, H, W, out.data_ptr(), cout, 1, 1, 0.25, 0.0, 0.0, None, 0, None)
            assert rc != 0 and "image larger than 2 GiB" in _lib.last_error(), (algo, rc, _lib.last_error())
        torch.cuda.synchronize()
        assert float(out.abs().max()) == 0.0
    finally:
        hip_lib.vfi_test_conv_algo(0)
        hip_lib.vfi_conv_destroy(handle)
        del xin, out
        torch.cuda.empty_cache()
