"""XVFI's new kernels on the device, one at a time, against the float64 restatements of tests/xvfi_restated.py.

  * Conv2d(4, 2, 1) as a layer form (vfi_conv_create_ex kind 0, k 4, stride 2): small-integer data, so every fp32 sum is exact in any order
    and the result must equal the float64 convolution bit for bit; NaN surroundings catch a stray read or write.
  * bicubic down-sampling, bwarp, CFR: rounding bounds derived below from the number of fp32 roundings on the path of one output and the
    absolute sum it rounds; each test prints max err / bound.

Bounds.  u = 2^-24 (fp32 unit roundoff).
  bicubic   16 products and 15 sums in two passes, at most 10 roundings on a path, over sum |k_i k_j x| <= 1.375^2 max|x|: 12 u 1.375^2 max|x|.
  bwarp     the sampling position is computed in fp32 in the same order by kernel and restatement (it is part of the function), the corner
            weights are differences of nearby floats (exact), so an output is 4 products of three factors summed: at most 6 roundings over
            sum w |x| <= max|x|: 8 u max|x|.  Inputs keep every sampled mask outside (0.998, 0.9999), so the gate is the same.
  CFR       a cell sums K contributions f w, w = (sigmoid(z) + 1e-5) exp(-d^2); expf / sigmoid and the rounding of d^2 cost at most 16 u
            relative, the sums K u: numerator and norm each within (K + 16) u of their absolute sums, and the quotient adds both:
            2 (K + 16) u (A / norm + |out|) with A the absolute sum of the numerator's terms.  Targets stay 1e-2 away from an integer, so
            floor() is the same.
"""
import ctypes as C

import pytest
import torch

import xvfi_restated as xr

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
NAN = float("nan")


def _ck(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


# ---- Conv2d(4, 2, 1) -----------------------------------------------------------------------------------------------------------------------

def _int_tensor(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _conv_case(lib, cin, cphys, cout, n, h, w, act=0, res=False, seed=0):
    """One layer, one call inside NaN surroundings -> max |got - want| (0 expected).  The input is a cphys-channel window at channel offset 8
    of a wider tensor; window positions beyond cin hold 12345 (finite; their weights are zero)."""
    g = torch.Generator().manual_seed(1000 + seed)
    wt, b = _int_tensor(g, (cout, cin, 4, 4), -2, 2), _int_tensor(g, (cout,), -3, 3)
    x = _int_tensor(g, (n, h, w, cin), -3, 3)
    want = xr.conv4x4s2_f64(x, wt, b)
    r = _int_tensor(g, (n, h // 2, w // 2, cout), -4, 4) if res else None
    if r is not None:
        want = want + r.double()
    if act == 1:
        want = torch.relu(want)
    assert float(want.abs().max()) < 2 ** 24
    handle = lib.vfi_conv_create_ex(0, wt.data_ptr(), b.data_ptr(), cout, cin, 4, 2, 0, None, cphys, None)
    assert handle, "vfi_conv_create_ex(k=4, stride=2) failed"
    try:
        in_cs, out_cs, off_i, off_o = 8 + cphys + 4, 3 + cout + 5, 8, 3
        xin = torch.full((w + n * h * w + w, in_cs), NAN)
        win = torch.full((n * h * w, cphys), 12345.0)
        win[:, :cin] = x.reshape(-1, cin)
        xin[w:w + n * h * w, off_i:off_i + cphys] = win
        xd = xin.cuda()
        ho, wo = h // 2, w // 2
        out = torch.full((1 + n * ho * wo + 2, out_cs), NAN, device="cuda")
        rd = r.reshape(-1, cout).cuda().contiguous() if r is not None else None
        _ck(lib.vfi_conv_forward_ex(handle, xd.data_ptr() + 4 * (w * in_cs + off_i), in_cs, h, w, out.data_ptr() + 4 * (out_cs + off_o), out_cs, n, act, 0.0,
                                    0.0, 0.0, rd.data_ptr() if rd is not None else None, cout if rd is not None else 0, None), "forward_ex")
        torch.cuda.synchronize()
        got = out.cpu()
        assert torch.isnan(got[0]).all() and torch.isnan(got[-2:]).all(), "wrote a guard pixel"
        body = got[1:-2]
        assert torch.isnan(body[:, :off_o]).all() and torch.isnan(body[:, off_o + cout:]).all(), "wrote a guard channel"
        val = body[:, off_o:off_o + cout].reshape(n, ho, wo, cout)
        assert not torch.isnan(val).any(), "an output is NaN: unwritten, or a NaN was read"
        return float((val.double() - want).abs().max())
    finally:
        lib.vfi_conv_destroy(handle)


@pytest.mark.parametrize("cin,cphys,cout,n,h,w,act,res", [
    (32, 32, 64, 1, 2, 2, 0, False),        # one output pixel: every tap but the centre four is padding
    (64, 64, 128, 1, 4, 6, 1, False),
    (132, 136, 128, 1, 18, 34, 0, False),   # conv_flow2's first layer: Cin 132 in a 136-channel window, more than one tile
    (128, 128, 256, 2, 4, 6, 1, True),      # a batch of two, ReLU, residual
    (30, 32, 64, 2, 18, 34, 0, False),      # a channel window with two dead positions, batch of two, ragged tiles
    (80, 80, 64, 1, 34, 18, 1, False),      # the RefineUNet's first layer at scale 2
])
def test_conv4x4s2_is_exact(hip_lib, cin, cphys, cout, n, h, w, act, res):
    d = _conv_case(hip_lib, cin, cphys, cout, n, h, w, act, res, seed=cin + h)
    print(f"conv4x4s2 {cin}->{cout} n{n} {h}x{w}: max |d| = {d}")
    assert d == 0.0


def test_conv4x4s2_refuses_odd_sizes_and_other_forms(hip_lib):
    from cfi_amd import _lib

    wt, b = torch.zeros(64, 32, 4, 4), torch.zeros(64)
    h = hip_lib.vfi_conv_create_ex(0, wt.data_ptr(), b.data_ptr(), 64, 32, 4, 2, 0, None, 32, None)
    assert h
    try:
        x, out = torch.zeros(1, 5, 6, 32, device="cuda"), torch.zeros(1, 3, 3, 64, device="cuda")
        for hh, ww in ((5, 6), (6, 5)):
            assert hip_lib.vfi_conv_forward_ex(h, x.data_ptr(), 32, hh, ww, out.data_ptr(), 64, 1, 0, 0.0, 0.0, 0.0, None, 0, None) != 0
            assert "even" in _lib.last_error()
    finally:
        hip_lib.vfi_conv_destroy(h)
    assert not hip_lib.vfi_conv_create_ex(0, wt.data_ptr(), b.data_ptr(), 64, 32, 4, 1, 0, None, 32, None)      # k 4 stride 1: no such form
    assert not hip_lib.vfi_conv_create_ex(0, wt.data_ptr(), b.data_ptr(), 64, 32, 4, 2, 1, None, 32, None)      # replicate padding neither


# ---- bicubic ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(8, 8), (32, 48)])
@pytest.mark.parametrize("l", [2, 4, 8])
def test_bicubic_down(hip_lib, h, w, l):
    g = torch.Generator().manual_seed(h + l)
    x = torch.rand((2, h, w, 3), generator=g) * 2 - 0.5
    want = xr.bicubic_down_f64(x, l)
    # the restatement's taps are torch's: F.interpolate(bicubic) in float64 agrees to rounding
    ref = torch.nn.functional.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=1.0 / l, mode="bicubic", align_corners=False).permute(0, 2, 3, 1)
    assert float((ref - want).abs().max()) < 1e-13
    xin = torch.full((2, h, w, 5), NAN)
    xin[..., 1:4] = x
    xd = xin.cuda()
    out = torch.full((2, h // l, w // l, 4), NAN, device="cuda")
    _ck(hip_lib.vfi_xvfi_bicubic_down(xd.data_ptr() + 4, 5, out.data_ptr(), 4, 2, h, w, 3, l, None), "bicubic")
    got = out.cpu()
    assert torch.isnan(got[..., 3]).all() and not torch.isnan(got[..., :3]).any()
    tol = 12 * U * 1.375 ** 2 * float(x.abs().max())
    err = float((got[..., :3].double() - want).abs().max())
    print(f"bicubic {h}x{w} l={l}: max err / bound = {err / tol:.3f}")
    assert err <= tol


# ---- bwarp -------------------------------------------------------------------------------------------------------------------------------------

def _bwarp_flows(n, h, w, seed):
    """Flows that push samples past every border, re-drawn where the sampled mask would lie in (0.998, 0.9999)"""
    g = torch.Generator().manual_seed(seed)
    flo = (torch.rand((n, h, w, 2), generator=g) * 2 - 1) * torch.tensor([0.8 * w, 0.8 * h])
    q = max(h // 4, 1)
    xs, ys = torch.arange(w, dtype=torch.float32).view(1, 1, w), torch.arange(h, dtype=torch.float32).view(1, h, 1)
    flo[:, :q] *= 0.05                             # small motion: interior samples, mask 1
    # samples a fraction of a pixel outside each border: a partly covered footprint, which the gate zeroes
    even = (torch.arange(w) % 2 == 0).view(1, 1, w).expand(n, q, w)
    side = torch.where(even, torch.tensor(-0.3), torch.tensor(w - 1 + 0.6))
    flo[:, q:2 * q, :, 0] = side - xs
    flo[:, q:2 * q, :, 1] *= 0.02
    side = torch.where(even, torch.tensor(-0.45), torch.tensor(h - 1 + 0.35))
    flo[:, 2 * q:3 * q, :, 1] = side - ys[:, 2 * q:3 * q]
    flo[:, 2 * q:3 * q, :, 0] *= 0.02
    flo[0, 0, 0] = torch.tensor([-3.0 * w, 0.0])    # far outside on each side
    flo[0, -1, -1] = torch.tensor([0.0, 5.0 * h])
    probe = torch.zeros(n, h, w, 1)
    for _ in range(20):
        mask = xr.bwarp_f64(probe, flo)[1]
        bad = (mask > 0.998) & (mask < 0.9999)
        if not bad.any():
            break
        flo[bad] += 0.37
    assert not bad.any()
    return flo


@pytest.mark.parametrize("h,w", [(5, 7), (33, 47)])
@pytest.mark.parametrize("c", [3, 64])
def test_bwarp(hip_lib, h, w, c):
    g = torch.Generator().manual_seed(h * c)
    x = torch.randn((2, h, w, c), generator=g)
    flo = _bwarp_flows(2, h, w, h + c)
    flo[1, 1, 1, 0] = float("inf")
    flo[1, 1, 2, 1] = float("nan")
    want, mask = xr.bwarp_f64(x, flo)
    gated = float(((mask < 0.999) & (mask > 0)).double().mean())
    assert gated > 0.05 and float((mask >= 0.999).double().mean()) > 0.1      # both sides of the gate are well represented
    xd, fd = x.cuda(), flo.cuda()
    tol = 8 * U * float(x.abs().max())
    for swap in (0, 1):
        out = torch.full((2, h, w, c + 1), NAN, device="cuda")
        _ck(hip_lib.vfi_xvfi_bwarp(xd.data_ptr(), c, h * w * c, swap, fd.data_ptr(), 2, h * w * 2, out.data_ptr(), c + 1, h * w * (c + 1), 2, h, w, c, None), "bwarp")
        got = out.cpu()
        assert torch.isnan(got[..., c]).all() and not torch.isnan(got[..., :c]).any()
        w_ = xr.bwarp_f64(x.flip(0), flo)[0] if swap else want
        err = float((got[..., :c].double() - w_).abs().max())
        print(f"bwarp {h}x{w} C={c} swap={swap}: max err / bound = {err / tol:.3f} (gated share {gated:.2f})")
        assert err <= tol
        assert float(got[1, 1, 1, :c].abs().max()) == 0.0 and float(got[1, 1, 2, :c].abs().max()) == 0.0      # non-finite positions give 0


def test_bwarp_channel_windows(hip_lib):
    """The object's use: both directions as channel windows of one tensor (image stride = a channel offset), partner swap"""
    h, w, c = 6, 10, 64
    g = torch.Generator().manual_seed(5)
    feat = torch.randn((2, h, w, 2 * c), generator=g)
    flo = _bwarp_flows(1, h, w, 11).repeat(1, 1, 1, 2)[0]      # [h,w,4]: the same flow for both images
    fd, fl = feat.cuda(), flo.contiguous().cuda()
    _ck(hip_lib.vfi_xvfi_bwarp(fd.data_ptr(), 2 * c, h * w * 2 * c, 1, fl.data_ptr(), 4, 2, fd.data_ptr() + 4 * c, 2 * c, h * w * 2 * c, 2, h, w, c, None), "bwarp")
    got = fd.cpu()
    assert torch.equal(got[..., :c], feat[..., :c])
    for n in (0, 1):
        want = xr.bwarp_f64(feat[n ^ 1, :, :, :c][None], flo[None, :, :, 2 * n:2 * n + 2])[0][0]
        assert float((got[n, :, :, c:].double() - want).abs().max()) <= 8 * U * float(feat.abs().max())


# ---- CFR ---------------------------------------------------------------------------------------------------------------------------------------

def _cfr_flow(h, w, t, kind, seed):
    """flow [h,w,4] whose targets t f01, (1 - t) f10 (as fp32 products) stay 1e-2 away from every integer"""
    g = torch.Generator().manual_seed(seed)
    if kind == "holes":      # everything converges on the centre: most cells receive nothing
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        base = torch.stack([w / 2 - xx, h / 2 - yy], -1) * 0.9
        tg = torch.cat([base, base], -1)
    else:
        tg = (torch.rand((h, w, 4), generator=g) * 2 - 1) * 3.0
    tg = torch.floor(tg) + 0.05 + 0.9 * torch.rand((h, w, 4), generator=g)
    t32 = torch.tensor(t, dtype=torch.float32)
    flow = torch.cat([tg[..., :2] / t32, tg[..., 2:] / (1 - t32)], -1)
    if kind == "far":
        flow[0, 0] = torch.tensor([1e4, -1e4, 3e9, -3e9])
        flow[-1, -1] = torch.tensor([-1e20, 1e20, 1e30, -1e30])
        flow[h // 2, w // 2] = torch.tensor([(2.5 * w + 0.4) / t, 0.3 / t, 0.3 / (1 - t), -(2.5 * h + 0.4) / (1 - t)])      # a few image widths outside
    if kind == "nonfinite":
        flow[0, 1, 0] = float("inf")
        flow[1, 0, 1] = float("nan")
        flow[1, 1, 2] = float("-inf")
        flow[h - 1, 0, 3] = float("nan")
    return flow


def _cfr_run(lib, flow, z, t):
    h, w = flow.shape[:2]
    fin = torch.full((h, w, 6), NAN)
    fin[..., 1:5] = flow
    zin = torch.full((h, w, 3), NAN)
    zin[..., :2] = z
    fd, zd = fin.cuda(), zin.cuda()
    out = torch.full((h, w, 5), NAN, device="cuda")
    scratch = torch.zeros(8, dtype=torch.int32, device="cuda")
    _ck(lib.vfi_xvfi_cfr(fd.data_ptr() + 4, 6, zd.data_ptr(), 3, float(t), out.data_ptr(), 5, scratch.data_ptr(), h, w, None), "cfr")
    got = out.cpu()
    assert torch.isnan(got[..., 4]).all()
    return got[..., :4]


@pytest.mark.parametrize("h,w", [(4, 4), (9, 13), (40, 56)])
@pytest.mark.parametrize("t", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("kind", ["random", "holes", "far", "nonfinite"])
def test_cfr(hip_lib, h, w, t, kind):
    flow = _cfr_flow(h, w, t, kind, h * 7 + int(t * 10))
    z = torch.randn((h, w, 2), generator=torch.Generator().manual_seed(h)) * 2
    want, tg, norms = xr.cfr_f64(flow, z, t)
    near = torch.isfinite(tg) & (tg.abs() < max(h, w) + 2)      # (a target further out lands nowhere, whatever its fraction)
    assert float((tg[near] - torch.round(tg[near])).abs().min()) >= 1e-2
    if kind == "holes":
        assert float((norms == 0).double().mean()) >= 0.3
    got = _cfr_run(hip_lib, flow, z, t)
    assert torch.equal(got.view(torch.int32), _cfr_run(hip_lib, flow, z, t).view(torch.int32)), "the same call twice differs"
    ok_flow = torch.where(torch.isfinite(flow), flow, torch.zeros_like(flow))
    aabs, k = xr.cfr_abs_sums(ok_flow, z, tg, t)
    t32 = float(torch.tensor(t, dtype=torch.float32))
    norm = (1 - t32) * norms[..., 0] + t32 * norms[..., 1]
    safe = torch.where(norm > 0, norm, torch.ones_like(norm))
    tol = 2 * (k + 16) * U * (aabs / safe + want.abs().amax(-1)) + 1e-30
    if kind == "nonfinite":      # a cell a non-finite source's OTHER, finite component would have fed: the reference drops the source whole
        assert torch.isfinite(want).all()
    assert torch.isfinite(got).all(), "a non-finite or far target leaked into the result"
    ratio = float(((got.double() - want).abs().amax(-1) / tol).max())
    print(f"cfr {h}x{w} t={t} {kind}: max err / bound = {ratio:.3f}, holes {float((norm == 0).double().mean()):.2f}, max sources per cell {int(k.max())}")
    assert ratio <= 1.0
