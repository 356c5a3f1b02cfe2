"""-m gpu: the ops backend's kernels (csrc/ref_ops.hip) at the shapes where tiled kernels go wrong, against the float64 / exact
restatements of tests/ref_ops_restated.py (pinned to the reference's goldens by tests/test_ref_ops_restated_cpu.py).

  * sepconv: the K = 51 tile kernel (64 x 8 tiles, pixel-row pairs, 4-channel groups) at partial tiles and channel tails, the any-K
    kernel, inputs larger than needed, channel slices and expanded (stride 0) operands, the grid limit;
  * AdaCoF: channel passes of 8 and their tail, F and dilation, offsets at exact integers, just around negative integers, and far
    outside the image;
  * correlation: channel passes of 8, images smaller than the 9 x 9 window and not a multiple of the 16 x 16 tile, N = 3 slices;
  * distance transform: bit for bit, both passes, every fp32 square root of an integer below 2^24, and the LDS line limit.

Every output is pre-filled with NaN, so an element the kernel does not write fails; where the API takes output strides the output
is a window of a larger NaN tensor whose other elements must stay NaN.  Operands that are windows of larger tensors have NaN
around them: a read outside the operand poisons the result.  Tolerances are gamma * 2^-24 * sum|terms| per element; for the
operands in [0.5, 1] each case also asserts that one summand (a tap, a channel) is larger than that tolerance, so a dropped or
doubled summand fails.  Fixed seeds throughout."""
import ctypes as C

import numpy as np
import pytest
import torch

import ref_ops_restated as rs

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def lib(hip_lib):
    from cfi_amd import ops

    ops.init()
    return hip_lib


@pytest.fixture(scope="module")
def ops(lib):
    from cfi_amd import ops as m

    return m


def _ck(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _st(t):
    return (C.c_longlong * 4)(*t.stride())


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _pos(shape, g, lo=0.5, hi=1.0):
    return lo + (hi - lo) * torch.rand(*shape, device=DEV, generator=g)


def _in_nan(shape, pad, g, make):
    """a tensor of `shape` that is the interior window of a NaN tensor padded by `pad` on every side of every dim"""
    big = torch.full([s + 2 * pad for s in shape], NAN, device=DEV)
    win = big[tuple(slice(pad, pad + s) for s in shape)]
    win.copy_(make(shape, g))
    return win


def _nan_window(shape):
    """(outer NaN tensor, output window of `shape` inside it, mask of the outer elements that must stay NaN)"""
    outer = torch.full([s + 3 for s in shape], NAN, device=DEV)
    idx = tuple(slice(1, 1 + s) for s in shape)
    keep = torch.ones(outer.shape, dtype=torch.bool, device=DEV)
    keep[idx] = False
    return outer, outer[idx], keep


def _check(got, want, M, gamma, what, mn=None):
    got = got.detach().double().cpu()
    tol = rs.tolerance(M.cpu(), gamma)
    d = (got - want.cpu()).abs()
    bad = ~(d <= tol)                          # NaN (an unwritten element) counts as bad
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {d.numel()} elements outside gamma*u*M "
                           f"(first at {tuple(int(i) for i in bad.nonzero()[0])}; NaN: {int(got.isnan().sum())})")
    if mn is not None:
        mn = mn.cpu()
        live = M.cpu() > 0
        assert (mn[live] > tol[live]).all(), f"{what}: a summand is below the tolerance; the case cannot see a dropped one"
    print(f"{what}: max|d| = {d.max():.3e}, max tol = {tol.max():.3e}")


# ---- separable adaptive convolution -----------------------------------------------------------------------------------------------

def _sepconv_direct(lib, x, ver, hor, out):
    N, Cc, Hin, Win = x.shape
    K, Ho, Wo = ver.shape[1:]
    return lib.vfi_sepconv(x.data_ptr(), _st(x), ver.data_ptr(), _st(ver), hor.data_ptr(), _st(hor), out.data_ptr(), _st(out), N, Cc,
                           Hin, Win, Ho, Wo, K, _stream())


def _sepconv_case(lib, seed, N, Cc, Ho, Wo, K, extra=(0, 0), signed=False):
    g = _gen(seed)
    make = (lambda s, g: torch.randn(*s, device=DEV, generator=g)) if signed else _pos
    x = _in_nan((N, Cc, Ho + K - 1 + extra[0], Wo + K - 1 + extra[1]), 2, g, make)
    taps = torch.full((N, 2 * K + 3, Ho + 2, Wo + 2), NAN, device=DEV)
    ver, hor = taps[:, 1:1 + K, 1:1 + Ho, 1:1 + Wo], taps[:, 2 + K:2 + 2 * K, 1:1 + Ho, 1:1 + Wo]
    ver.copy_(make((N, K, Ho, Wo), g) / K)
    hor.copy_(make((N, K, Ho, Wo), g) / K)
    outer, out, keep = _nan_window((N, Cc, Ho, Wo))
    _ck(_sepconv_direct(lib, x, ver, hor, out), "vfi_sepconv")
    torch.cuda.synchronize()
    assert outer[keep].isnan().all(), "sepconv wrote outside its output window"
    # rows / columns beyond Ho + K - 1 / Wo + K - 1 (the extra ones) are NaN-free input the result must not depend on
    want, M, mn = rs.sepconv(x.cpu(), ver.cpu(), hor.cpu(), min_term=True)
    _check(out, want, M, rs.gamma_sepconv(K), f"sepconv N{N} C{Cc} {Ho}x{Wo} K{K} extra{extra}", None if signed else mn)
    return x, ver, hor, out


# (N, C, Ho, Wo): every C in {1,2,3,5,8}, Wo in {1,63,64,65,130}, Ho in {1,2,7,8,9,17}, N in {1,3} at least once; C = 3 with
# partial edge tiles in both directions (130 = 2*64 + 2, 17 = 2*8 + 1)
SEP51 = [(1, 1, 1, 1), (1, 2, 2, 63), (3, 3, 17, 130), (1, 3, 9, 65), (3, 5, 8, 64), (1, 8, 7, 130), (3, 3, 1, 65), (1, 5, 17, 1)]


@pytest.mark.parametrize("N,Cc,Ho,Wo", SEP51)
def test_sepconv_k51_tiles(lib, N, Cc, Ho, Wo):
    _sepconv_case(lib, 100 + Cc * Ho + Wo, N, Cc, Ho, Wo, 51)


@pytest.mark.parametrize("K,N,Cc,Ho,Wo", [(1, 3, 3, 5, 7), (3, 1, 5, 9, 65), (13, 3, 2, 17, 1), (49, 1, 3, 8, 66), (53, 3, 1, 2, 9)])
def test_sepconv_any_k(lib, K, N, Cc, Ho, Wo):
    _sepconv_case(lib, 200 + K, N, Cc, Ho, Wo, K)


@pytest.mark.parametrize("K", [51, 5])
def test_sepconv_larger_input(lib, K):
    """the API accepts an input with more than Ho + K - 1 rows / Wo + K - 1 columns; poison the extra ones with NaN"""
    x, ver, hor, out = _sepconv_case(lib, 300 + K, 3, 3, 9, 65, K, extra=(11, 70))
    xp = x.clone()
    xp[:, :, 9 + K - 1:] = NAN
    xp[:, :, :, 65 + K - 1:] = NAN
    o2 = torch.full_like(out, NAN)
    _ck(_sepconv_direct(lib, xp, ver, hor, o2), "vfi_sepconv")
    assert torch.equal(o2, out)


def test_sepconv_signed(lib):
    """signed operands: cancellation, still inside the magnitude bound"""
    _sepconv_case(lib, 400, 3, 3, 17, 130, 51, signed=True)
    _sepconv_case(lib, 401, 1, 5, 9, 20, 7, signed=True)


def test_sepconv_slices_and_expanded(lib, ops):
    """channel-slice and stride-0 operands through the wrapper: bit for bit the contiguous call, and within the bound"""
    g = _gen(500)
    K, N, Ho, Wo = 51, 3, 9, 70
    big = _pos((N, 7, Ho + K - 1, Wo + K - 1), g)
    x = big[:, 2:5]                                            # C = 3 slice
    ver = _pos((1, K, Ho, Wo), g).div_(K).expand(N, K, Ho, Wo)  # batch stride 0
    hor = _pos((N, K, Ho, Wo), g).div_(K)
    assert ver.stride(0) == 0 and not x.is_contiguous()
    got = ops.sepconv_func.apply(x, ver, hor)
    assert torch.equal(got, ops.sepconv_func.apply(x.contiguous(), ver.contiguous(), hor))
    want, M, mn = rs.sepconv(x.cpu(), ver.cpu(), hor.cpu(), min_term=True)
    _check(got, want, M, rs.gamma_sepconv(K), "sepconv slices / expanded", mn)
    # one image broadcast over every channel (channel stride 0) on the any-K kernel as well as the tile kernel
    for k in (K, 3):
        img = _pos((N, 1, Ho + k - 1, Wo + k - 1), g).expand(N, 5, Ho + k - 1, Wo + k - 1)
        v, h = ver[:, :k] * K / k, hor[:, :k] * K / k
        got = ops.sepconv_func.apply(img, v, h)
        assert torch.equal(got, ops.sepconv_func.apply(img.contiguous(), v, h))
        assert torch.equal(got, got[:, :1].expand_as(got))
        want, M = rs.sepconv(img.cpu(), v.cpu(), h.cpu())
        _check(got, want, M, rs.gamma_sepconv(k), f"sepconv channel-stride-0 K{k}")


def test_sepconv_grid_limit_rejected(lib):
    """N * ceil(C / 4) >= 65536 on the tile kernel: an error before any launch (the output stays NaN)"""
    K, N, Cc = 51, 16384, 16
    x = torch.zeros(1, 1, K, K, device=DEV).expand(N, Cc, K, K)
    t = torch.zeros(1, K, 1, 1, device=DEV).expand(N, K, 1, 1)
    out = torch.full((N, Cc, 1, 1), NAN, device=DEV)
    rc = _sepconv_direct(lib, x, t, t, out)
    assert rc != 0
    from cfi_amd import _lib

    assert "exceeds the grid" in _lib.last_error()
    torch.cuda.synchronize()
    assert out.isnan().all()
    out2 = torch.full((N, 15, 1, 1), NAN, device=DEV)               # ceil(15 / 4) = 4 groups: still 65536
    assert _sepconv_direct(lib, x[:, :15], t, t, out2) != 0
    # one image fewer is accepted
    out3 = torch.full((N - 1, Cc, 1, 1), NAN, device=DEV)
    _ck(_sepconv_direct(lib, x[:N - 1], t[:N - 1], t[:N - 1], out3), "vfi_sepconv")
    torch.cuda.synchronize()
    assert (out3 == 0).all()


# ---- AdaCoF -------------------------------------------------------------------------------------------------------------------------

def _offsets(kind, shape, g, H, W):
    if kind == "rand":
        return (torch.rand(*shape, device=DEV, generator=g) * 2 - 1) * 3
    if kind == "int":
        return torch.randint(-3, 4, shape, device=DEV, generator=g).float()
    if kind == "near_neg":      # just above / below a negative integer and a hair below zero: truncation and the negative fraction
        vals = torch.tensor([-1 + 1e-6, -1 - 1e-6, -1e-7, -2 + 1e-6, -2 - 1e-6, 1e-7], device=DEV)
        return vals[torch.randint(0, len(vals), shape, device=DEV, generator=g)]
    if kind == "huge":          # far outside: every corner clamps to the edge
        sgn = torch.randint(0, 2, shape, device=DEV, generator=g).float() * 2 - 1
        return sgn * (5 * (H + W) + torch.rand(*shape, device=DEV, generator=g))
    raise ValueError(kind)


def _adacof_case(lib, seed, Cc, Fs, dil, kind, N=2, Ho=13, Wo=19, signed=False):
    g = _gen(seed)
    H, W = Ho + (Fs - 1) * dil, Wo + (Fs - 1) * dil
    lo = 0.9 if kind == "near_neg" else 0.5      # the extrapolated bilinear sum stays away from zero on [0.9, 1]
    if signed:
        x = torch.randn(N, Cc, H, W, device=DEV, generator=g)
        w = torch.randn(N, Fs * Fs, Ho, Wo, device=DEV, generator=g)
    else:
        x = _pos((N, Cc, H, W), g, lo)
        w = _pos((N, Fs * Fs, Ho, Wo), g)
    oi = _offsets(kind, (N, Fs * Fs, Ho, Wo), g, H, W)
    oj = _offsets(kind, (N, Fs * Fs, Ho, Wo), g, H, W)
    out = torch.full((N, Cc, Ho, Wo), NAN, device=DEV)
    _ck(lib.vfi_adacof(x.data_ptr(), w.data_ptr(), oi.data_ptr(), oj.data_ptr(), out.data_ptr(), N, Cc, H, W, Fs, dil, Ho, Wo,
                       _stream()), "vfi_adacof")
    want, M, mn = rs.adacof(x.cpu(), w.cpu(), oi.cpu(), oj.cpu(), dil, min_term=True)
    _check(out, want, M, rs.gamma_adacof(Fs), f"adacof C{Cc} F{Fs} d{dil} {kind}", None if signed else mn)
    return x, w, oi, oj, out


# every C in {1,3,8,9,17}, F in {1,3,5}, dilation in {1,2,3} and offset kind at least once
ADACOF = [(1, 1, 1, "rand"), (3, 3, 2, "int"), (8, 5, 1, "near_neg"), (9, 3, 3, "rand"), (17, 5, 2, "huge"), (9, 1, 3, "near_neg"),
          (17, 3, 1, "rand"), (3, 5, 3, "int"), (9, 5, 1, "huge"), (17, 3, 2, "near_neg")]


@pytest.mark.parametrize("Cc,Fs,dil,kind", ADACOF)
def test_adacof_edges(lib, Cc, Fs, dil, kind):
    _adacof_case(lib, 600 + Cc * 7 + Fs * 3 + dil, Cc, Fs, dil, kind)


def test_adacof_signed_and_wrapper(lib, ops):
    _adacof_case(lib, 700, 9, 3, 2, "rand", signed=True)
    x, w, oi, oj, out = _adacof_case(lib, 701, 17, 5, 1, "rand")
    assert torch.equal(ops.FunctionAdaCoF.apply(x, w, oi, oj, 1), out)


# ---- correlation --------------------------------------------------------------------------------------------------------------------

CORR = [(1, 1, 1), (7, 3, 40), (8, 8, 17), (9, 15, 16), (33, 16, 15), (9, 17, 3), (7, 40, 8), (33, 40, 1), (1, 16, 40)]


def _corr_case(lib, seed, Cc, H, W, N=3, signed=False):
    g = _gen(seed)
    make = (lambda s, g: torch.randn(*s, device=DEV, generator=g)) if signed else _pos
    a = _in_nan((N, Cc, H, W), 3, g, make)            # slices of NaN tensors: reads outside the image must not happen
    b = _in_nan((N, Cc, H, W), 5, g, make)
    out = torch.full((N, 81, H, W), NAN, device=DEV)
    _ck(lib.vfi_correlation81(a.data_ptr(), _st(a), b.data_ptr(), _st(b), out.data_ptr(), N, Cc, H, W, _stream()), "vfi_correlation81")
    want, M, mn = rs.correlation(a.cpu(), b.cpu(), min_term=True)
    _check(out, want, M, rs.gamma_correlation(Cc), f"correlation C{Cc} {H}x{W}", None if signed else mn)
    return a, b, out


@pytest.mark.parametrize("Cc,H,W", CORR)
def test_correlation_edges(lib, Cc, H, W):
    _corr_case(lib, 800 + Cc + H * 3 + W, Cc, H, W)


def test_correlation_signed_and_wrapper(lib, ops):
    _corr_case(lib, 900, 33, 17, 40, signed=True)
    a, b, out = _corr_case(lib, 901, 9, 16, 17)
    assert torch.equal(ops.FunctionCorrelation(a, b), out)


# ---- distance transform ----------------------------------------------------------------------------------------------------------

def _edt_direct(lib, data, diam2, tmp=None):
    N, H, W = data.shape
    tmp = torch.full_like(data, NAN) if tmp is None else tmp
    out = torch.full_like(data, NAN)
    _ck(lib.vfi_edt(data.data_ptr(), tmp.data_ptr(), out.data_ptr(), N, H, W, diam2, _stream()), "vfi_edt")
    return tmp, out


def _masks(h, w, g):
    """N = 3 per kind: empty (every pixel sqrt(diam2)), full, one pixel in a corner, random"""
    kinds = {"empty": torch.zeros(3, h, w, device=DEV), "full": torch.ones(3, h, w, device=DEV)}
    c = torch.zeros(3, h, w, device=DEV)
    c[0, 0, 0], c[1, h - 1, w - 1], c[2, 0, w - 1] = 1, 1, 1
    kinds["corner"] = c
    kinds["random"] = (torch.rand(3, h, w, device=DEV, generator=g) > 0.97).float()
    return kinds


EDT_SHAPES = [(1, 1), (1, 2), (2, 255), (255, 256), (256, 257), (257, 600), (600, 2), (600, 600), (2, 1)]


@pytest.mark.parametrize("h,w", EDT_SHAPES)
def test_edt_bit_exact(ops, h, w):
    g = _gen(1000 + h + w)
    for kind, m in _masks(h, w, g).items():
        got = ops.batch_edt(m).cpu()
        want = rs.batch_edt(m)
        assert torch.equal(got, want), f"edt {h}x{w} {kind}: {int((got != want).sum())} pixels differ"
    if h * w <= 256 * 257:       # a non-binary float mask: the fp32 emulation
        m = torch.rand(3, h, w, device=DEV, generator=g)
        got = ops.batch_edt(m).cpu()
        assert torch.equal(got, rs.batch_edt(m)), f"edt {h}x{w} non-binary"


def test_edt_first_pass_bit_exact(lib):
    """vfi_edt's tmp (the pass along rows) against the exact row pass, for a 0/1 mask and for non-binary data"""
    g = _gen(1100)
    m = (torch.rand(3, 257, 600, device=DEV, generator=g) > 0.99).float()
    data, diam2 = rs.edt_data(m)
    tmp, out = _edt_direct(lib, data, diam2)
    assert torch.equal(tmp.cpu(), rs.edt_rows_exact(m.cpu()).float())
    assert torch.equal(out.cpu(), rs.sqrt_rn(rs.edt_squared_exact(m.cpu()).float()))
    data = rs.edt_data(torch.rand(3, 37, 255, device=DEV, generator=g))[0]
    tmp, out = _edt_direct(lib, data, diam2)
    assert torch.equal(tmp.cpu(), rs.edt_rows_fp32(data.cpu(), diam2))
    assert torch.equal(out.cpu(), rs.edt_fp32(data.cpu(), diam2))


def test_edt_mask_dtypes(ops):
    g = _gen(1200)
    m = torch.rand(3, 30, 40, device=DEV, generator=g) > 0.95
    want = rs.batch_edt(m.float())                     # distances below 50: the uint8 cast is exact after truncation
    got_b = ops.batch_edt(m)
    assert got_b.dtype == torch.bool and torch.equal(got_b.cpu(), want != 0)
    got_u = ops.batch_edt(m.to(torch.uint8))
    assert got_u.dtype == torch.uint8 and torch.equal(got_u.cpu(), want.to(torch.uint8))
    got_4 = ops.batch_edt(m.float().unsqueeze(1))
    assert got_4.shape == (3, 1, 30, 40) and torch.equal(got_4[:, 0].cpu(), want)


@pytest.mark.parametrize("h,w", [(1, 16384), (16384, 1)])
def test_edt_longest_line(ops, h, w):
    """the LDS limit: lines of 16384 work (diam2 > 2^24, so the fp32 rounding of (p - j)^2 and of diam2 matters); 16385 is
    rejected"""
    g = _gen(1300)
    m = torch.zeros(2, h, w, device=DEV)
    flat = m.view(2, -1)
    flat[0, torch.randint(0, 16384, (5,), device=DEV, generator=g)] = 1
    got = ops.batch_edt(m).cpu()
    assert torch.equal(got, rs.batch_edt(m.cpu()))
    with pytest.raises(RuntimeError, match="16384"):
        ops.batch_edt(torch.zeros(1, h + (h > 1), w + (w > 1), device=DEV))


def test_edt_sqrt_exhaustive(lib):
    """vfi_edt on N images of 1 x 1 with data = v and diam2 = 2^25 returns the kernel's sqrt_rn(v): every integer below 2^24, then
    2^22 random non-negative float bit patterns below diam2, against the correctly rounded value.  Chunks of 2^22 images keep the
    grid (N * H workgroups of 256) below 2^32 threads."""
    chunk = 1 << 22
    diam2 = float(1 << 25)

    def run(v):
        got = torch.empty_like(v)
        for i in range(0, v.numel(), chunk):
            d = v[i:i + chunk].view(-1, 1, 1)
            got[i:i + chunk] = _edt_direct(lib, d, diam2)[1].view(-1)
        return got.cpu()

    v = torch.arange(0, 1 << 24, device=DEV, dtype=torch.int32).float()
    got, want = run(v), rs.sqrt_rn(v)
    assert torch.equal(got, want), f"sqrt_rn wrong for {int((got != want).sum())} integers, first {v.cpu()[got != want][:5].tolist()}"
    g = torch.Generator().manual_seed(1400)
    bits = torch.randint(0, 0x4C000000, (chunk,), generator=g, dtype=torch.int64).to(torch.int32)   # 0x4C000000 = bits of 2^25
    v = bits.view(torch.float32).to(DEV)
    got, want = run(v), rs.sqrt_rn(v)
    assert torch.equal(got, want), f"sqrt_rn wrong for {int((got != want).sum())} floats, first {v.cpu()[got != want][:5].tolist()}"
