"""Float64 restatements, error bounds, case tables, wrong restatements and the buffer harness for the kernels of csrc/gen_ops.hip
(avgpool2, upsample_nearest, resize_bilinear, warp_film, axpby / axpby4), csrc/ifrnet_ops.hip (ifrnet_prep, ifrnet_center,
conv7x7s2_prelu<64>, sigmoid, fill_items, resize_ratio, ifrnet_output) and the cooperative CBAM kernels of csrc/ifunet_fast.hip behind
vfi_channel_pool / vfi_cbam_gate / vfi_cbam_scale_compress / vfi_cbam_spatial.  No product code is imported: every op is the
mathematical function of the reference formula its kernel comment cites (film_arch.py, IFRNet_L_arch.py / IFRNet_S_arch.py,
IFUNet_arch.py:411-503), evaluated in float64 on the fp32 inputs.  U, E_EXP, SIGMOID_U, TINY, Buffers, compare, Case and the sampler
machinery (bilinear, local_spread, the position term) are those of tests/small_ops_restated.py; its module docstring states the
buffer rules and the form of the bounds (gamma U sum|terms|, samplers add R U (|p| + size - 1) per axis times the local spread).

R, the roundings of a kernel's coordinate chain:
  warp_film_kernel      R_FILM = 10    lin_ls (product, addition), flow * mul, W * 0.5, the division, the subtraction, + 1, * W, - 1, / 2
  resize_bilinear       R_SIZE = 6     in / out (vfi_resize_bilinear rounds the ratio itself), d + 0.5, the product, - 0.5, src - i0, 1 - l
  resize_ratio          R_RATIO = 5    the same without the division: the ratio is an input
  ifrnet_output_kernel  R_WARP = 7     small_ops_restated's count of the same chain (lin11 with its step, the division, the addition, + 1, * halfw)

Exact ops (torch.equal): upsample_nearest (torch's rule min(floor(dst * fl32(in / out)), in - 1) in float32), ifrnet_prep, fill_items, the
max outputs of channel_pool and cbam_scale_compress, the xs output of cbam_scale_compress (one product), and axpby / avgpool2, whose
kernels are written in __f*_rn intrinsics in a stated order: their fp32 result is the numpy-float32 evaluation in that order; both are
ALSO compared with float64 under the counted bound (3 roundings each).

WRONG RESTATEMENTS.  Every op takes `mut`, the name of one deliberate error in the restatement (MUTATIONS); NEGATIVE pairs each with the
cases it must fail on.  tests/test_gen_ops_restated_cpu.py asserts that right and wrong differ by more than both bounds together, the
device test that the kernel's result fails the wrong one.
"""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as Fn

from small_ops_restated import E_EXP, INF, NAN, SIGMOID_U, TINY, U, Buffers, Case, _pos_err, bilinear, compare  # noqa: F401

R_FILM, R_SIZE, R_RATIO, R_WARP = 10, 6, 5, 7
D53 = 2.0 ** -53


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _pos(g, *shape):
    return 0.5 + 0.5 * torch.rand(*shape, generator=g)


def _noise(g, *shape, s=1.0):
    return torch.randn(*shape, generator=g) * s


def _make(g, kind, *shape):
    return _pos(g, *shape) if kind == "pos" else _noise(g, *shape)


def _exact(buf, want, **kw):
    return dict(buf=buf, want=want.double(), tol=None, **kw)


def _poke(B, name, fn):
    """rewrites the whole [px, cs] body of a buffer on host and device (sentinels outside the window)"""
    b = B.b[name]
    fn(b.host[b.G:b.G + b.px * b.cs].view(b.px, b.cs))
    b.dev = b.host.clone().to(B.device)


def _sigmoid_tol(t, tol_t):
    """sigmoid(t) and its bound when t carries tol_t: the slope y (1 - y) grows by at most tol_t over the interval (|(y (1 - y))'| < 1);
    1 / (1 + expf(-t)) itself within SIGMOID_U U y; a saturated result may flush."""
    y = torch.sigmoid(t)
    return y, (y * (1 - y) + tol_t) * tol_t + SIGMOID_U * U * y + TINY


# ---------------------------------------------------------------------------------------------------------------- gen_ops.hip

def op_avgpool2(P, B):
    """F.avg_pool2d(2, 2) (film_arch.py:655-674), odd sizes floor: (((a + b) + c) + d) * 0.25 with a, b the upper row.  Three additions
    round, the product by 0.25 is exact: 3 U sum|terms| / 4.  The row / column an odd size drops holds NaN unless P.odd_finite."""
    g = _g(P.seed)
    x = _make(g, P.kind, P.N, P.H, P.W, P.C)
    if not getattr(P, "odd_finite", False):
        if P.H % 2:
            x[:, -1] = NAN
        if P.W % 2:
            x[:, :, -1] = NAN
    B.add("in", x.reshape(-1, P.C), cs=P.in_cs, off=P.in_off)
    Ho, Wo = P.H // 2, P.W // 2
    B.add("out", None, P.N * Ho * Wo, P.C, P.out_cs, P.out_off, role="out")
    r0 = 1 if P.mut == "odd row kept" else 0
    t = [x[:, r0 + dy:r0 + dy + 2 * Ho:2, dx:dx + 2 * Wo:2] for dy in (0, 1) for dx in (0, 1)]
    n = [v.numpy() for v in t]
    w32 = torch.from_numpy((((n[0] + n[1]) + n[2]) + n[3]) * np.float32(0.25))
    d = [v.double() for v in t]
    want, M = sum(d) / 4, sum(v.abs() for v in d) / 4
    args = [B.ptr("in"), P.in_cs, B.ptr("out"), P.out_cs, P.N, P.H, P.W, P.C]
    return [("vfi_avgpool2", args)], [_exact("out", w32), dict(buf="out", want=want, tol=3 * U * M, mn=torch.stack(d).abs().amin(0) / 4 if P.kind == "pos" and not P.mut else None)]


def nearest_index(n_in, n_out, mut=None):
    """torch's 'nearest' source index in float32: min(floor(dst * fl32(in / out)), in - 1)"""
    s = np.float32(n_in) / np.float32(n_out)
    v = np.arange(n_out, dtype=np.float32) * s
    i = np.rint(v) if mut == "round instead of floor" else np.floor(v)
    return torch.from_numpy(np.minimum(i.astype(np.int64), n_in - 1))


def nearest_disagreements(limit=64):
    """(in, out, dst) where the float32 rule and the rational floor(dst * in / out) differ"""
    out = []
    for n_in in range(1, limit + 1):
        for n_out in range(1, limit + 1):
            a = nearest_index(n_in, n_out).numpy()
            b = np.minimum(np.arange(n_out, dtype=np.int64) * n_in // n_out, n_in - 1)
            out += [(n_in, n_out, int(d)) for d in np.nonzero(a != b)[0]]
    return out


def op_upsample_nearest(P, B):
    """F.interpolate(size=, mode='nearest') (film_arch.py:286).  Exact."""
    x = _noise(_g(P.seed), P.N, P.Hi, P.Wi, P.C)
    B.add("in", x.reshape(-1, P.C), cs=P.in_cs, off=P.in_off)
    B.add("out", None, P.N * P.Ho * P.Wo, P.C, P.out_cs, P.out_off, role="out")
    iy, ix = nearest_index(P.Hi, P.Ho, P.mut), nearest_index(P.Wi, P.Wo, P.mut)
    want = x[:, iy][:, :, ix]
    return [("vfi_upsample_nearest", [B.ptr("in"), P.in_cs, B.ptr("out"), P.out_cs, P.N, P.Hi, P.Wi, P.Ho, P.Wo, P.C])], [_exact("out", want)]


def _resize(img, ry, rx, Ho, Wo, R, ac=False):
    """torch's bilinear source position max(ratio (d + 0.5) - 0.5, 0) (align_corners=False; its index and lambda guards are the border
    clamp) -> value, bound without the value roundings' factor, M, largest tap"""
    N, Hi, Wi, _ = img.shape
    dx, dy = torch.arange(Wo, dtype=torch.float64), torch.arange(Ho, dtype=torch.float64)
    if ac:
        sx, sy = dx * ((Wi - 1) / (Wo - 1) if Wo > 1 else 0.0), dy * ((Hi - 1) / (Ho - 1) if Ho > 1 else 0.0)
    else:
        sx, sy = (rx * (dx + 0.5) - 0.5).clamp_min(0), (ry * (dy + 0.5) - 0.5).clamp_min(0)
    px, py = sx.view(1, 1, -1).expand(N, Ho, Wo), sy.view(1, -1, 1).expand(N, Ho, Wo)
    out, M, big, D = bilinear(img, px, py, True)
    d = _pos_err(px, Wi, R, True) + _pos_err(py, Hi, R, True)
    assert float(d.max()) < 0.5
    return out, d.unsqueeze(-1) * D, M, big


def op_resize_bilinear(P, B):
    """F.interpolate(mul * v, size=, mode='bilinear') (film_arch.py:597,610,752): ratio in / out.  Value: the product with mul, the two
    weight products and additions per axis: 9 U M like vfi_resize_bilinear_ac."""
    g = _g(P.seed)
    img = _make(g, P.kind, P.N, P.Hi, P.Wi, P.C)
    B.add("in", img.reshape(-1, P.C), cs=P.in_cs, off=P.in_off)
    B.add("out", None, P.N * P.Ho * P.Wo, P.C, P.out_cs, P.out_off, role="out")
    mul = _f32(P.mul)
    if P.mut == "sign of mul dropped":
        mul = abs(mul)
    out, tp, M, big = _resize(img.double() * mul, P.Hi / P.Ho, P.Wi / P.Wo, P.Ho, P.Wo, R_SIZE, ac=P.mut == "align_corners=True")
    args = [B.ptr("in"), P.in_cs, B.ptr("out"), P.out_cs, P.N, P.Hi, P.Wi, P.Ho, P.Wo, P.C, C.c_float(P.mul)]
    return [("vfi_resize_bilinear", args)], [dict(buf="out", want=out, tol=tp + 9 * U * M, mn=big if P.kind == "pos" and not P.mut else None)]


def film_flow(g, N, H, W, kind):
    """[N, H, W, 2] = (dx, dy)"""
    if kind == "zero":
        return torch.zeros(N, H, W, 2)
    if kind == "sub":
        return _noise(g, N, H, W, 2, s=0.3)
    if kind == "far":                                   # +-30: every pixel is clamped, on all four sides over the image
        f = torch.full((N, H, W, 2), 30.0)
        f[:, ::2, :, 1] = -30.0
        f[:, :, ::2, 0] = -30.0
        return f
    f = torch.zeros(N, H, W, 2)                         # planted integer shifts, dx != dy, both signs
    f[..., 0], f[..., 1] = kind[0], kind[1]
    return f


def op_warp_film(P, B):
    """film_arch.warp :677-724 (grid_sample, border, align_corners=False) at pixel + flow * flow_mul.  In exact arithmetic
    linspace(-(1 - 1/W), 1 - 1/W, W)[x] + f / (W / 2) un-normalises to x + f.  Value: 8 U M as every sampler of the suite."""
    g = _g(P.seed)
    if P.kind == "ramp":                                # x + 10 y: the result names the displacement
        img = (torch.arange(P.W).view(1, 1, P.W, 1) + 10.0 * torch.arange(P.H).view(1, P.H, 1, 1)).expand(P.N, P.H, P.W, P.C).contiguous()
    else:
        img = _make(g, P.kind, P.N, P.H, P.W, P.C)
    fl = film_flow(g, P.N, P.H, P.W, P.flow)
    px_n = P.N * P.H * P.W
    B.add("in", img.reshape(px_n, P.C), cs=P.in_cs, off=P.in_off)
    B.add("flow", fl.reshape(px_n, 2), cs=P.flow_cs, off=P.flow_off)
    B.add("out", None, px_n, P.C, P.out_cs, P.out_off, role="out")
    fm = 1.0 if P.mut == "flow_mul omitted" else _f32(P.flow_mul)
    fx, fy = fl[..., 0].double() * fm, fl[..., 1].double() * fm
    if P.mut == "dx and dy exchanged":
        fx, fy = fy, fx
    if P.mut == "flow subtracted":
        fx, fy = -fx, -fy
    X, Y = torch.arange(P.W, dtype=torch.float64).view(1, 1, P.W), torch.arange(P.H, dtype=torch.float64).view(1, P.H, 1)
    px, py = X + fx, Y + fy + 0 * X
    if P.mut == "align_corners=True un-normalisation":  # ((g + 1) / 2) (W - 1) with g + 1 = (2 p + 1) / W
        px, py = (2 * px + 1) * (P.W - 1) / (2 * P.W), (2 * py + 1) * (P.H - 1) / (2 * P.H)
    border = P.mut != "zeros padding"
    out, M, big, D = bilinear(img.double(), px, py, border)
    d = _pos_err(px, P.W, R_FILM, border) + _pos_err(py, P.H, R_FILM, border)
    assert float(d.max()) < 0.5
    e = dict(buf="out", want=out, tol=d.unsqueeze(-1) * D + 8 * U * M, mn=big if P.kind == "pos" and not P.mut else None, px=px, py=py)
    args = [B.ptr("in"), P.in_cs, B.ptr("flow"), P.flow_cs, C.c_float(P.flow_mul), B.ptr("out"), P.out_cs, P.N, P.H, P.W, P.C]
    return [("vfi_warp_film", args)], [e]


def op_axpby(P, B):
    """alpha a + beta b (b may be absent): fl(fl(a alpha) + fl(b beta)), the kernels' stated order; float64: 3 U (|a alpha| + |b beta|).
    P.inplace: out is a (rife40.py:216-217, ifunet.py:225-238, gmfss.py:296 call it so; no caller passes out == b)."""
    g = _g(P.seed)
    a = _make(g, P.kind, P.px, P.C)
    b = _make(g, P.kind, P.px, P.C) if P.b else None
    B.add("a", a, cs=P.a_cs, off=P.a_off, role="inout" if P.inplace else "in")
    if P.b:
        B.add("b", b, cs=P.b_cs, off=P.b_off)
    if not P.inplace:
        B.add("out", None, P.px, P.C, P.out_cs, P.out_off, role="out")
    ob = "a" if P.inplace else "out"
    al, be = np.float32(P.alpha), np.float32(P.beta)
    if P.mut == "beta applied to a":
        al, be = be, al
    w32 = a.numpy() * al
    want, M = a.double() * float(al), (a.double() * float(al)).abs()
    if P.b:
        w32 = w32 + b.numpy() * be
        want, M = want + b.double() * float(be), M + (b.double() * float(be)).abs()
    args = [B.ptr("a"), P.a_cs, B.ptr("b") if P.b else None, P.b_cs if P.b else 0, B.ptr(ob), P.a_cs if P.inplace else P.out_cs, P.px, P.C,
            C.c_float(P.alpha), C.c_float(P.beta)]
    mn = torch.minimum((a.double() * float(al)).abs(), (b.double() * float(be)).abs()) if P.b and P.kind == "pos" and P.beta and not P.mut else None
    return [("vfi_axpby", args)], [_exact(ob, torch.from_numpy(w32)), dict(buf=ob, want=want, tol=3 * U * M, mn=mn)]


# ---------------------------------------------------------------------------------------------------------------- ifrnet_ops.hip

def op_ifrnet_prep(P, B):
    """F.pad of (frame.rgb, 0) into Hp x Wp (IFRNet_L_arch.py:230-235).  Exact; the frames' channels past 3 hold NaN."""
    g = _g(P.seed)
    fr = [_noise(g, P.H * P.W, P.C) for _ in range(2)]
    want = []
    for k, f in enumerate(fr):
        f[:, 3:] = NAN
        B.add(f"f{k}", f)
        B.add(f"out{k}", None, P.Hp * P.Wp, 4, role="out")
        w = torch.zeros(P.Hp, P.Wp, 4)
        w[:P.H, :P.W, :3] = f.view(P.H, P.W, P.C)[..., :3]
        want.append(_exact(f"out{k}", w))
    return [("vfi_ifrnet_prep", [B.ptr("f0"), B.ptr("f1"), P.C, P.H, P.W, B.ptr("out0"), B.ptr("out1"), P.Hp, P.Wp])], want


def op_ifrnet_center(P, B):
    """mean_ over both images and their 3 channels (:242-247) from the per-image channel means cm [2N][4], subtracted in place:
    m = (((a0 + a1) + a2) + ((b0 + b1) + b2)) / 6: five additions and the division, 6 U sum|cm| / 6; v - m one more rounding.
    The fourth channel of img holds 7.25 and must come back bit-identical (it lies outside the window)."""
    g = _g(P.seed)
    cm = _noise(g, 2 * P.N, 3, s=0.1 * P.scale) + P.scale
    img = _noise(g, 2 * P.N * P.px, 3, s=0.3 * P.scale) + P.scale
    B.add("img", img, cs=4, off=0, role="inout")
    _poke(B, "img", lambda v: v[:, 3].fill_(7.25))
    B.add("cm", cm, cs=4, off=0)
    B.add("mean", None, 1, P.N, cs=P.N + 5, off=3, role="out")
    c = cm.double()
    if P.mut == "mean over one image only":
        m, S = c[:P.N].sum(1) / 3, c[:P.N].abs().sum(1) / 3
    else:
        div = 8.0 if P.mut == "divided by 8" else 6.0
        m, S = (c[:P.N].sum(1) + c[P.N:].sum(1)) / div, (c[:P.N].abs().sum(1) + c[P.N:].abs().sum(1)) / div
    tm = 6 * U * S
    mm, tt = m.repeat(2).repeat_interleave(P.px).unsqueeze(1), tm.repeat(2).repeat_interleave(P.px).unsqueeze(1)
    want = img.double() - mm
    args = [B.ptr("img"), B.ptr("cm"), B.ptr("mean"), P.N, P.px]
    return [("vfi_ifrnet_center", args)], [dict(buf="img", want=want, tol=tt + U * want.abs()), dict(buf="mean", want=m.view(1, -1), tol=tm.view(1, -1))]


def conv7_inputs(P):
    g = _g(P.seed)
    x = torch.rand(P.N, 3, P.Hin, P.Win, generator=g) * 2 - 1
    w = (torch.rand(64, 3, 7, 7, generator=g) * 2 - 1) / 147 ** 0.5
    return x, w, torch.rand(64, generator=g) - 0.5, 0.1 + 0.3 * torch.rand(64, generator=g)


def op_conv7x7s2_prelu(P, B):
    """Conv2d(3, 64, 7, 2, 3) + PReLU(64) (Encoder, IFRNet_L_arch.py:128-130): 147 fused multiply-adds, the bias and the slope's product:
    tests/test_gpu_amt_g.py's bound for the 84-channel instantiation, 150 U M with M the convolution of the absolute values."""
    x, w, b, sl = conv7_inputs(P)
    B.add("in", x.permute(0, 2, 3, 1).reshape(-1, 3), cs=P.in_cs, off=0)
    B.add("w", w.permute(2, 3, 1, 0).reshape(-1, 64))
    B.add("bias", b.view(1, 64))
    B.add("slope", sl.view(1, 64))
    Ho, Wo = (P.Hin - 1) // 2 + 1, (P.Win - 1) // 2 + 1
    B.add("out", None, P.N * Ho * Wo, 64, P.out_cs, P.out_off, role="out")
    xd, wd, sd = x.double(), w.double().clone(), sl.double()
    if P.mut == "last tap dropped":
        wd[:, :, 6, 6] = 0
    if P.mut == "slope of channel c ^ 1":
        sd = sd.view(32, 2).flip(1).reshape(64)
    pl, ph = (2, 4) if P.mut == "padding 2" else (3, 3)
    pad = lambda t: Fn.pad(t, (pl, ph, pl, ph))
    pre = Fn.conv2d(pad(xd), wd, b.double(), 2)
    M = Fn.conv2d(pad(xd.abs()), wd.abs(), b.double().abs(), 2)
    want = Fn.prelu(pre, sd)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(-1, 64)
    args = [B.ptr("in"), P.in_cs, B.ptr("w"), B.ptr("bias"), B.ptr("slope"), 64, B.ptr("out"), P.out_cs, P.N, P.Hin, P.Win]
    return [("vfi_conv7x7s2_prelu", args)], [dict(buf="out", want=nhwc(want), tol=nhwc(150 * U * M), pre=pre)]


SIGMOID_PLANTED = (0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0)


def op_sigmoid(P, B):
    """torch.sigmoid (:278) in place on a channel window: SIGMOID_U U y; below 2^-126 the result may flush."""
    x = _noise(_g(P.seed), P.px, P.C, s=3.0)
    flat = x.view(-1)
    for i, v in enumerate(SIGMOID_PLANTED[:flat.numel()]):
        flat[(i * 37) % flat.numel()] = v
    B.add("x", x, cs=8, off=P.off, role="inout")
    y = torch.sigmoid(x.double())
    if P.mut == "tanh":
        y = torch.tanh(x.double())
    return [("vfi_sigmoid", [B.ptr("x"), 8, P.C, P.px])], [dict(buf="x", want=y, tol=SIGMOID_U * U * y.abs() + TINY)]


def op_fill_items(P, B):
    """embt.repeat(1, 1, h, w) (:160-163): item n's pixels hold value[n].  Exact."""
    vals = torch.rand(P.N, generator=_g(P.seed))
    B.add("out", None, P.N * P.ppi, P.C, P.C + 2, 1, role="out")
    want = vals.repeat_interleave(P.ppi).view(-1, 1).expand(-1, P.C)
    return [("vfi_fill_items", [B.ptr("out"), P.C + 2, P.C, P.N, P.ppi, (C.c_float * P.N)(*vals.tolist())])], [_exact("out", want)]


def op_resize_ratio(P, B):
    """resize() = F.interpolate(scale_factor=s, bilinear, align_corners=False) * post_mul (:38-41, 281-288): output floor(in * s), source
    ratio fl32(1 / s), an input.  Value 9 U M (post_mul is the ninth)."""
    g = _g(P.seed)
    Ho, Wo = int(math.floor(P.Hi * P.s)), int(math.floor(P.Wi * P.s))
    img = _make(g, P.kind, P.N, P.Hi, P.Wi, P.C)
    B.add("in", img.reshape(-1, P.C), cs=P.in_cs, off=P.in_off)
    B.add("out", None, P.N * Ho * Wo, P.C, P.out_cs, P.out_off, role="out")
    r = _f32(1.0 / P.s)
    ry, rx = (P.Hi / Ho, P.Wi / Wo) if P.mut == "ratio from the output size" else (r, r)
    pm = _f32(P.post_mul)
    out, tp, M, big = _resize(img.double(), ry, rx, Ho, Wo, R_RATIO)
    args = [B.ptr("in"), P.in_cs, B.ptr("out"), P.out_cs, P.N, P.Hi, P.Wi, Ho, Wo, P.C, C.c_float(r), C.c_float(r), C.c_float(P.post_mul)]
    e = dict(buf="out", want=out * pm, tol=(tp + 9 * U * M) * abs(pm), mn=big * abs(pm) if P.kind == "pos" and not P.mut else None)
    return [("vfi_resize_bilinear_ratio", args)], [e]


def op_ifrnet_output(P, B):
    """clamp(mask warp(img0, f0) + (1 - mask) warp(img1, f1) + mean_ + res, 0, 1)[:H, :W] (:290-294).  warp() builds its grid from the
    FLOW's size Hf x Wf and grid_sample un-normalises with the image's Hp x Wp (align_corners=True, border): position
    (X + fx) (Wp - 1) / (Wf - 1).  Each warp: sampler bound with R_WARP and 8 U M.  Blend: 1 - m (one rounding on the second term), two
    products, three additions: 4 U on every term.  The clamp is 1-Lipschitz.  The images' fourth channel holds NaN."""
    g = _g(P.seed)
    N, Hp, Wp, Hf, Wf, H, W = P.N, P.Hp, P.Wp, P.Hf, P.Wf, P.H, P.W
    imgs = [0.2 + 0.6 * torch.rand(N, Hp, Wp, 3, generator=g) for _ in range(2)]
    fin = torch.zeros(N, Hf, Wf, 8)
    if P.flow == "rand":
        fin[..., :4] = _noise(g, N, Hf, Wf, 4, s=4.0)
    elif P.flow == "far":
        fin[..., :4] = 40.0
        fin[:, ::2, :, 0:2] = -40.0
        fin[:, :, ::2, 2:4] = -40.0
    i = torch.arange(N * Hf * Wf).view(N, Hf, Wf)
    fin[..., 4] = torch.where(i % 3 == 0, torch.zeros(()), torch.where(i % 3 == 1, torch.ones(()), torch.rand(N, Hf, Wf, generator=g)))
    res = _noise(g, N, Hf, Wf, 3, s=0.05)
    res[(i % 4 == 1)] -= 2.0                            # the clamp binds at 0 ...
    res[(i % 4 == 2)] += 2.0                            # ... and at 1
    fin[..., 5:8] = res
    mean = 0.05 + 0.1 * torch.rand(N, generator=g)
    for k in range(2):
        B.add(f"img{k}", imgs[k].reshape(-1, 3), cs=4, off=0)
    B.add("fin", fin.reshape(-1, 8))
    B.add("mean", mean.view(1, N), cs=N + 2, off=1)
    B.add("out", None, N * H * W, 3, role="out")
    X, Y = torch.arange(Wf, dtype=torch.float64).view(1, 1, Wf), torch.arange(Hf, dtype=torch.float64).view(1, Hf, 1)
    kx, ky = ((Wp - 1) / (Wf - 1), (Hp - 1) / (Hf - 1)) if P.mut != "grid normalised with the image size" else (1.0, 1.0)
    wv, tw = [], []
    for k in range(2):
        px, py = (X + fin[..., 2 * k].double()) * kx, (Y + fin[..., 2 * k + 1].double() + 0 * X) * ky
        out, M, big, D = bilinear(imgs[k].double(), px, py, True)
        d = _pos_err(px, Wp, R_WARP, True) + _pos_err(py, Hp, R_WARP, True)
        assert float(d.max()) < 0.5
        wv.append(out)
        tw.append(d.unsqueeze(-1) * D + 8 * U * M)
    m = fin[..., 4:5].double()
    m0, m1 = (1 - m, m) if P.mut == "masks exchanged" else (m, 1 - m)
    mn_ = torch.zeros(N, 1, 1, 1, dtype=torch.float64) if P.mut == "mean omitted" else mean.double().view(N, 1, 1, 1)
    t0, t1, rs = m0 * wv[0], m1 * wv[1], fin[..., 5:8].double()
    pre = t0 + t1 + mn_ + rs
    tol = m0 * tw[0] + m1 * tw[1] + U * m1 * wv[1].abs() + 4 * U * (t0.abs() + t1.abs() + mn_.abs() + rs.abs())
    want = pre if P.mut == "no clamp" else pre.clamp(0, 1)
    crop = lambda t: t[:, :H, :W]
    args = [B.ptr("img0"), B.ptr("img1"), B.ptr("fin"), B.ptr("mean"), B.ptr("out"), N, Hp, Wp, Hf, Wf, H, W]
    return [("vfi_ifrnet_output", args)], [dict(buf="out", want=crop(want), tol=crop(tol), pre=crop(pre))]


# ---------------------------------------------------------------------------------------------------------------- ifunet_fast.hip (CBAM)

def pool_strips(ws_bytes, N, Cc):
    """vfi_channel_pool's strip rule: as many as the workspace holds, 64 (refused below) .. 128"""
    per = N * Cc * 12
    return min(ws_bytes // per, 128), per


def op_channel_pool(P, B):
    """ChannelGate's avg_pool2d / max_pool2d over the whole image (IFUNet_arch.py:411-452) -> stats [N][C][2] = (mean, max).  The maximum
    is exact.  The mean is summed in float64 in some order (each of at most HW - 1 additions rounds by 2^-53 of a partial sum) and rounded
    to fp32 once: U |mean| + (HW + 1) 2^-53 mean|v|.  The workspace is a byte buffer: its window is what min(strips, 128) strips use."""
    g = _g(P.seed)
    x = (_pos(g, P.N, P.HW, P.C) if P.kind == "pos" else _noise(g, P.N, P.HW, P.C, s=P.sigma)) + P.mean
    B.add("x", x.reshape(-1, P.C), cs=P.C + 8, off=3)
    B.add("stats", None, P.N * P.C, 2, role="out")
    strips, per = pool_strips(P.ws_bytes, P.N, P.C)
    B.add("ws", None, -(-P.ws_bytes // 4), 1, role="scratch")
    if strips >= 64:
        w = B.b["ws"]
        w.win[w.G + strips * per // 4:] = False          # bytes past what the strips use must come back untouched
    xd = x.double()
    if P.mut == "mean over per * strips":
        mean = xd.sum(1) / (-(-P.HW // strips) * strips)
    else:
        mean = xd.mean(1)
    mx = xd.abs().amax(1) if P.mut == "max of absolute values" else xd.amax(1)
    tol = U * mean.abs() + (P.HW + 1) * D53 * xd.abs().mean(1)
    args = [B.ptr("x"), P.C + 8, P.C, P.N, P.HW, B.ptr("stats"), B.ptr("ws"), P.ws_bytes]
    mn = xd.abs().amin(1) / P.HW if P.kind == "pos" and not P.mut else None
    return [("vfi_channel_pool", args)], [dict(buf="stats", cols=0, want=mean.reshape(-1, 1), tol=tol.reshape(-1, 1), mn=None if mn is None else mn.reshape(-1, 1)),
                                          _exact("stats", mx.reshape(-1, 1), cols=1)]


def op_cbam_gate(P, B):
    """sigmoid(mlp(avg) + mlp(max)), mlp = Linear(C, R) -> ReLU -> Linear(R, C) (:419-452).  Hidden unit: C products and additions in any
    order and the bias: (C + 2) U (|b1| + sum|w1 v|); ReLU is 1-Lipschitz.  Output: sum_r |w2| tol_h + (R + 2) U (|b2| + sum|w2 h|); the
    two branches' sum one more rounding; then _sigmoid_tol."""
    g = _g(P.seed)
    st = _noise(g, P.N, P.C, 2)
    w1, b1 = _noise(g, P.R, P.C) / P.C ** 0.5, _noise(g, P.R, s=0.1)
    w2, b2 = _noise(g, P.C, P.R) / P.R ** 0.5, _noise(g, P.C, s=0.1)
    for nm, t in (("stats", st.reshape(-1, 2)), ("w1", w1), ("b1", b1.view(1, -1)), ("w2", w2), ("b2", b2.view(1, -1))):
        B.add(nm, t)
    B.add("scale", None, P.N, P.C, role="out")
    v = st.double().permute(0, 2, 1)                                                         # [N, 2, C]
    hp = v @ w1.double().t() + b1.double()                                                   # [N, 2, R]
    th = (P.C + 2) * U * (v.abs() @ w1.double().abs().t() + b1.double().abs())
    h = hp if P.mut == "no ReLU" else hp.clamp_min(0)
    o = h @ w2.double().t() + b2.double()                                                    # [N, 2, C]
    to = th @ w2.double().abs().t() + (P.R + 2) * U * (h.abs() @ w2.double().abs().t() + b2.double().abs())
    if P.mut == "sigmoid per branch then summed":
        y, tol = torch.sigmoid(o).sum(1), to.sum(1)
    else:
        att = o.sum(1)
        y, tol = _sigmoid_tol(att, to.sum(1) + U * att.abs())
    args = [B.ptr("stats"), B.ptr("w1"), B.ptr("b1"), B.ptr("w2"), B.ptr("b2"), P.C, P.R, P.N, B.ptr("scale")]
    return [("vfi_cbam_gate", args)], [dict(buf="scale", want=y, tol=tol, hid=hp, hid_tol=th)]


def op_cbam_scale_compress(P, B):
    """xs = x * scale[n][c] (one product: exact); comp = (max_c xs, mean_c xs) (:451-466): the maximum of the fp32 products is exact, the
    mean C - 1 fp32 additions in any order and the division: (C + 1) U mean|xs|."""
    g = _g(P.seed)
    x = _make(g, P.kind, P.N * P.HW, P.C)
    sc = 0.2 + 0.8 * torch.rand(P.N, P.C, generator=g)
    B.add("x", x, cs=P.C + 4, off=2)
    B.add("scale", sc)
    B.add("xs", None, P.N * P.HW, P.C, P.C + 7, 3, role="out")
    B.add("comp", None, P.N * P.HW, 2, role="out")
    scp = sc.repeat_interleave(P.HW, 0)
    xs = (x.double() * scp.double()).float()
    xd = xs.double()
    mean = xd.sum(1) / ((P.C + 4) if P.mut == "mean over cs" else P.C)
    if P.mut == "max before scaling":
        j = x.argmax(1, keepdim=True)
        mx = xd.gather(1, j)
    else:
        mx = xd.amax(1, keepdim=True)
    args = [B.ptr("x"), P.C + 4, B.ptr("scale"), P.C, P.N, P.HW, B.ptr("xs"), P.C + 7, B.ptr("comp")]
    mn = xd.abs().amin(1, keepdim=True) / P.C if P.kind == "pos" and not P.mut else None
    return [("vfi_cbam_scale_compress", args)], [_exact("xs", xs), _exact("comp", mx, cols=0),
                                                 dict(buf="comp", cols=1, want=mean.view(-1, 1), tol=(P.C + 1) * U * xd.abs().mean(1, keepdim=True), mn=mn)]


def op_cbam_spatial(P, B):
    """SpatialGate (:469-482): xs *= sigmoid(bn_a conv7x7(comp) + bn_b), in place on a channel window.  s: up to 98 products and additions
    in any order: 99 U sum|q w|; bn_a s + bn_b two roundings; _sigmoid_tol; the product one rounding."""
    g = _g(P.seed)
    xs = _noise(g, P.N * P.H * P.W, P.C)
    comp = _noise(g, P.N, P.H, P.W, 2)
    w = _noise(g, 7, 7, 2, s=0.1)
    B.add("xs", xs, cs=P.C + 5, off=2, role="inout")
    B.add("comp", comp.reshape(-1, 2))
    B.add("w", w.reshape(-1, 2))
    a, b = _f32(P.bn_a), _f32(P.bn_b)
    wd = w.double().permute(2, 0, 1)[None]
    if P.mut == "tap order transposed":
        wd = wd.transpose(2, 3)
    cd = comp.double().permute(0, 3, 1, 2)
    s = Fn.conv2d(cd, wd, padding=3)[:, 0]
    ts = 99 * U * Fn.conv2d(cd.abs(), wd.abs(), padding=3)[:, 0]
    bb = 0.0 if P.mut == "gate without bn_b" else b
    t = s * a + bb
    gate, tg = _sigmoid_tol(t, abs(a) * ts + 2 * U * ((s * a).abs() + abs(bb)))
    gate, tg = gate.reshape(-1, 1), tg.reshape(-1, 1)
    want = xs.double() * gate
    args = [B.ptr("xs"), P.C + 5, B.ptr("comp"), B.ptr("w"), C.c_float(P.bn_a), C.c_float(P.bn_b), P.C, P.N, P.H, P.W]
    return [("vfi_cbam_spatial", args)], [dict(buf="xs", want=want, tol=xs.double().abs() * tg + U * want.abs())]


OPS = {k[3:]: v for k, v in list(globals().items()) if k.startswith("op_")}


# ---------------------------------------------------------------------------------------------------------------- runner

def _build(case, mut, device):
    B = Buffers(device)
    calls, expects = OPS[case.op](SimpleNamespace(**{"kind": "noise", **case.p, "mut": mut}), B)
    return B, calls, expects


def expectation(case, mut=None):
    return _build(case, mut, "cpu")[2]


def _rc(rc, name):
    assert rc == 0, f"{name} -> {rc}"


def run_case(lib, case, device="cpu", stream=None, sync=None, check=_rc, mut=None):
    """builds the buffers on `device`, calls the entry point of `lib`, synchronises once, checks guards, inputs and results against the
    restatement (the wrong one named by `mut`).  -> largest err / tol of the case (0.0 for an exact one)"""
    B, calls, expects = _build(case, mut, device)
    for name, args in calls:
        check(getattr(lib, name)(*args, stream), name)
    if sync is not None:
        sync()
    outs = B.finish()
    worst = 0.0
    for e in expects:
        got = outs[e["buf"]]
        if e.get("cols") is not None:
            got = got[:, e["cols"]:e["cols"] + 1]
        worst = max(worst, _compare(got, e, f"{case.id}:{e['buf']}") or 0.0)
    return worst


def _compare(got, e, what):
    """small_ops_restated.compare; an exact expectation is a bound of zero and fails in the same words as a toleranced one"""
    if e["tol"] is not None:
        return compare(got, e, what)
    w32 = e["want"].reshape(got.shape).float()
    bad = ~(got == w32)
    if bad.any():
        i = tuple(int(k) for k in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound (zero: the result is exact); first at {i}: got {got[i].item()!r} "
                             f"want {w32[i].item()!r}")
    return None


# ---------------------------------------------------------------------------------------------------------------- case tables

def _w(d, **names):
    for nm, (cs, off) in names.items():
        d[nm + "_cs"], d[nm + "_off"] = cs, off
    return d


# vfi_avgpool2: N Ho Wo C/4 threads of 256.  3x3: the dropped row and column hold NaN.  130 and 1548 threads: below a block, a tail block
AVGPOOL_CASES = [Case("avgpool2", tag, seed=1, N=n, H=h, W=w, C=c, kind=kind, **_w({}, **win))
                 for tag, n, h, w, c, kind, win in (
                     ("2x2-c4-dense", 1, 2, 2, 4, "noise", {"in": (4, 0), "out": (4, 0)}),
                     ("3x3-c4-window-nan-edge", 1, 3, 3, 4, "noise", {"in": (12, 4), "out": (8, 4)}),
                     ("n2-5x9-c8-odd-h", 2, 5, 9, 8, "pos", {"in": (12, 4), "out": (8, 0)}),
                     ("4x130-c4-n130", 1, 4, 130, 4, "noise", {"in": (12, 4), "out": (8, 4)}),
                     ("6x344-c12-n1548-tail", 1, 6, 344, 12, "noise", {"in": (12, 0), "out": (12, 0)}))]
AVGPOOL_NEG = Case("avgpool2", "n2-5x9-c8-odd-finite", seed=1, N=2, H=5, W=9, C=8, kind="pos", odd_finite=True, **_w({}, **{"in": (12, 4), "out": (8, 0)}))

NEAREST_SHAPES = [(1, 1, 1, 3, 5, 4), (1, 2, 3, 4, 6, 4), (1, 3, 5, 7, 11, 4), (1, 5, 7, 3, 4, 12), (1, 4, 4, 4, 4, 4), (2, 3, 5, 7, 11, 12)]
NEAREST_EXTRA = []          # size pairs where torch's float32 rule leaves the rational one (nearest_disagreements): filled below
NEAREST_CASES = [Case("upsample_nearest", f"n{n}-{hi}x{wi}to{ho}x{wo}-c{c}", seed=2, N=n, Hi=hi, Wi=wi, Ho=ho, Wo=wo, C=c, **_w({}, **{"in": (c + 4, 4), "out": (c + 8, 4)}))
                 for n, hi, wi, ho, wo, c in NEAREST_SHAPES]

BIL_WIN = _w({}, **{"in": (5, 1), "out": (4, 1)})
BILINEAR_CASES = [Case("resize_bilinear", f"n{n}-{hi}x{wi}to{ho}x{wo}-c{c}-mul{mul}-{kind}", seed=3, N=n, Hi=hi, Wi=wi, Ho=ho, Wo=wo, C=c, mul=mul, kind=kind,
                       **(BIL_WIN if c <= 3 else _w({}, **{"in": (c, 0), "out": (c, 0)})))
                  for n, hi, wi, ho, wo, c, mul, kind in (
                      (1, 1, 1, 4, 4, 1, 2.0, "noise"), (1, 2, 2, 4, 4, 2, 2.0, "pos"), (1, 3, 5, 6, 10, 3, 1.0, "noise"), (2, 4, 7, 9, 13, 2, 2.0, "pos"),
                      (1, 9, 13, 4, 7, 3, -1.5, "noise"), (1, 5, 5, 5, 5, 5, 1.0, "noise"), (2, 9, 13, 19, 27, 2, -1.5, "noise"))]      # the last: 1026 pixels, a tail block

FILM_WIN = dict(in_cs=16, in_off=4, out_cs=20, out_off=8)
FILM_CASES = []
for tag, n, h, w, c in (("2x2-c4", 1, 2, 2, 4), ("3x5-c12", 1, 3, 5, 12), ("9x16-c4", 1, 9, 16, 4), ("n2-5x7-c4", 2, 5, 7, 4)):
    for fl, fm, (fcs, foff) in (("zero", 1.0, (2, 0)), ("sub", 0.5, (4, 1)), ("far", 1.0, (2, 0))):
        FILM_CASES.append(Case("warp_film", f"{tag}-{fl}-mul{fm}", seed=4, N=n, H=h, W=w, C=c, kind="pos" if fl == "sub" else "noise", flow=fl, flow_mul=fm,
                               flow_cs=fcs, flow_off=foff, **FILM_WIN))
FILM_PLANTED = [Case("warp_film", f"9x16-c4-planted{dx:+d}{dy:+d}-mul{fm}", seed=4, N=1, H=9, W=16, C=4, kind="ramp", flow=(dx, dy), flow_mul=fm, flow_cs=4, flow_off=1, **FILM_WIN)
                for dx, dy, fm in ((2, -1, 1.0), (-3, 1, 1.0), (4, -2, 0.5), (-2, 6, 0.5))]
FILM_CASES += FILM_PLANTED

# vfi_axpby: float4 form while C % 4 == 0, every stride % 4 == 0 and every pointer 16-byte aligned; else the scalar form
_AB = ((0.5, 2.0), (1.0, -1.0), (-0.25, 0.0))
AXPBY_CASES = []
for i, (tag, px, c, acs, aoff, bcs, boff, ocs, ooff) in enumerate((
        ("v4-px1-c4", 1, 4, 8, 4, 4, 0, 12, 8), ("v4-px65-c4", 65, 4, 8, 4, 8, 0, 4, 0), ("v4-px257-c8", 257, 8, 12, 4, 8, 0, 16, 4),
        ("scalar-c1", 300, 1, 3, 1, 2, 0, 4, 2), ("scalar-c3", 85, 3, 5, 1, 4, 0, 3, 0), ("scalar-c5", 52, 5, 8, 0, 8, 3, 8, 1),
        ("scalar-c4-a-off1", 65, 4, 8, 1, 8, 0, 8, 0), ("scalar-c4-a_cs6", 65, 4, 6, 0, 8, 0, 8, 0), ("scalar-c4-b_cs6", 65, 4, 8, 0, 6, 0, 8, 0))):
    al, be = _AB[i % 3]
    AXPBY_CASES.append(Case("axpby", tag, seed=5, px=px, C=c, kind="pos", b=True, inplace=False, alpha=al, beta=be, **_w({}, a=(acs, aoff), b=(bcs, boff), out=(ocs, ooff))))
AXPBY_CASES += [
    Case("axpby", "v4-px65-c4-b-null", seed=5, px=65, C=4, b=False, inplace=False, alpha=0.5, beta=2.0, **_w({}, a=(8, 4), b=(0, 0), out=(4, 0))),
    Case("axpby", "scalar-c3-b-null", seed=5, px=85, C=3, b=False, inplace=False, alpha=-0.25, beta=0.0, **_w({}, a=(5, 1), b=(0, 0), out=(4, 1))),
    Case("axpby", "v4-px257-c4-inplace-a", seed=5, px=257, C=4, kind="pos", b=True, inplace=True, alpha=1.0, beta=-1.0, **_w({}, a=(8, 4), b=(4, 0), out=(0, 0))),
    Case("axpby", "scalar-c1-inplace-a", seed=5, px=300, C=1, kind="pos", b=True, inplace=True, alpha=0.5, beta=2.0, **_w({}, a=(8, 7), b=(1, 0), out=(0, 0)))]

PREP_CASES = [Case("ifrnet_prep", f"c{c}-{h}x{w}to{hp}x{wp}", seed=6, C=c, H=h, W=w, Hp=hp, Wp=wp)
              for c, h, w, hp, wp in ((3, 1, 1, 1, 1), (3, 5, 7, 8, 8), (4, 5, 7, 5, 7), (5, 3, 300, 4, 320))]
CENTER_CASES = [Case("ifrnet_center", f"n{n}-px{px}-scale{sc}", seed=7, N=n, px=px, scale=sc)
                for n, px, sc in ((1, 1, 0.5), (2, 255, 0.5), (3, 257, 1000.0), (1, 257, 0.5), (2, 1, 1000.0))]
CONV7_CASES = [Case("conv7x7s2_prelu", f"n{n}-{h}x{w}-in_cs{ics}", seed=8, N=n, Hin=h, Win=w, in_cs=ics, out_cs=72, out_off=4)
               for n, h, w, ics in ((1, 1, 1, 4), (1, 2, 3, 8), (2, 7, 9, 4), (1, 13, 20, 8), (1, 31, 33, 4))]
SIGMOID_CASES = [Case("sigmoid", f"c{c}-n{px * c}", seed=9, C=c, px=px, off=off) for c, px, off in ((1, 1, 2), (1, 255, 0), (1, 258, 7), (3, 85, 1), (3, 86, 5), (5, 51, 2))]
FILL_CASES = [Case("fill_items", f"n{n}-c{c}-ppi{ppi}", seed=10, N=n, C=c, ppi=ppi) for n, c, ppi in ((1, 1, 1), (3, 2, 129), (64, 1, 300), (64, 2, 1), (3, 1, 300))]

RATIO_CASES = []
for si, s in enumerate((0.5, 0.75, 1 / 0.75, 2.0, 4.0, 1.0)):
    for ii, (hi, wi) in enumerate(((8, 12), (7, 9), (3, 3), (1, 1))):
        if int(math.floor(hi * s)) < 1:
            continue
        c = (1, 3, 5)[(si + ii) % 3]
        RATIO_CASES.append(Case("resize_ratio", f"s{s:.4g}-{hi}x{wi}-c{c}", seed=11, N=1 + (si + ii) % 2, Hi=hi, Wi=wi, s=s, C=c, post_mul=(1.5, 1.0)[(si + ii) % 2],
                                kind=("pos", "noise")[ii % 2], **(BIL_WIN if c <= 3 else _w({}, **{"in": (7, 1), "out": (6, 1)}))))

OUTPUT_SHAPES = ((1, 2, 2, 2, 2, 2, 2), (2, 8, 16, 8, 16, 5, 11), (1, 8, 16, 7, 15, 5, 11), (1, 8, 16, 8, 16, 8, 16), (1, 32, 32, 32, 32, 17, 17))
OUTPUT_CASES = [Case("ifrnet_output", f"n{n}-img{hp}x{wp}-flow{hf}x{wf}-crop{h}x{w}-{fl}", seed=12, N=n, Hp=hp, Wp=wp, Hf=hf, Wf=wf, H=h, W=w, flow=fl)
                for i, (n, hp, wp, hf, wf, h, w) in enumerate(OUTPUT_SHAPES) for fl in (("zero", "rand", "far") if i in (1, 2) else (("rand", "far", "zero")[i % 3],))]

# vfi_channel_pool: chan_pool_partial_wg_kernel while C <= 256 (256 / C pixel lanes; C = 96: 64 idle lanes), else the body; a strip holds
# ceil(HW / strips) pixels, so HW = 1 leaves every strip but one empty
def _pool(tag, n, hw, c, strips, kind="noise", mean=0.0, sigma=1.0, short=0):
    return Case("channel_pool", tag, seed=13, N=n, HW=hw, C=c, kind=kind, mean=mean, sigma=sigma, ws_bytes=strips * n * c * 12 - short)


POOL_CASES = [_pool("c1-hw1000-strips64", 1, 1000, 1, 64, "pos"), _pool("c17-hw63-strips100", 2, 63, 17, 100), _pool("c32-hw64-strips64", 1, 64, 32, 64, "pos"),
              _pool("c96-hw129-strips64-idle-lanes", 2, 129, 96, 64), _pool("c96-hw1-strips100-empty-strips", 1, 1, 96, 100), _pool("c256-hw129-strips200-capped", 1, 129, 256, 200),
              _pool("c256-hw1-strips64", 2, 1, 256, 64), _pool("c257-hw63-strips64-body", 1, 63, 257, 64), _pool("c257-hw1000-strips200-body-capped", 1, 1000, 257, 200),
              _pool("c17-hw1000-mean1000-sigma0.01", 2, 1000, 17, 64, mean=1000.0, sigma=0.01), _pool("c1-hw1-strips64", 1, 1, 1, 64)]
POOL_REFUSED = _pool("c17-one-byte-short", 1, 63, 17, 64, short=1)

GATE_CASES = [Case("cbam_gate", f"n{n}-c{c}-r{r}" + ("-body" if r > 64 else ""), seed=14 + c + r, N=n, C=c, R=r)
              for n, c, r in ((1, 1, 1), (1, 17, 2), (2, 32, 2), (1, 96, 6), (3, 256, 16), (1, 64, 64), (1, 64, 65))]
SCALE_CASES = [Case("cbam_scale_compress", f"c{c}-hw{hw}-{kind}", seed=15, N=2, C=c, HW=hw, kind=kind)
               for c, hw, kind in ((1, 1, "noise"), (2, 63, "pos"), (17, 65, "noise"), (64, 517, "noise"), (96, 63, "pos"), (96, 1, "noise"), (256, 65, "noise"), (1, 517, "noise"))]
SPATIAL_CASES = [Case("cbam_spatial", f"n{n}-c{c}-{h}x{w}", seed=16, N=n, C=c, H=h, W=w, bn_a=0.8, bn_b=-0.1)
                 for n, c, h, w in ((1, 1, 1, 1), (1, 17, 3, 5), (2, 32, 7, 7), (1, 96, 8, 9), (1, 256, 4, 4))]

for _hi, _ho in sorted({(a, b) for a, b, _ in nearest_disagreements()})[:2]:
    NEAREST_EXTRA.append(Case("upsample_nearest", f"fp32-rule-{_hi}to{_ho}", seed=2, N=1, Hi=_hi, Wi=_hi, Ho=_ho, Wo=_ho, C=4, **_w({}, **{"in": (8, 4), "out": (4, 0)})))
NEAREST_CASES += NEAREST_EXTRA

TABLES = dict(avgpool2=AVGPOOL_CASES, upsample_nearest=NEAREST_CASES, resize_bilinear=BILINEAR_CASES, warp_film=FILM_CASES, axpby=AXPBY_CASES,
              ifrnet_prep=PREP_CASES, ifrnet_center=CENTER_CASES, conv7x7s2_prelu=CONV7_CASES, sigmoid=SIGMOID_CASES, fill_items=FILL_CASES,
              resize_ratio=RATIO_CASES, ifrnet_output=OUTPUT_CASES, channel_pool=POOL_CASES, cbam_gate=GATE_CASES, cbam_scale_compress=SCALE_CASES,
              cbam_spatial=SPATIAL_CASES)
ALL_CASES = [c for t in TABLES.values() for c in t]
HOST_CASES = POOL_CASES + GATE_CASES + SCALE_CASES + SPATIAL_CASES          # the four CBAM entry points exist in the host build (tests/hostcheck)
_by = {c.id: c for c in ALL_CASES}


def _ids(op, *tags):
    return [_by[f"{op}-{t}"] for t in tags]


# wrong restatement -> the cases it must fail on
MUTATIONS = {
    "odd row kept": [AVGPOOL_NEG],
    "round instead of floor": _ids("upsample_nearest", "n1-3x5to7x11-c4", "n1-5x7to3x4-c12"),
    "align_corners=True": _ids("resize_bilinear", "n1-3x5to6x10-c3-mul1.0-noise", "n2-4x7to9x13-c2-mul2.0-pos"),
    "sign of mul dropped": _ids("resize_bilinear", "n1-9x13to4x7-c3-mul-1.5-noise", "n2-9x13to19x27-c2-mul-1.5-noise"),
    "dx and dy exchanged": FILM_PLANTED,
    "flow subtracted": FILM_PLANTED + _ids("warp_film", "9x16-c4-sub-mul0.5"),
    "zeros padding": _ids("warp_film", "9x16-c4-far-mul1.0", "3x5-c12-far-mul1.0"),
    "align_corners=True un-normalisation": _ids("warp_film", "9x16-c4-zero-mul1.0", "n2-5x7-c4-sub-mul0.5"),
    "flow_mul omitted": FILM_PLANTED[2:] + _ids("warp_film", "9x16-c4-sub-mul0.5"),
    "beta applied to a": _ids("axpby", "v4-px65-c4", "scalar-c3", "v4-px257-c4-inplace-a"),
    "mean over one image only": _ids("ifrnet_center", "n2-px255-scale0.5", "n3-px257-scale1000.0"),
    "divided by 8": _ids("ifrnet_center", "n2-px255-scale0.5", "n1-px1-scale0.5"),
    "padding 2": _ids("conv7x7s2_prelu", "n2-7x9-in_cs4", "n1-13x20-in_cs8"),
    "last tap dropped": _ids("conv7x7s2_prelu", "n2-7x9-in_cs4", "n1-13x20-in_cs8"),
    "slope of channel c ^ 1": _ids("conv7x7s2_prelu", "n1-1x1-in_cs4", "n1-31x33-in_cs4"),
    "tanh": _ids("sigmoid", "c1-n255"),
    "ratio from the output size": _ids("resize_ratio", "s0.75-7x9-c5"),
    "grid normalised with the image size": _ids("ifrnet_output", "n1-img8x16-flow7x15-crop5x11-rand", "n1-img8x16-flow7x15-crop5x11-zero"),
    "masks exchanged": _ids("ifrnet_output", "n2-img8x16-flow8x16-crop5x11-rand", "n1-img2x2-flow2x2-crop2x2-rand"),
    "mean omitted": _ids("ifrnet_output", "n2-img8x16-flow8x16-crop5x11-zero", "n1-img32x32-flow32x32-crop17x17-far"),
    "no clamp": _ids("ifrnet_output", "n2-img8x16-flow8x16-crop5x11-far", "n1-img8x16-flow8x16-crop8x16-rand"),
    "mean over per * strips": _ids("channel_pool", "c1-hw1000-strips64", "c17-hw63-strips100"),
    "max of absolute values": _ids("channel_pool", "c96-hw129-strips64-idle-lanes", "c257-hw63-strips64-body"),
    "sigmoid per branch then summed": _ids("cbam_gate", "n1-c17-r2", "n3-c256-r16"),
    "no ReLU": _ids("cbam_gate", "n1-c96-r6", "n1-c64-r65-body"),
    "mean over cs": _ids("cbam_scale_compress", "c2-hw63-pos", "c96-hw63-pos"),
    "max before scaling": _ids("cbam_scale_compress", "c17-hw65-noise", "c256-hw65-noise"),
    "tap order transposed": _ids("cbam_spatial", "n2-c32-7x7", "n1-c96-8x9"),
    "gate without bn_b": _ids("cbam_spatial", "n1-c1-1x1", "n1-c256-4x4"),
}
NEGATIVE = [(c, m) for m, cs in MUTATIONS.items() for c in cs]


# refusals: (entry point, why, arguments builder taking two aligned device / host pointers p, q) — nothing is launched
def refusals(p, q):
    f = C.c_float
    return [
        ("vfi_avgpool2", "N = 0", [p, 4, q, 4, 0, 4, 4, 4]), ("vfi_avgpool2", "in_cs < C", [p, 4, q, 8, 1, 4, 4, 8]), ("vfi_avgpool2", "out_cs < C", [p, 8, q, 4, 1, 4, 4, 8]),
        ("vfi_avgpool2", "C = 0", [p, 4, q, 4, 1, 4, 4, 0]), ("vfi_avgpool2", "input window off by one float", [p + 4, 8, q, 4, 1, 4, 4, 4]),
        ("vfi_avgpool2", "output window off by two floats", [p, 4, q + 8, 8, 1, 4, 4, 4]),
        ("vfi_upsample_nearest", "N = 0", [p, 4, q, 4, 0, 2, 2, 4, 4, 4]), ("vfi_upsample_nearest", "Hin = 0", [p, 4, q, 4, 1, 0, 2, 4, 4, 4]),
        ("vfi_upsample_nearest", "Wout = 0", [p, 4, q, 4, 1, 2, 2, 4, 0, 4]), ("vfi_upsample_nearest", "Hout < 0", [p, 4, q, 4, 1, 2, 2, -1, 4, 4]),
        ("vfi_upsample_nearest", "in_cs < C", [p, 4, q, 8, 1, 2, 2, 4, 4, 8]), ("vfi_upsample_nearest", "out_cs < C", [p, 8, q, 4, 1, 2, 2, 4, 4, 8]),
        ("vfi_upsample_nearest", "input window off by one float", [p + 4, 8, q, 4, 1, 2, 2, 4, 4, 4]),
        ("vfi_upsample_nearest", "output window off by one float", [p, 4, q + 4, 8, 1, 2, 2, 4, 4, 4]),
        ("vfi_resize_bilinear", "N = 0", [p, 2, q, 2, 0, 2, 2, 4, 4, 2, f(1.0)]), ("vfi_resize_bilinear", "Win = 0", [p, 2, q, 2, 1, 2, 0, 4, 4, 2, f(1.0)]),
        ("vfi_resize_bilinear", "Hout = 0", [p, 2, q, 2, 1, 2, 2, 0, 4, 2, f(1.0)]), ("vfi_resize_bilinear", "in_cs < C", [p, 1, q, 2, 1, 2, 2, 4, 4, 2, f(1.0)]),
        ("vfi_resize_bilinear", "out_cs < C", [p, 2, q, 1, 1, 2, 2, 4, 4, 2, f(1.0)]),
        ("vfi_warp_film", "input window off by one float", [p + 4, 8, p, 2, f(1.0), q, 4, 1, 2, 2, 4]),
        ("vfi_warp_film", "output window off by three floats", [p, 4, p, 2, f(1.0), q + 12, 8, 1, 2, 2, 4]),
        ("vfi_ifrnet_output", "H = 0", [p, p, p, p, q, 1, 8, 8, 8, 8, 0, 8]), ("vfi_ifrnet_output", "W < 0", [p, p, p, p, q, 1, 8, 8, 8, 8, 8, -1]),
        ("vfi_conv7x7s2_prelu", "Cout = 32", [p, 4, p, p, p, 32, q, 32, 1, 4, 4]),
        ("vfi_fill_items", "N = 65", [q, 1, 1, 65, 1, (C.c_float * 65)()]),
    ]
