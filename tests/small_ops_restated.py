"""Float64 restatements, error bounds, case tables and the buffer harness for the small ops underneath the RIFE 4.0, IFRNet, IFUNet
and GMFSS nodes: the body-launched entry points of csrc/gmfss_ops.hip and csrc/ifunet_ops.hip (bodies in gmfss_bodies.h /
ifunet_bodies.h, launched by body_launch.h), the device kernels of vfi_instnorm_stats (csrc/gmfss_fast.hip) and the four entry points
of csrc/rife40_ops.hip.  No product code is imported: every op is stated as the mathematical function of the reference formula its
body cites (GMFSS_Fortuna_union_arch.py, IFUNet_arch.py, rife_arch.py), evaluated in float64 on the fp32 inputs.

tests/test_small_ops_restated_cpu.py runs the tables through the host build of the bodies (tests/hostcheck), tests/test_gpu_small_ops.py
through the device library; both use `run_case` below, so buffers, bounds and conditions are the same on both.

BOUNDS.  U = 2^-24.  Every toleranced op returns a per-element bound on |fp32 - float64|: gamma * U * sum|terms| with gamma the
number of roundings on the way to one element (counted in each op's docstring), plus where they apply

  samplers (vfi_warp_rife: border clamp; vfi_flow_sample and the backwarps of vfi_gmfss_metric_inputs: zeros; all align_corners=True;
      vfi_resize_bilinear_ac).  The reference samples at the exact position p = X + fx (Y + fy).  The sampled value is continuous
      and piecewise bilinear in p, border and zero padding included, with slope at most D = the spread (max - min) of the 4 x 4 pixels around
      the cell (local_spread: the cell's four taps and those of the neighbouring cells, padding included).  The kernels reach p through a chain of R fp32 roundings of quantities whose size in
      pixels is at most |p| + (size - 1), so their position is off by at most d = R U (|p| + size - 1) per axis and the value by
      (dx + dy) D — on whichever side of an integer either position lies: no exclusion at integer positions.  Where p is further
      than d outside the range in which the value still depends on it (the image for border clamp, one pixel more for zeros) both
      agree exactly and the term is zero.  The value-rounding term is 8 U sum|tap * weight| (two 1 - w, the weight product, four
      products, three additions).
  expf       3 ulp (OpenCL full profile; CUDA's table gives 2): relative 2 * 3 U, since one ulp of y is at most 2 U |y|.
  tanhf      5 ulp (OpenCL full profile; CUDA's table gives 2).
  erff       E_ERF = 4 ulp and GELU's bound 0.5 |v| (E_ERF + 3) U + 2 U |y|: tests/conv_restated.py.
  sigmoid    1 / (1 + expf(-v)) within 8 U y: tests/conv_restated.py (the FLAVR gate's figure).
      The ROCm installation documents no accuracy table for these functions; the figures are the larger of the two public tables, as
      conv_restated does for erff.  None is fitted to the kernels: both runners print max err / tol of every toleranced case.
  underflow  results below 2^-126 (a softmax term behind a -100 mask, a saturated sigmoid) may be flushed: an absolute 2^-126 times
      the size of what they multiply.  Where a softmax term exp(t - max) is below 2^-151 the fp32 result must be exactly zero.
  softmax    y_j = exp(t_j - max) / sum: the exponent is off by A_j = U (|t_j| + |max| + |t_j - max|) when a mask is added first (one
      rounding of each sum, one of the difference), U |t_j - max| without one; numerator and denominator each carry that and expf;
      the sum has cols - 1 additions; then one reciprocal or division and one product:
      relative (A_j + max_k A_k) + (4 * 3 + cols + 1) U.

EXACT OPS (bound zero, compared with torch.equal): pad_rgb, prelu_scalar (one product: the rounded float64 product IS the fp32
result), window_partition both ways, pixel_shuffle2, clamp_crop, fill_channels, rife40_prep, absmax, splat_prep's flow output.

Where the inputs are positive ([0.5, 1]) a restatement also returns `mn`, the size of one summand (a channel, a softmax term, the
largest tap of a sampler), and the comparison first asserts mn > tol: a dropped or doubled summand cannot pass.

BUFFERS (class Buffers).  Every operand and every output is a [pixels, C] window at channel offset `off` of a [pixels, cs] body that
sits between two guard rows (after an output: 256 rows, what the tail threads of the last block would reach without their
guard); everything outside the window is NaN.  After the call every buffer is read back and compared BIT FOR
BIT with what it held before, outside the window for outputs and in-place operands, everywhere for inputs: a stray write fails, a
read outside the operand poisons the result, an output element left NaN is a missing write.  Dense operands (cs = C) have the guard
rows only.  The body starts 16-byte aligned, so `off` alone decides a window's alignment.
"""
import ctypes as C
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as Fn

U = 2.0 ** -24
E_ERF, E_EXP, E_TANH, SIGMOID_U = 4.0, 3.0, 5.0, 8.0
TINY = 2.0 ** -126
NAN = float("nan")
INF = float("inf")


# ---------------------------------------------------------------------------------------------------------------- buffers

class Buffers:
    def __init__(self, device):
        self.device = device
        self.b = {}

    def add(self, name, body, px=None, C=None, cs=None, off=0, role="in", dtype=torch.float32):
        """body: [px, C] values of the window (None: NaN, an output).  role: in / out / inout / scratch."""
        if body is not None:
            body = body.reshape(body.shape[0], -1) if body.dim() > 1 else body.reshape(-1, 1)
            px, C = body.shape
        cs = C if cs is None else cs
        assert off + C <= cs and px > 0
        G = max(4, -(-cs // 4) * 4)
        after = G + (256 * cs if role != "in" else 0)      # a body without its guard writes up to 255 elements' worth past the end: still inside
        host = torch.full((G + px * cs + after,), NAN, dtype=dtype)
        if body is not None:
            host[G:G + px * cs].view(px, cs)[:, off:off + C] = body.to(dtype)
        win = torch.zeros(host.shape, dtype=torch.bool)
        win[G:G + px * cs].view(px, cs)[:, off:off + C] = True
        dev = host.clone().to(self.device)
        self.b[name] = SimpleNamespace(host=host, dev=dev, win=win, G=G, px=px, C=C, cs=cs, off=off, role=role)

    def ptr(self, name, extra=0):
        b = self.b[name]
        return b.dev.data_ptr() + b.dev.element_size() * (b.G + b.off + extra)

    def finish(self):
        """-> {name: [px, C] window after the call}; asserts the guards (and the inputs) are bit-identical to before."""
        outs = {}
        for name, b in self.b.items():
            after = b.dev.cpu()
            it = torch.int32 if after.dtype == torch.float32 else torch.int64
            same = after.view(it) == b.host.view(it)
            must = ~b.win if b.role != "in" else torch.ones_like(b.win)
            bad = must & ~same
            assert not bad.any(), (f"{name} ({b.role}): {int(bad.sum())} element(s) outside the window changed (a stray write); first at flat "
                                   f"index {int(bad.nonzero()[0])} of a body starting at {b.G}, cs {b.cs}, window {b.off}..{b.off + b.C}")
            outs[name] = after[b.G:b.G + b.px * b.cs].view(b.px, b.cs)[:, b.off:b.off + b.C].clone()
        return outs


# ---------------------------------------------------------------------------------------------------------------- comparison

def compare(got, e, what):
    """e: dict(want float64, tol float64 or None for exact, mn, where, zero).  -> max err / tol (None for exact)."""
    want = e["want"].reshape(got.shape)
    tol = e.get("tol")
    if tol is None:
        w32 = want.float()
        if not torch.equal(got, w32):
            bad = ~(got == w32)
            i = tuple(int(k) for k in bad.nonzero()[0])
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result; first at {i}: got {got[i].item()!r} want {w32[i].item()!r}")
        return None
    tol = tol.reshape(got.shape)
    where = e.get("where")
    where = torch.ones_like(got, dtype=torch.bool) if where is None else where.reshape(got.shape)
    if e.get("mn") is not None:          # from the reference alone, before the output is looked at
        mn = e["mn"].reshape(got.shape)
        assert bool((mn[where] > tol[where]).all()), f"{what}: a summand is below the tolerance; the case cannot see a dropped one"
    nan = torch.isnan(got)
    assert not nan.any(), f"{what}: {int(nan.sum())} of {nan.numel()} outputs NaN (unwritten, or a NaN was read); first at {nan.nonzero()[0].tolist()}"
    err = (got.double() - want).abs()
    rel = torch.where(err <= tol, torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.zeros_like(err)), torch.full_like(err, INF))
    rel = torch.where(err == 0, torch.zeros_like(err), rel)
    rel = torch.where(where, rel, torch.zeros_like(rel))
    ratio = float(rel.max())
    print(f"  {what}: max err / tol = {ratio:.3f} (max err {float(err[where].max()):.3e})")
    if not ratio <= 1.0:
        i = tuple(int(k) for k in (rel == rel.max()).nonzero()[0])
        raise AssertionError(f"{what}: {int((rel > 1).sum())} of {rel.numel()} elements outside the bound; worst at {i}: got {got[i].item()!r} "
                             f"want {want[i].item()!r} tol {tol[i].item():.3e}")
    if e.get("zero") is not None:
        z = e["zero"].reshape(got.shape)
        assert bool((got[z] == 0).all()), f"{what}: a softmax term below 2^-151 is not exactly zero"
    return ratio


def _rc(rc, name):
    assert rc == 0, f"{name} -> {rc}"


def run_case(lib, case, device="cpu", stream=None, sync=None, check=_rc):
    """Builds the case's buffers on `device`, calls the entry point(s) of `lib` (any library exporting the C ABI), checks guards and
    results.  -> largest err / tol of the case (0.0 for an exact one)."""
    B = Buffers(device)
    calls, expects = OPS[case.op](SimpleNamespace(**case.p), B)
    for name, args in calls:
        check(getattr(lib, name)(*args, stream), name)
    if sync is not None:
        sync()
    outs = B.finish()
    worst = 0.0
    for e in expects:
        r = compare(outs[e["buf"]], e, f"{case.id}:{e['buf']}")
        worst = max(worst, r or 0.0)
    return worst


class Case:
    def __init__(self, op, tag, **p):
        self.op, self.id, self.p = op, f"{op}-{tag}", p

    def __repr__(self):
        return self.id

    def but(self, **p):
        return Case(self.op, self.id.split("-", 1)[1] + "-mut", **{**self.p, **p})


# ---------------------------------------------------------------------------------------------------------------- input makers

def _g(seed):
    return torch.Generator().manual_seed(seed)


def _pos(g, *shape):
    return 0.5 + 0.5 * torch.rand(*shape, generator=g)


def _noise(g, *shape, s=1.0):
    return torch.randn(*shape, generator=g) * s


def _make(g, kind, *shape):
    return _pos(g, *shape) if kind == "pos" else _noise(g, *shape)


def _exact(buf, want):
    return dict(buf=buf, want=want.double(), tol=None)


FAMILIES = ("zero", "int", "+half", "-half", "int+1e-6", "int-1e-6", "just below 0", "just above size-1", "+1e4", "-1e4", "random")
FAMILIES_WARP = FAMILIES + ("+1e30", "-1e30")


def flow_field(g, N, H, W, kind, nfam):
    """[N, H, W, 2] fp32.  'zero'; 'rand': N(0, 1.5); 'mixed': pixel i takes family (i + 3 n) % nfam in x and another in y, so every
    family of FAMILIES meets every image position class over the batch."""
    if kind == "zero":
        return torch.zeros(N, H, W, 2)
    if kind in ("far+", "far-"):
        return torch.full((N, H, W, 2), 1e4 if kind == "far+" else -1e4)
    rnd = _noise(g, N, H, W, 2, s=1.5)
    if kind == "rand":
        return rnd
    f = torch.zeros(N, H, W, 2)
    for n in range(N):
        for y in range(H):
            for x in range(W):
                i = (y * W + x) + 3 * n
                for ax, (pos, size, k) in enumerate(((x, W, i % nfam), (y, H, (5 * i + 2) % nfam))):
                    integer = float(1 - 3 * ((i + ax) % 2))          # +1 or -2
                    v = (0.0, integer, 0.5, -0.5, integer + 1e-6, integer - 1e-6, -pos - 0.5, size - 0.5 - pos, 1e4, -1e4,
                         float(rnd[n, y, x, ax]), 1e30, -1e30)[k]
                    f[n, y, x, ax] = v
    return f


# ---------------------------------------------------------------------------------------------------------------- samplers

def bilinear(img, px, py, border):
    """img [N,H,W,C] float64, exact positions px, py [N,H,W] float64 -> (value, sum|tap*weight|, largest |tap*weight|).  border: the
    position is clamped to the image (grid_sample padding_mode='border'); otherwise taps outside the image are zero."""
    N, H, W, Cc = img.shape
    if border:
        px, py = px.clamp(0, W - 1), py.clamp(0, H - 1)
    else:
        px, py = px.clamp(-2, W + 1), py.clamp(-2, H + 1)        # further out every tap is outside: the value is 0 either way
    x0, y0 = px.floor(), py.floor()
    wx, wy = px - x0, py - y0
    n = torch.arange(N).view(N, 1, 1).expand(px.shape)
    out = torch.zeros(*px.shape, Cc, dtype=torch.float64)
    M, big = torch.zeros_like(out), torch.zeros_like(out)
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = (x0 + dx).long(), (y0 + dy).long()
            w = (wx if dx else 1 - wx) * (wy if dy else 1 - wy)
            valid = ((xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)).double()
            if border:
                valid = torch.ones_like(valid)                    # an index past the edge carries weight 0
            term = img[n, yi.clamp(0, H - 1), xi.clamp(0, W - 1)] * (w * valid).unsqueeze(-1)
            out += term
            M += term.abs()
            big = torch.maximum(big, term.abs())
    return out, M, big, local_spread(img, x0, y0, border)


def local_spread(img, x0, y0, border):
    """max - min of the 4 x 4 pixels x0-1 .. x0+2, y0-1 .. y0+2 (outside the image: the edge pixel for border, zero otherwise): the four
    taps of the cell and of every cell a position error below one pixel can reach; the slope of the bilinear surface there is at
    most this."""
    N, H, W, Cc = img.shape
    t = img.permute(0, 3, 1, 2)
    t = Fn.pad(t, (2, 2, 2, 2), mode="replicate") if border else Fn.pad(t, (2, 2, 2, 2))
    sp = (Fn.max_pool2d(t, 4, 1) + Fn.max_pool2d(-t, 4, 1)).permute(0, 2, 3, 1)          # [N, H+1, W+1, C]; entry (i, j): rows i-2 .. i+1
    n = torch.arange(N).view(N, 1, 1).expand(x0.shape)
    return sp[n, (y0.long() + 1).clamp(0, H), (x0.long() + 1).clamp(0, W)]


def _pos_err(p, size, R, border):
    d = R * U * (p.abs() + (size - 1))
    lo, hi = (0.0, size - 1.0) if border else (-1.0, float(size))
    return torch.where((p < lo - d) | (p > hi + d), torch.zeros_like(d), d)


def sample(img, fx, fy, border, R, shift=0.0):
    """value, bound, largest tap of sampling img [N,H,W,C] at (X + fx, Y + fy); R roundings in the kernel's coordinate chain."""
    N, H, W, Cc = img.shape
    X = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    Y = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    px, py = X + fx.double() + shift, Y + fy.double() + 0 * X
    out, M, big, D = bilinear(img, px, py, border)
    d = _pos_err(px, W, R, border) + _pos_err(py, H, R, border)
    assert float(d.max()) < 0.5, "local_spread covers position errors below one pixel only"
    return out, d.unsqueeze(-1) * D + 8 * U * M, torch.where(M > 0, big, torch.full_like(big, INF))      # no summand where every tap is outside


R_FLOW = 5        # X + f, / (W-1), - 1, + 1, * (W-1)                         (flow_sample_body, ztap_from_norm; * 2 and / 2 are exact)
R_BACKWARP = 7    # 2/(n-1), step * i, -1 + ., f / half, + , + 1, * (W-1)      (lin11h + metric_inputs_body + ztap_from_norm)
R_WARP = 7        # the same chain in rife_warp.h: lin11, fx / halfw, +, + 1, * halfw
R_RESIZE = 2      # (in-1)/(out-1), * x


def _op_sampler(P, B, fn, border, R):
    g = _g(P.seed)
    img = _make(g, P.kind, P.N, P.H, P.W, P.C)
    nfam = len(FAMILIES_WARP if border else FAMILIES)
    fl = flow_field(g, P.N, P.H, P.W, P.flow, nfam)
    px = P.N * P.H * P.W
    B.add("in", img.reshape(px, P.C), cs=P.in_cs, off=P.in_off)
    B.add("flow", fl.reshape(px, 2), cs=P.flow_cs, off=P.flow_off)
    B.add("out", None, px, P.C, P.out_cs, P.out_off, role="out")
    want, tol, big = sample(img.double(), fl[..., 0], fl[..., 1], border, R, shift=getattr(P, "shift", 0.0))
    if getattr(P, "drop", None) is not None:
        want[..., P.drop] = 0
    e = dict(buf="out", want=want, tol=tol, mn=big if P.kind == "pos" and getattr(P, "drop", None) is None else None)
    return [(fn, [B.ptr("in"), P.in_cs, B.ptr("flow"), P.flow_cs, B.ptr("out"), P.out_cs, P.N, P.H, P.W, P.C])], [e]


def op_warp_rife(P, B):
    """rife_arch.py warp() :31-70: grid_sample(border, align_corners=True) at pixel + flow."""
    return _op_sampler(P, B, "vfi_warp_rife", True, R_WARP)


def op_flow_sample(P, B):
    """GMFSS flow_warp / bilinear_sample :955-991: zeros padding at pixel + flow."""
    return _op_sampler(P, B, "vfi_flow_sample", False, R_FLOW)


def op_resize_bilinear_ac(P, B):
    """F.interpolate(bilinear, align_corners=True) * post_mul :1302-1307: source position x (in-1)/(out-1), an interior point of the
    image (border clamp never acts); 2 coordinate roundings; value: 8 U M (1 - l twice, 6 products / additions) and one for post_mul."""
    g = _g(P.seed)
    img = _make(g, P.kind, P.N, P.Hi, P.Wi, P.C)
    B.add("in", img.reshape(-1, P.C), cs=P.in_cs, off=P.in_off)
    B.add("out", None, P.N * P.Ho * P.Wo, P.C, P.out_cs, P.out_off, role="out")
    sx = torch.arange(P.Wo, dtype=torch.float64) * ((P.Wi - 1) / (P.Wo - 1) if P.Wo > 1 else 0.0)
    sy = torch.arange(P.Ho, dtype=torch.float64) * ((P.Hi - 1) / (P.Ho - 1) if P.Ho > 1 else 0.0)
    px, py = sx.view(1, 1, -1).expand(P.N, P.Ho, P.Wo), sy.view(1, -1, 1).expand(P.N, P.Ho, P.Wo)
    pm = float(torch.tensor(P.post_mul, dtype=torch.float32))
    out, M, big, D = bilinear(img.double(), px, py, True)
    out, M, big, D = out * pm, M * abs(pm), big * abs(pm), D * abs(pm)
    d = R_RESIZE * U * (px + (P.Wi - 1)) + R_RESIZE * U * (py + (P.Hi - 1))
    tol = d.unsqueeze(-1) * D + 9 * U * M
    args = [B.ptr("in"), P.in_cs, B.ptr("out"), P.out_cs, P.N, P.Hi, P.Wi, P.Ho, P.Wo, P.C, C.c_float(P.post_mul)]
    return [("vfi_resize_bilinear_ac", args)], [dict(buf="out", want=out, tol=tol, mn=big if P.kind == "pos" else None)]


def op_gmfss_metric_inputs(P, B):
    """MetricNet's input :1375-1454 (one image pair).  0..5 copies (exact).  6, 7: -mean_c |img - backwarp(other, flow)|: the three
    sampler bounds, one subtraction each, two additions, the division: (sum_c (tol_c + U |diff_c|)) / 3 + 4 U |out|.  8..11: flow /
    ((size-1)/2), one rounding.  12, 13: the bits d > thr of forward_backward_consistency_check :994-1012 with d = |f + f'(x + f)|,
    thr = 0.01 (|f01| + |f10|) + 0.5.  d: the two sampled components carry their sampler bounds tw, the sums one rounding each, the
    norm is 1-Lipschitz in each component and its squares, sum and root add 3 U d; thr: two roots (3 U each with their squares), their
    sum, the constant 0.01 in fp32, the product and the addition: 7 U thr.  The bit is compared where |d - thr| exceeds
    tw_x + tw_y + U (|a| + |b|) + 3 U d + 7 U thr; the share of pixels left out is asserted <= 1 % from the reference alone."""
    g = _g(P.seed)
    H, W = P.H, P.W
    i0, i1 = _make(g, P.kind, 1, H, W, 3), _make(g, P.kind, 1, H, W, 3)
    if P.flow == "far":         # every backwarp and both consistency samples land far outside the image
        fa, fb = flow_field(g, 1, H, W, "far+", 0), flow_field(g, 1, H, W, "far-", 0)
    else:                       # 'mixed' stops at 'just above size-1' here: the flows are also the IMAGE the consistency check samples, and a
        #                         neighbour of 1e4 in it makes the occlusion bits ill-conditioned (bound ~0.1); the 'far' cases cover +-1e4
        fa, fb = flow_field(g, 1, H, W, P.flow, 8), flow_field(_g(P.seed + 1), 1, H, W, P.flow, 8)
    if P.flow == "mixed":
        fb = fb.flip(1, 2).contiguous()
    for nm, t, cs, off in (("img0", i0, P.img_cs, P.img_off), ("img1", i1, P.img_cs, P.img_off), ("f01", fa, P.f_cs, P.f_off), ("f10", fb, P.f_cs, P.f_off)):
        B.add(nm, t.reshape(H * W, -1), cs=cs, off=off)
    B.add("out", None, H * W, 14, P.out_cs, P.out_off, role="out")
    d0, d1, A, Bf = i0.double(), i1.double(), fa.double(), fb.double()
    want = torch.zeros(1, H, W, 14, dtype=torch.float64)
    tol = torch.zeros_like(want)
    where = torch.ones_like(want, dtype=torch.bool)
    want[..., 0:3], want[..., 3:6] = d0, d1
    for ch, (a, b, f) in enumerate(((d0, d1, fa), (d1, d0, fb))):
        w, tw, _ = sample(b, f[..., 0], f[..., 1], False, R_BACKWARP, shift=getattr(P, "shift", 0.0))
        diff = (a - w).abs()
        want[..., 6 + ch] = -diff.mean(-1)
        tol[..., 6 + ch] = (tw + U * diff).sum(-1) / 3 + 4 * U * diff.mean(-1)
    half = torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0], dtype=torch.float64)
    want[..., 8:10], want[..., 10:12] = A / half, Bf / half
    tol[..., 8:12] = U * want[..., 8:12].abs()
    mag = A.norm(dim=-1) + Bf.norm(dim=-1)
    thr = 0.01 * mag + 0.5
    for ch, (f, other, fo) in enumerate(((A, Bf, fa), (Bf, A, fb))):
        w, tw, _ = sample(other, fo[..., 0], fo[..., 1], False, R_FLOW)
        s = f + w
        d = s.norm(dim=-1)
        td = tw.sum(-1) + U * s.abs().sum(-1) + 3 * U * d + 7 * U * thr
        want[..., 12 + ch] = (d > thr).double()
        where[..., 12 + ch] = (d - thr).abs() > td
    out_share = 1.0 - where[..., 12:].double().mean().item()
    assert out_share <= 0.01, f"{out_share:.3%} of the occlusion bits are within the bound of their threshold: choose other flows"
    args = [B.ptr("img0"), B.ptr("img1"), P.img_cs, B.ptr("f01"), B.ptr("f10"), P.f_cs, B.ptr("out"), P.out_cs, H, W]
    return [("vfi_gmfss_metric_inputs", args)], [dict(buf="out", want=want, tol=tol, where=where)]


# ---------------------------------------------------------------------------------------------------------------- element-wise

def _pc(P, B, g, name, kind=None, C=None, cs=None, off=None, role="in"):
    C = P.C if C is None else C
    t = _make(g, kind or P.kind, P.px, C)
    B.add(name, t, cs=getattr(P, name + "_cs") if cs is None else cs, off=getattr(P, name + "_off") if off is None else off, role=role)
    return t


def op_pad_rgb(P, B):
    """F.pad of channels 0..2 of an [H, W, C] frame into [Hp, Wp] (gmfss_fortuna/__init__.py:43-48).  Exact."""
    fr = _noise(_g(P.seed), P.H * P.W, P.C)
    B.add("frame", fr)
    B.add("out", None, P.Hp * P.Wp, 3, P.out_cs, P.out_off, role="out")
    want = torch.zeros(P.Hp, P.Wp, 3)
    want[:P.H, :P.W] = fr.view(P.H, P.W, P.C)[..., :3]
    return [("vfi_pad_rgb", [B.ptr("frame"), P.C, P.H, P.W, B.ptr("out"), P.out_cs, P.Hp, P.Wp])], [_exact("out", want)]


def op_normalize_channels(P, B):
    """normalize_img :1123-1131, (x - mean_c) / std_c: a subtraction and a division, 3 U |y| (the division sees the difference's error)."""
    g = _g(P.seed)
    x = _pc(P, B, g, "in")
    B.add("out", None, P.px, P.C, P.out_cs, P.out_off, role="out")
    mean, std = torch.rand(P.C, generator=g), 0.2 + 0.1 * torch.rand(P.C, generator=g)
    y = (x.double() - mean.double()) / std.double()
    args = [B.ptr("in"), P.in_cs, B.ptr("out"), P.out_cs, P.C, P.px, (C.c_float * P.C)(*mean.tolist()), (C.c_float * P.C)(*std.tolist())]
    return [("vfi_normalize_channels", args)], [dict(buf="out", want=y, tol=3 * U * y.abs())]


def op_prelu_scalar(P, B):
    """nn.PReLU() with one slope: v or v * slope.  Exact: the float64 product of two fp32 numbers is exact, its cast the one rounding."""
    x = _pc(P, B, _g(P.seed), "in")
    B.add("out", None, P.px, P.C, P.out_cs, P.out_off, role="out")
    slope = float(torch.tensor(P.slope, dtype=torch.float32))
    want = torch.where(x > 0, x.double(), x.double() * slope)
    return [("vfi_prelu_scalar", [B.ptr("in"), P.in_cs, B.ptr("out"), P.out_cs, P.C, P.px, C.c_float(P.slope)])], [_exact("out", want)]


def op_gelu(P, B):
    """nn.GELU() (erf form), in place: conv_restated's bound 0.5 |v| (E_ERF + 3) U + 2 U |y|."""
    x = _noise(_g(P.seed), P.px, P.C, s=2.0)
    B.add("x", x, cs=P.x_cs, off=P.x_off, role="inout")
    v = x.double()
    y = 0.5 * v * (1 + torch.erf(v / math.sqrt(2.0)))
    tol = 0.5 * v.abs() * (E_ERF + 3) * U + 2 * U * y.abs()
    return [("vfi_gelu", [B.ptr("x"), P.x_cs, P.C, P.px])], [dict(buf="x", want=y, tol=tol)]


def op_tanh_scale(P, B):
    """tanh(x) * s :1465, in place: tanhf E_TANH ulp = 2 E_TANH U relative, one product."""
    x = _pc(P, B, _g(P.seed), "x", role="inout")
    y = torch.tanh(x.double() * 1.0) * float(torch.tensor(P.s, dtype=torch.float32))
    return [("vfi_tanh_scale", [B.ptr("x"), P.x_cs, P.C, P.px, C.c_float(P.s)])], [dict(buf="x", want=y, tol=(2 * E_TANH + 1) * U * y.abs())]


def op_fill_channels(P, B):
    """a constant over a channel window.  Exact."""
    B.add("out", None, P.px, P.C, P.out_cs, P.out_off, role="out")
    want = torch.full((P.px, P.C), P.v, dtype=torch.float32)
    return [("vfi_fill_channels", [B.ptr("out"), P.out_cs, P.C, P.px, C.c_float(P.v)])], [_exact("out", want)]


def op_lerp_mask(P, B):
    """a m + b (1 - m) :764: 1 - m, two products, one addition: 4 U (|a m| + |b (1 - m)|).  Summand: one of the two products."""
    g = _g(P.seed)
    a, b = _pc(P, B, g, "a"), _pc(P, B, g, "b")
    m = torch.rand(P.px, 1, generator=g) * 0.8 + 0.1 if P.kind == "pos" else _noise(g, P.px, 1)
    B.add("m", m, cs=P.m_cs, off=P.m_off)
    B.add("out", None, P.px, P.C, P.out_cs, P.out_off, role="out")
    ta, tb = a.double() * m.double(), b.double() * (1 - m.double())
    if getattr(P, "drop", None) is not None:
        tb[:, P.drop] = 0
    Mm = ta.abs() + tb.abs()
    args = [B.ptr("a"), P.a_cs, B.ptr("b"), P.b_cs, B.ptr("m"), P.m_cs, B.ptr("out"), P.out_cs, P.C, P.px]
    return [("vfi_lerp_mask", args)], [dict(buf="out", want=ta + tb, tol=4 * U * Mm, mn=torch.minimum(ta.abs(), tb.abs()) if P.kind == "pos" and getattr(P, "drop", None) is None else None)]


def op_add_clamp01(P, B):
    """clamp(a + b, 0, 1) :161: one addition; the clamp is 1-Lipschitz."""
    g = _g(P.seed)
    a, b = _pc(P, B, g, "a"), _pc(P, B, g, "b")
    B.add("out", None, P.px, P.C, P.out_cs, P.out_off, role="out")
    s = a.double() + b.double()
    args = [B.ptr("a"), P.a_cs, B.ptr("b"), P.b_cs, B.ptr("out"), P.out_cs, P.C, P.px]
    return [("vfi_add_clamp01", args)], [dict(buf="out", want=s.clamp(0, 1), tol=U * s.abs())]


def op_splat_prep(P, B):
    """softsplat 'soft' (softsplat.py:408-432): e = exp(zs z); out = (x e, e); flow_out = fs flow (one product: exact).  The argument's
    rounding moves e by U |zs z| relative, expf 2 E_EXP U, the product one more."""
    g = _g(P.seed)
    x = _pc(P, B, g, "x")
    z = _noise(g, P.px, 1, s=2.0)
    fl = _noise(g, P.px, 2, s=3.0)
    B.add("z", z, cs=P.z_cs, off=P.z_off)
    B.add("flow", fl, cs=P.flow_cs, off=P.flow_off)
    B.add("out", None, P.px, P.C + 1, role="out")
    B.add("flow_out", None, P.px, 2, role="out")
    zs, fs = float(torch.tensor(P.zs, dtype=torch.float32)), float(torch.tensor(P.fs, dtype=torch.float32))
    arg = zs * z.double()
    e = torch.exp(arg)
    want = torch.cat([x.double() * e, e], 1)
    tol = want.abs() * (U * arg.abs() + (2 * E_EXP + 1) * U)
    args = [B.ptr("x"), P.x_cs, B.ptr("z"), P.z_cs, B.ptr("flow"), P.flow_cs, B.ptr("out"), B.ptr("flow_out"), P.C, P.px, C.c_float(P.zs), C.c_float(P.fs)]
    return [("vfi_splat_prep", args)], [dict(buf="out", want=want, tol=tol), _exact("flow_out", fl.double() * fs)]


def op_splat_normalize(P, B):
    """s[0:C] / (s[C] + 1e-7): the constant in fp32, the addition, the division: 4 U |y| (denominators are positive)."""
    g = _g(P.seed)
    s = torch.cat([_noise(g, P.px, P.C), _pos(g, P.px, 1)], 1)
    B.add("s", s)
    B.add("out", None, P.px, P.C, P.out_cs, P.out_off, role="out")
    y = s[:, :P.C].double() / (s[:, P.C:].double() + 1e-7)
    return [("vfi_splat_normalize", [B.ptr("s"), B.ptr("out"), P.out_cs, P.C, P.px])], [dict(buf="out", want=y, tol=4 * U * y.abs())]


def op_pixel_shuffle2(P, B):
    """nn.PixelShuffle(2): out[2y+dy, 2x+dx, c] = in[y, x, 4c + 2dy + dx].  Exact."""
    x = _noise(_g(P.seed), P.N, P.H, P.W, 4 * P.C)
    B.add("in", x.reshape(-1, 4 * P.C), cs=P.in_cs, off=P.in_off)
    B.add("out", None, P.N * 4 * P.H * P.W, P.C, P.out_cs, P.out_off, role="out")
    want = x.view(P.N, P.H, P.W, P.C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(P.N, 2 * P.H, 2 * P.W, P.C)
    return [("vfi_pixel_shuffle2", [B.ptr("in"), P.in_cs, B.ptr("out"), P.out_cs, P.N, P.H, P.W, P.C])], [_exact("out", want)]


def op_clamp_crop(P, B):
    """clamp(x, 0, 1)[:H, :W] into a dense [H, W, C].  Exact."""
    x = _noise(_g(P.seed), P.Hp, P.Wp, P.C)
    B.add("in", x.reshape(-1, P.C), cs=P.in_cs, off=P.in_off)
    B.add("out", None, P.H * P.W, P.C, role="out")
    return [("vfi_clamp_crop", [B.ptr("in"), P.in_cs, P.Hp, P.Wp, B.ptr("out"), P.H, P.W, P.C])], [_exact("out", x[:P.H, :P.W].clamp(0, 1))]


def op_window_partition(P, B):
    """roll by (-sh, -sw) and split into K x K windows, or the inverse (:367-436, split_feature / merge_splits :1059-1120).  Exact."""
    img = _noise(_g(P.seed), P.B, P.h, P.w, P.C)
    wh, ww = P.h // P.K, P.w // P.K
    win = torch.roll(img, (-P.sh, -P.sw), (1, 2)).view(P.B, P.K, wh, P.K, ww, P.C).permute(0, 1, 3, 2, 4, 5).reshape(-1, P.C)
    src, want = (win, img) if P.inverse else (img, win)
    B.add("in", src.reshape(-1, P.C), cs=P.in_cs, off=P.in_off)
    B.add("out", None, P.B * P.h * P.w, P.C, P.out_cs, P.out_off, role="out")
    args = [B.ptr("in"), P.in_cs, B.ptr("out"), P.out_cs, P.B, P.h, P.w, P.C, P.K, P.sh, P.sw, P.inverse]
    return [("vfi_window_partition", args)], [_exact("out", want)]


# ---------------------------------------------------------------------------------------------------------------- products, softmax

def op_bmm_nt(P, B):
    """alpha sum_k A[b,m,k] Bm[b,n,k] (:319,417-420,810-812): K products and additions in any association, the product with alpha:
    (K + 2) U |alpha| sum|a b|.  Summand: one k."""
    g = _g(P.seed)
    a, b = _make(g, P.kind, P.nb, P.M, P.K), _make(g, P.kind, P.nb, P.N, P.K)
    B.add("A", a.reshape(-1, P.K), cs=P.a_cs, off=P.a_off)
    B.add("Bm", b.reshape(-1, P.K), cs=P.b_cs, off=P.b_off)
    B.add("out", None, P.nb * P.M, P.N, role="out")
    alpha = float(torch.tensor(P.alpha, dtype=torch.float32))
    terms = a.double().unsqueeze(2) * b.double().unsqueeze(1) * alpha          # [nb, M, N, K]
    if getattr(P, "drop", None) is not None:
        terms[..., P.drop] = 0
    args = [B.ptr("A"), P.a_cs, B.ptr("Bm"), P.b_cs, B.ptr("out"), P.nb, P.M, P.N, P.K, C.c_float(P.alpha)]
    e = dict(buf="out", want=terms.sum(-1), tol=(P.K + 2) * U * terms.abs().sum(-1), mn=terms.abs().amin(-1) if P.kind == "pos" and getattr(P, "drop", None) is None else None)
    return [("vfi_bmm_nt", args)], [e]


def op_bmm_nn(P, B):
    """sum_n P[b,m,n] V[b,n,c]: (N + 1) U sum|p v|."""
    g = _g(P.seed)
    p, v = _make(g, P.kind, P.nb, P.M, P.N), _make(g, P.kind, P.nb, P.N, P.C)
    B.add("P", p.reshape(-1, P.N))
    B.add("V", v.reshape(-1, P.C), cs=P.v_cs, off=P.v_off)
    B.add("out", None, P.nb * P.M, P.C, P.out_cs, P.out_off, role="out")
    terms = p.double().unsqueeze(-1) * v.double().unsqueeze(1)                 # [nb, M, N, C]
    args = [B.ptr("P"), B.ptr("V"), P.v_cs, B.ptr("out"), P.out_cs, P.nb, P.M, P.N, P.C]
    return [("vfi_bmm_nn", args)], [dict(buf="out", want=terms.sum(2), tol=(P.N + 1) * U * terms.abs().sum(2), mn=terms.abs().amin(2) if P.kind == "pos" else None)]


def softmax_bound(t, masked):
    """(y, relative bound, where exp(t - max) is below 2^-151 even with the exponent's error: the fp32 term, half the smallest
    denormal at most, is then exactly zero) of softmax over the last axis of float64 logits t (module docstring)."""
    mx = t.amax(-1, keepdim=True)
    A = U * ((t.abs() + mx.abs() + (t - mx).abs()) if masked else (t - mx).abs())
    y = torch.softmax(t, -1)
    return y, A + A.amax(-1, keepdim=True) + (4 * E_EXP + t.shape[-1] + 1) * U, (t - mx + A) < -151 * math.log(2.0)


def op_softmax_rows(P, B):
    """softmax over rows of [nb, rows, cols] in place, after adding mask[b % period] (:422-423).  Summand: dropping term k changes y_j
    by more than y_j y_k."""
    g = _g(P.seed)
    x = _make(g, P.kind, P.nb, P.rows, P.cols)
    if getattr(P, "gap", 0):
        x[0, 0, 0] += P.gap
    B.add("x", x.reshape(-1, P.cols), role="inout")
    t = x.double()
    mask_ptr = None
    if P.period:
        mk = torch.where(torch.rand(P.period, P.rows, P.cols, generator=g) < 0.3, torch.tensor(P.fill), torch.tensor(0.0))
        mk[:, :, 0] = 0                          # a row is never masked entirely
        B.add("mask", mk.reshape(-1, P.cols))
        mask_ptr = B.ptr("mask")
        t = t + mk.double().repeat(P.nb // P.period, 1, 1)
    if getattr(P, "omit", None) is not None:
        t[..., P.omit] = -INF
    y, rel, zero = softmax_bound(t, bool(P.period))
    e = dict(buf="x", want=y, tol=y * rel + TINY, zero=zero,
             mn=y * y.amin(-1, keepdim=True) if P.kind == "pos" and not P.period and getattr(P, "omit", None) is None else None)
    return [("vfi_softmax_rows", [B.ptr("x"), P.nb, P.rows, P.cols, mask_ptr, P.period])], [e]


def _op_convex(P, B, fn, FC):
    """GMFlow.upsample_flow :1237-1258 / IFBlock.upsample_flow :627-638: softmax over the 9 mask logits of a fine pixel, weighted sum of
    the 3x3 neighbourhood of K * flow (zero outside).  Weight: softmax bound without mask (9 columns); then K * f, the product, up to 9
    additions: sum|term| (rel + 11 U).  Summand: the smallest term inside the image."""
    g = _g(P.seed)
    K, KK = P.K, P.K * P.K
    mask = _make(g, P.kind, P.N, P.H, P.W, 9, KK)
    flow = _make(g, P.kind, P.N, P.H, P.W, FC)
    B.add("mask", mask.reshape(-1, 9 * KK), cs=P.mask_cs, off=P.mask_off)
    B.add("flow", flow.reshape(-1, FC), cs=P.flow_cs, off=P.flow_off)
    B.add("out", None, P.N * K * P.H * K * P.W, FC, P.out_cs, P.out_off, role="out")
    y, rel, _ = softmax_bound(mask.double().transpose(-1, -2), False)                  # [N,H,W,KK,9]
    fp = torch.nn.functional.pad(flow.double().permute(0, 3, 1, 2), (1, 1, 1, 1))  # [N,FC,H+2,W+2]
    inside = torch.nn.functional.pad(torch.ones(1, 1, P.H, P.W, dtype=torch.float64), (1, 1, 1, 1))
    out = torch.zeros(P.N, P.H, P.W, KK, FC, dtype=torch.float64)
    tol, mn = torch.zeros_like(out), torch.full_like(out, INF)
    for j in range(9):
        f = fp[:, :, j // 3:j // 3 + P.H, j % 3:j % 3 + P.W].permute(0, 2, 3, 1).unsqueeze(3) * K     # [N,H,W,1,FC]
        term = y[..., j].unsqueeze(-1) * f
        out += term
        tol += term.abs() * (rel[..., j].unsqueeze(-1) + 11 * U)
        ins = inside[0, 0, j // 3:j // 3 + P.H, j % 3:j % 3 + P.W].view(1, P.H, P.W, 1, 1) > 0
        mn = torch.where(ins, torch.minimum(mn, term.abs()), mn)
    fine = lambda t: t.view(P.N, P.H, P.W, K, K, FC).permute(0, 1, 3, 2, 4, 5).reshape(P.N, K * P.H, K * P.W, FC)
    args = [B.ptr("mask"), P.mask_cs, B.ptr("flow"), P.flow_cs, B.ptr("out"), P.out_cs, P.N, P.H, P.W, K] + ([FC] if fn.endswith("_c") else [])
    return [(fn, args)], [dict(buf="out", want=fine(out), tol=fine(tol), mn=fine(mn) if P.kind == "pos" else None)]


def op_convex_upsample(P, B):
    return _op_convex(P, B, "vfi_convex_upsample", 2)


def op_convex_upsample_c(P, B):
    return _op_convex(P, B, "vfi_convex_upsample_c", P.FC)


def op_ifunet_blend(P, B):
    """ResynNet's blend :188-192, cropped to H x W: softmax over (clamp(m0, -4, 4), clamp(m1, -4, 4), 0) weights img0, img1, deg.  The
    body has no sampler.  Weight: softmax bound without mask (3 columns); one product and three additions: sum|term| (rel + 4 U)."""
    g = _g(P.seed)
    px = P.Hp * P.Wp
    imgs = [_make(g, P.kind, px, 3) for _ in range(3)]
    ms = [_noise(g, px, 1, s=4.0) for _ in range(2)]
    for nm, t in zip(("img0", "img1", "deg"), imgs):
        B.add(nm, t, cs=P.img_cs, off=P.img_off)
    for nm, t in zip(("m0", "m1"), ms):
        B.add(nm, t, cs=P.m_cs, off=P.m_off)
    B.add("out", None, P.H * P.W, 3, role="out")
    t = torch.cat([ms[0].double().clamp(-4, 4), ms[1].double().clamp(-4, 4), torch.zeros(px, 1, dtype=torch.float64)], 1)
    y, rel, _ = softmax_bound(t, False)
    terms = torch.stack([imgs[k].double() * y[:, k:k + 1] for k in range(3)])
    if getattr(P, "omit", None) is not None:
        terms[P.omit] = 0
    tol = (terms.abs() * (rel.t().unsqueeze(-1) + 4 * U)).sum(0)
    crop = lambda v: v.view(P.Hp, P.Wp, 3)[:P.H, :P.W]
    args = [B.ptr("img0"), B.ptr("img1"), B.ptr("deg"), P.img_cs, B.ptr("m0"), B.ptr("m1"), P.m_cs, B.ptr("out"), P.Hp, P.Wp, P.H, P.W]
    e = dict(buf="out", want=crop(terms.sum(0)), tol=crop(tol), mn=crop(terms.abs().amin(0)) if P.kind == "pos" and getattr(P, "omit", None) is None else None)
    return [("vfi_ifunet_blend", args)], [e]


# ---------------------------------------------------------------------------------------------------------------- instance norm

def op_instnorm_stats(P, B):
    """InstanceNorm2d statistics :165-215 (biased variance, eps 1e-5): mean and 1 / sqrt(var + eps) per (n, c).  The library sums v and
    v^2 in float64 in some order: each of at most HW - 1 additions rounds by 2^-53 of a partial sum, so sum / HW is off by at most
    (HW + 1) 2^-53 mean|v| and var = E v^2 - mean^2 by dv = (2 HW + 6) 2^-53 E v^2 (both terms are at most E v^2).  One fp32 rounding
    each: mean within U |mean| + (HW + 1) 2^-53 mean|v|, rstd within U rstd + rstd dv / (2 (var + eps)) (1 + dv / (var + eps)).
    The reference centres before squaring, so it has no such cancellation."""
    g = _g(P.seed)
    x = _noise(g, P.N, P.HW, P.C, s=P.sigma) + P.mean
    B.add("x", x.reshape(-1, P.C), cs=P.cs, off=P.off)
    B.add("stats", None, P.N * P.C, 2, role="out")
    per = P.N * P.C * 2
    B.add("ws", None, P.strips * per, 1, role="scratch", dtype=torch.float64)
    xd = x.double()
    mean = xd.mean(1)
    var = ((xd - mean.unsqueeze(1)) ** 2).mean(1)
    eps = float(torch.tensor(1e-5, dtype=torch.float32))
    rstd = 1 / torch.sqrt(var + eps)
    d = 2.0 ** -53
    dv = (2 * P.HW + 6) * d * (xd ** 2).mean(1)
    want = torch.stack([mean, rstd], -1)
    tol = torch.stack([U * mean.abs() + (P.HW + 1) * d * xd.abs().mean(1), U * rstd + rstd * dv / (2 * (var + eps)) * (1 + dv / (var + eps))], -1)
    args = [B.ptr("x"), P.cs, P.C, P.N, P.HW, B.ptr("stats"), B.ptr("ws"), P.strips * per * 8]
    return [("vfi_instnorm_stats", args)], [dict(buf="stats", want=want, tol=tol)]


def op_instnorm_apply(P, B):
    """act2(act1((x - mean) rstd) + add): a subtraction, a product, an addition: 3 U (|t| + |add|) (ReLU is 1-Lipschitz)."""
    g = _g(P.seed)
    x = _noise(g, P.N, P.HW, P.C) + 0.5
    st = torch.stack([_noise(g, P.N, P.C), 0.5 + torch.rand(P.N, P.C, generator=g)], -1)
    B.add("x", x.reshape(-1, P.C), cs=P.cs, off=P.off)
    B.add("stats", st.reshape(-1, 2))
    B.add("out", None, P.N * P.HW, P.C, P.out_cs, P.out_off, role="out")
    t = (x.double() - st[..., 0].double().unsqueeze(1)) * st[..., 1].double().unsqueeze(1)
    bound = t.abs()
    if P.relu1:
        t = t.clamp_min(0)
    add_ptr = None
    if P.add:
        a = _noise(g, P.N, P.HW, P.C)
        B.add("add", a.reshape(-1, P.C), cs=P.add_cs, off=P.add_off)
        add_ptr = B.ptr("add")
        t = t + a.double()
        bound = bound + a.double().abs()
    if P.relu2:
        t = t.clamp_min(0)
    args = [B.ptr("x"), P.cs, B.ptr("stats"), P.C, P.N, P.HW, P.relu1, add_ptr, P.add_cs if P.add else 0, P.relu2, B.ptr("out"), P.out_cs]
    return [("vfi_instnorm_apply", args)], [dict(buf="out", want=t, tol=3 * U * bound)]


# ---------------------------------------------------------------------------------------------------------------- RIFE 4.0

def op_rife40_prep(P, B):
    """rife_arch.py:476-499: (clamp(f0.rgb, 0, 1), clamp(f1.rgb, 0, 1), t, 0) inside H x W, (0 x 6, t, 0) in the padding.  Exact."""
    g = _g(P.seed)
    f0, f1 = _noise(g, P.H, P.W, P.C) * 0.7 + 0.5, _noise(g, P.H, P.W, P.C) * 0.7 + 0.5
    B.add("f0", f0.reshape(-1, P.C))
    B.add("f1", f1.reshape(-1, P.C))
    B.add("out", None, P.Hp * P.Wp, 8, role="out")
    want = torch.zeros(P.Hp, P.Wp, 8)
    want[:P.H, :P.W, 0:3], want[:P.H, :P.W, 3:6] = f0[..., :3].clamp(0, 1), f1[..., :3].clamp(0, 1)
    want[..., 6] = torch.tensor(P.t, dtype=torch.float32)
    return [("vfi_rife40_prep", [B.ptr("f0"), B.ptr("f1"), P.C, P.H, P.W, C.c_float(P.t), B.ptr("out"), P.Hp, P.Wp])], [_exact("out", want)]


def op_absmax(P, B):
    """max |x| over a channel window (rife_arch.py:598-607 f0[:, :2].abs().max()), one call per entry of P.calls = (channel offset, C),
    each writing the next float of one small output.  Exact."""
    g = _g(P.seed)
    x = _noise(g, P.px, P.cs, s=3.0)
    if P.fillv is not None:
        x[:] = P.fillv
    for (p, c, v) in P.plant:
        x[p, c] = v
    B.add("x", x, cs=P.cs + 2, off=1)
    B.add("out", None, 1, len(P.calls), cs=len(P.calls) + 3, off=1, role="out")
    calls = [("vfi_absmax", [B.ptr("x", off), P.cs + 2, Cc, P.px, B.ptr("out", i)]) for i, (off, Cc) in enumerate(P.calls)]
    want = torch.stack([x[:, off:off + Cc].abs().max() for off, Cc in P.calls]).view(1, -1)
    return calls, [_exact("out", want)]


def op_rife40_output(P, B):
    """rife_arch.py:703-732, cropped: clamp(w0 m + w1 (1 - m) [-> clamp(. + (2 res - 1), 0, 1)], 0, 1), m = sigmoid(mask).  m within
    8 U m (sigmoid), 1 - m within that and one rounding; two products and the addition: 3 U (|w0 m| + |w1 (1 - m)|); with res: 2 res - 1
    one rounding and the sum one rounding.  A saturated sigmoid underflows: 2^-126 (|w0| + |w1|).  Clamps are 1-Lipschitz."""
    g = _g(P.seed)
    px = P.B * P.Hp * P.Wp
    wm = torch.full((px, 8), NAN)
    wm[:, 0:6] = _make(g, P.kind, px, 6)
    logit = _noise(g, px, s=3.0)
    logit[::7], logit[3::11] = 100.0, -100.0
    wm[:, 7] = logit
    B.add("wm", wm, cs=P.w_cs, off=P.w_off)
    res_ptr = None
    B.add("out", None, P.B * P.H * P.W, 3, role="out")
    w0, w1, m = wm[:, 0:3].double(), wm[:, 3:6].double(), torch.sigmoid(logit.double()).unsqueeze(1)
    t0, t1 = w0 * m, w1 * (1 - m)
    if getattr(P, "omit", None) is not None:
        t1 = t1 * 0
    v = t0 + t1
    tol = w0.abs() * SIGMOID_U * U * m + w1.abs() * (SIGMOID_U * U * m + U * (1 - m)) + 3 * U * (t0.abs() + t1.abs()) + TINY * (w0.abs() + w1.abs())
    if P.res:
        r = torch.rand(px, 3, generator=g)
        B.add("res", r, cs=P.r_cs, off=P.r_off)
        res_ptr = B.ptr("res")
        rr = 2 * r.double() - 1
        tol = tol + U * rr.abs() + U * (v + rr).abs()
        v = (v + rr).clamp(0, 1)
    crop = lambda q: q.view(P.B, P.Hp, P.Wp, 3)[:, :P.H, :P.W]
    args = [B.ptr("wm"), P.w_cs, B.ptr("wm", 7), P.w_cs, res_ptr, P.r_cs if P.res else 0, B.ptr("out"), P.B, P.Hp, P.Wp, P.H, P.W]
    return [("vfi_rife40_output", args)], [dict(buf="out", want=crop(v.clamp(0, 1)), tol=crop(tol))]


OPS = {k[3:]: v for k, v in list(globals().items()) if k.startswith("op_")}


# ---------------------------------------------------------------------------------------------------------------- case tables
# n below is the thread count the entry point passes to run<> (body_launch.h): 256-thread blocks, (n + 255) / 256 of them.

def _pc_cases(op, names, extra=None, kind="noise", C=3):
    """px * C threads: 513 (n % 256 = 1), 255 (< 256, n % 256 = 255), 768 (a multiple); every operand a window with its own stride"""
    out = []
    for tag, px in (("n513", 171), ("n255", 85), ("n768", 256)):
        p = dict(seed=len(op) + px, px=px, C=C, kind=kind, **(extra or {}))
        for i, nm in enumerate(names):
            p[nm + "_cs"], p[nm + "_off"] = C + 3 + i, 1 + i % 2
        out.append(Case(op, tag, **p))
    return out


def _win(d, **names):
    for nm, (cs, off) in names.items():
        d[nm + "_cs"], d[nm + "_off"] = cs, off
    return d


BODY_CASES = []
BODY_CASES += _pc_cases("normalize_channels", ["in", "out"])
BODY_CASES += _pc_cases("prelu_scalar", ["in", "out"], dict(slope=0.2))
BODY_CASES += _pc_cases("gelu", ["x"])
BODY_CASES += _pc_cases("tanh_scale", ["x"], dict(s=10.0))
BODY_CASES += _pc_cases("fill_channels", ["out"], dict(v=0.3))
BODY_CASES += _pc_cases("lerp_mask", ["a", "b", "out"], dict(m_cs=3, m_off=1), kind="pos")
BODY_CASES += _pc_cases("add_clamp01", ["a", "b", "out"])
BODY_CASES += _pc_cases("splat_normalize", ["out"])
BODY_CASES += [Case("splat_prep", tag, seed=7, px=px, C=2, kind="noise", zs=0.5, fs=0.5 if tag != "n768" else 0.3, **_win({}, x=(5, 2), z=(3, 1), flow=(4, 2)))
               for tag, px in (("n513", 171), ("n255", 85), ("n768", 256))]                                  # n = px (C + 1)
BODY_CASES += [Case("pad_rgb", tag, seed=3, C=c, H=h, W=w, Hp=hp, Wp=wp, out_cs=7, out_off=2)                # n = Hp Wp
               for tag, c, h, w, hp, wp in (("n513", 4, 20, 17, 27, 19), ("n240", 3, 12, 20, 12, 20), ("n256", 3, 9, 11, 16, 16))]
BODY_CASES += [Case("clamp_crop", tag, seed=4, C=3, H=h, W=w, Hp=hp, Wp=wp, in_cs=6, in_off=2)               # n = H W C
               for tag, h, w, hp, wp in (("n513", 9, 19, 16, 32), ("n255", 5, 17, 5, 17), ("n768", 16, 16, 16, 24))]
BODY_CASES += [Case("pixel_shuffle2", tag, seed=5, N=n, H=h, W=w, C=3, **_win({}, **{"in": (14, 1), "out": (5, 1)}))   # n = 4 N H W C: a multiple of 4
               for tag, n, h, w in (("n2052-tail4", 3, 3, 19), ("n252", 3, 1, 7), ("n768", 2, 4, 8))]
BODY_CASES += [Case("window_partition", tag, seed=6, B=b, h=h, w=w, C=c, K=k, sh=sh, sw=sw, inverse=inv, **_win({}, **{"in": (c + 2, 1), "out": (c + 3, 2)}))
               for tag, b, h, w, c, k, sh, sw, inv in (("n513-fwd", 3, 9, 19, 1, 1, 4, 9, 0), ("n240-fwd", 2, 4, 6, 5, 2, 1, 1, 0), ("n240-inv", 2, 4, 6, 5, 2, 1, 1, 1),
                                                       ("n256-inv", 2, 8, 8, 2, 2, 0, 0, 1), ("n768-fwd-k4", 2, 8, 16, 3, 4, 1, 2, 0))]     # n = B h w C
# vfi_bmm_nt: the 4x4-tile body needs K % 4 == 0, a_cs % 4 == 0, b_cs % 4 == 0 and both pointers 16-byte aligned (gmfss_ops.hip);
# n = nb ceil(M/4) ceil(N/4) there, nb M N in the scalar body
BODY_CASES += [Case("bmm_nt", tag, seed=8, nb=nb, M=m, N=n, K=k, alpha=0.25, kind="pos", a_cs=acs, a_off=ao, b_cs=bcs, b_off=bo)
               for tag, nb, m, n, k, acs, ao, bcs, bo in (
                   ("tile4-n24-10x13", 2, 10, 13, 16, 24, 4, 20, 0), ("tile4-n513", 3, 36, 76, 16, 20, 4, 16, 0), ("tile4-n256", 2, 30, 61, 8, 12, 0, 8, 0),
                   ("scalar-K5-n513", 3, 9, 19, 5, 8, 0, 12, 4), ("scalar-K5-n70", 2, 5, 7, 5, 7, 1, 5, 0), ("scalar-K6-n256", 2, 8, 16, 6, 8, 0, 8, 0),
                   ("scalar-misaligned-n260", 2, 10, 13, 16, 20, 1, 20, 0), ("scalar-misaligned-b-n70", 2, 5, 7, 16, 20, 0, 24, 1))]
BODY_CASES += [Case("bmm_nn", tag, seed=9, nb=nb, M=m, N=n, C=c, kind="pos", v_cs=c + 3, v_off=1, out_cs=c + 2, out_off=2)   # n = nb M C
               for tag, nb, m, n, c in (("n513", 3, 9, 11, 19), ("n70", 2, 5, 9, 7), ("n256", 2, 8, 5, 16))]
BODY_CASES += [Case("softmax_rows", tag, seed=10, nb=nb, rows=r, cols=c, period=per, fill=fill, kind=kind, gap=gap)          # n = nb rows
               for tag, nb, r, c, per, fill, kind, gap in (
                   ("n513-nomask", 3, 171, 7, 0, 0.0, "pos", 0), ("n40-mask100-period4", 8, 5, 9, 4, -100.0, "noise", 0), ("n256-mask1e9-period4", 8, 32, 6, 4, -1e9, "noise", 0),
                   ("n6-cols1", 2, 3, 1, 0, 0.0, "noise", 0), ("n6-cols1-mask", 2, 3, 1, 2, -100.0, "noise", 0), ("n257-gap200", 1, 257, 5, 0, 0.0, "noise", 200.0))]
for op, extra, fc in (("convex_upsample", {}, 2), ("convex_upsample_c", dict(FC=4), 4)):         # n = N H W K^2: tails are multiples of K^2
    shapes = [("k2-n516-tail4", 3, 1, 43, 2), ("k2-n252", 3, 3, 7, 2), ("k2-n512", 2, 4, 16, 2), ("k4-n528-tail16", 3, 1, 11, 4)]
    shapes += [(f"k{k}-{h}x{w}", 2, h, w, k) for k in (2, 4) for h, w in ((1, 1), (2, 3), (5, 7))]
    BODY_CASES += [Case(op, tag, seed=11, N=n, H=h, W=w, K=k, kind="pos", **extra, **_win({}, mask=(9 * k * k + 3, 2), flow=(fc + 2, 1), out=(fc + 3, 1)))
                   for tag, n, h, w, k in shapes]
BODY_CASES += [Case("resize_bilinear_ac", tag, seed=12, N=n, Hi=hi, Wi=wi, Ho=ho, Wo=wo, C=3, post_mul=pm, kind=kind, **_win({}, **{"in": (5, 1), "out": (4, 1)}))   # n = N Ho Wo
               for tag, n, hi, wi, ho, wo, pm, kind in (
                   ("n513-9x15to9x19", 3, 9, 15, 9, 19, 1.0, "noise"), ("n616-9x15to14x22", 2, 9, 15, 14, 22, 0.5, "pos"), ("x2-n256", 2, 4, 8, 8, 16, 2.0, "noise"),
                   ("identity-n70", 2, 5, 7, 5, 7, 1.0, "noise"), ("Hout1", 2, 6, 7, 1, 9, 1.0, "noise"), ("Wout1", 2, 6, 7, 5, 1, 1.0, "noise"), ("Hin1", 2, 1, 7, 4, 9, 1.0, "noise"))]
SAMPLER_WIN = dict(in_cs=6, in_off=1, flow_cs=4, flow_off=2, out_cs=5, out_off=1)
BODY_CASES += [Case("flow_sample", tag, seed=13, N=n, H=h, W=w, C=3, kind="noise", flow=fl, **SAMPLER_WIN)                  # n = N H W
               for tag, n, h, w, fl in (("2x2-mixed", 3, 2, 2, "mixed"), ("3x5-mixed", 3, 3, 5, "mixed"), ("12x18-mixed", 2, 12, 18, "mixed"), ("n513-mixed", 3, 9, 19, "mixed"),
                                        ("n256-rand", 2, 8, 16, "rand"), ("3x5-zero", 2, 3, 5, "zero"))]
BODY_CASES += [Case("flow_sample", "12x18-rand-pos", seed=13, N=2, H=12, W=18, C=3, kind="pos", flow="rand", **SAMPLER_WIN)]
METRIC_WIN = dict(img_cs=5, img_off=1, f_cs=4, f_off=2, out_cs=17, out_off=2)
BODY_CASES += [Case("gmfss_metric_inputs", tag, seed=14, H=h, W=w, kind="noise", flow=fl, **METRIC_WIN)                      # n = H W
               for tag, h, w, fl in (("2x2-mixed", 2, 2, "mixed"), ("3x5-mixed", 3, 5, "mixed"), ("12x18-mixed", 12, 18, "mixed"), ("n513-rand", 27, 19, "rand"),
                                     ("n256-rand", 16, 16, "rand"), ("12x18-zero", 12, 18, "zero"), ("3x5-far", 3, 5, "far"), ("12x18-far", 12, 18, "far"))]
BODY_CASES += [Case("ifunet_blend", tag, seed=15, H=h, W=w, Hp=hp, Wp=wp, kind="pos", img_cs=5, img_off=1, m_cs=3, m_off=2)   # n = H W
               for tag, h, w, hp, wp in (("n513-crop", 27, 19, 32, 32), ("n15", 3, 5, 3, 5), ("n256-crop", 16, 16, 16, 20))]
# vfi_instnorm_apply: n = N HW C; the four relu1 / add / relu2 forms, the add operand a window
BODY_CASES += [Case("instnorm_apply", tag, seed=16, N=n, HW=hw, C=c, relu1=r1, add=add, relu2=r2, cs=c + 2, off=1, out_cs=c + 3, out_off=2, add_cs=c + 1, add_off=1)
               for tag, n, hw, c, r1, add, r2 in (("n513-plain", 3, 57, 3, 0, 0, 0), ("n252-relu", 2, 63, 2, 1, 0, 0), ("n768-add-relu2", 2, 16, 24, 0, 1, 1), ("n1200-relu-add", 2, 600, 1, 1, 1, 0))]
# vfi_instnorm_stats: strips = min(workspace / (N C 16 bytes), 1024) >= 64.  Device: instnorm_partial_wg_kernel while C <= 256
# (instnorm_partial_wg_fits), else instnorm_partial_body with n = N strips C; always instnorm_final_wave_kernel.  Host: both bodies.
INSTNORM_STATS_CASES = [Case("instnorm_stats", tag, seed=17, N=2, HW=hw, C=c, cs=c + 3, off=2, strips=s, mean=mu, sigma=sg)
                        for tag, hw, c, s, mu, sg in (
                            ("C1-HW4099-strips64", 4099, 1, 64, 0.3, 1.0), ("C24-HW600-strips100", 600, 24, 100, 0.3, 1.0), ("C24-HW63-strips64-empty", 63, 24, 64, 0.3, 1.0),
                            ("C64-HW1-strips64", 1, 64, 64, 0.3, 1.0), ("C64-HW4099-strips1500-capped", 4099, 64, 1500, 0.3, 1.0), ("C96-HW600-strips64", 600, 96, 64, -2.0, 3.0),
                            ("C96-HW4099-strips100", 4099, 96, 100, 0.3, 1.0), ("C256-HW63-strips100", 63, 256, 100, 0.3, 1.0), ("C256-HW600-strips64", 600, 256, 64, 0.3, 1.0),
                            ("C320-HW600-strips64-body", 600, 320, 64, 0.3, 1.0), ("C320-HW63-strips65-body-tail", 63, 320, 65, 0.3, 1.0),
                            ("C24-HW600-mean1000-sigma0.01", 600, 24, 64, 1000.0, 0.01), ("C320-HW600-mean1000-sigma0.01-body", 600, 320, 64, 1000.0, 0.01))]
BODY_CASES += INSTNORM_STATS_CASES

# vfi_warp_rife (rife40_ops.hip): C == 3 -> warp_rife_c_kernel<3>; else C % 4 == 0 && in_cs % 4 == 0 && out_cs % 4 == 0 && in and out
# pointers 16-byte aligned -> warp_rife_v4_kernel; else warp_rife_kernel.  The flow is channels 2..3 of a 4-channel tensor.
def _warp(tag, n, h, w, c, fl, in_cs, in_off, out_cs, out_off, kind="noise"):
    return Case("warp_rife", tag, seed=20 + c, N=n, H=h, W=w, C=c, kind=kind, flow=fl, in_cs=in_cs, in_off=in_off, flow_cs=4, flow_off=2, out_cs=out_cs, out_off=out_off)


RIFE_CASES = []
for tag, c, ics, ioff, ocs, ooff in (("c3-template", 3, 6, 1, 5, 1), ("c4-v4", 4, 8, 4, 16, 8), ("c8-v4", 8, 16, 4, 16, 4), ("c8-off1-generic", 8, 16, 1, 16, 4),
                                     ("c8-cs9-generic", 8, 9, 0, 16, 4), ("c8-out-off1-generic", 8, 16, 4, 16, 1), ("c1-generic", 1, 3, 1, 4, 2), ("c5-generic", 5, 8, 0, 7, 1)):
    RIFE_CASES += [_warp(f"{tag}-2x2-n3-mixed", 3, 2, 2, c, "mixed", ics, ioff, ocs, ooff), _warp(f"{tag}-3x5-n1-mixed", 1, 3, 5, c, "mixed", ics, ioff, ocs, ooff),
                   _warp(f"{tag}-17x31-n3-mixed", 3, 17, 31, c, "mixed", ics, ioff, ocs, ooff), _warp(f"{tag}-17x31-n1-zero", 1, 17, 31, c, "zero", ics, ioff, ocs, ooff),
                   _warp(f"{tag}-2x2-n3-zero", 3, 2, 2, c, "zero", ics, ioff, ocs, ooff),
                   _warp(f"{tag}-2x2-n3-rand-pos", 3, 2, 2, c, "rand", ics, ioff, ocs, ooff, kind="pos")]
RIFE_CASES += [Case("rife40_prep", tag, seed=30, C=c, H=h, W=w, Hp=hp, Wp=wp, t=t)
               for tag, c, h, w, hp, wp, t in (("c3-pad-n513", 3, 20, 17, 27, 19, 0.5), ("c4-pad-n520", 4, 11, 23, 13, 40, 0.25), ("c3-nopad-n256", 3, 16, 16, 16, 16, 0.75))]
_A = dict(seed=31, fillv=None, plant=(), cs=1, calls=((0, 1),))
RIFE_CASES += [
    Case("absmax", "one-element", **{**_A, "px": 1}), Case("absmax", "all-zero", **{**_A, "px": 300, "fillv": 0.0}),
    Case("absmax", "negative-max", **{**_A, "px": 1000, "plant": ((613, 0, -77.5),)}),
    Case("absmax", "last-of-80000", **{**_A, "px": 80000, "plant": ((79999, 0, 55.25),)}),         # 256 x 256 threads: the grid-stride loop wraps
    Case("absmax", "cs4-c2-offsets-0-2-adjacent-outputs", **{**_A, "px": 20000, "cs": 4, "calls": ((0, 2), (2, 2)),
                                                            "plant": ((5, 2, 900.0), (19999, 1, -40.5), (7, 3, 33.0), (11, 0, 12.0))}),
    Case("absmax", "cs4-c2-big-in-excluded", **{**_A, "px": 777, "cs": 4, "calls": ((2, 2), (0, 2)), "plant": ((776, 0, 1e6), (0, 1, -1e6), (400, 3, -64.0))}),
]
RIFE_CASES += [Case("rife40_output", tag, seed=32, B=b, H=h, W=w, Hp=hp, Wp=wp, res=res, kind="pos", w_cs=wcs, w_off=woff, r_cs=5, r_off=1)
               for tag, b, h, w, hp, wp, res, wcs, woff in (("b1-n513-crop", 1, 27, 19, 32, 32, 0, 8, 0), ("b3-n513-crop-res", 3, 27, 19, 32, 32, 1, 8, 0),
                                                            ("b3-n15-window", 3, 3, 5, 3, 5, 0, 11, 2), ("b1-n256-res", 1, 16, 16, 16, 20, 1, 8, 0))]

ALL_CASES = BODY_CASES + RIFE_CASES

# negative controls: (a case, what is wrong with the restatement it is compared against) — each must FAIL the comparison
_by_id = {c.id: c for c in ALL_CASES}
NEGATIVE_BODY = [
    (_by_id["flow_sample-n256-rand"].but(shift=1.0), "tap index off by one"),
    (_by_id["gmfss_metric_inputs-n256-rand"].but(shift=1.0), "tap index off by one"),
    (_by_id["flow_sample-n256-rand"].but(drop=2), "channel dropped from a window"),
    (_by_id["lerp_mask-n513"].but(drop=0), "channel dropped from a window"),
    (_by_id["bmm_nt-tile4-n24-10x13"].but(drop=7), "summand dropped"),
    (_by_id["softmax_rows-n513-nomask"].but(omit=3), "softmax term omitted"),
    (_by_id["ifunet_blend-n15"].but(omit=2), "softmax term omitted"),
]
NEGATIVE_RIFE = [
    (_by_id["warp_rife-c3-template-17x31-n3-mixed"].but(shift=1.0), "tap index off by one"),
    (_by_id["warp_rife-c8-v4-17x31-n3-mixed"].but(drop=7), "channel dropped from a window"),
    (_by_id["rife40_output-b3-n15-window"].but(omit=1), "blend term omitted"),
]
