"""Float64 restatements, error bounds and case tables for the RIFE stage kernels of csrc/rife_ops.hip, one launcher at a time:
stage_in, stage_in0_staged, flow_up, feat_up, stage_trans (cell and quad kernels), stage_trans_x, trans1_conv0a, final_blend,
planar4_up, t_down — reached through the vfi_test_rife_* taps of include/vfi_hip_test.h.  No product code is imported: every op is
stated as the reference formula it implements (vfi_models/rife/rife_arch.py: warp :31-70; IFBlock's F.interpolate calls :238-248,
:263-273; the torch.cat orders of 4.7 / 4.17 :543-548,629-644 and 4.26 :555-583; flow / mask update :645,698-699; blend :721-723,732),
evaluated in float64 on the fp32 inputs.  tests/test_rife_stage_restated_cpu.py ties these restatements to oracle/rife_oracle.py
(a float64 forward whose glue is this file agrees with the oracle's to 1e-11); tests/test_gpu_rife_stage.py runs the tables on the device.

LAYOUTS (rife_ops.hip).  planar4 = C channels as C/4 planes of [H][W] float4.  Frame pack: planar4 [1 + NF][Hp][Wp][4] (plane 0 = rgb,
planes 1.. = features) at Ppool + slot * pack_stride.  F [B][Hp][Wp][4] = (F01 -> frame 0, F23 -> frame 1).  T = a block's output,
planar4 [B][tp][Hs][Ws][4]: tp = 2: (flow delta 4 | mask, -, -, -); tp = 4 (arch 4.26): (flow 4 | mask, g0..g2 | g3..g6 | g7, -, -, -).
The '-' components and the fourth component of the rgb plane are NaN or noise here: nothing may depend on them.

PRIMITIVES.  U = 2^-24; first-order bounds gamma * U * sum|terms| as in tests/small_ops_restated.py, whose Buffers, compare, bilinear,
local_spread, sample, flow_field are reused.  The default -ffp-contract=fast only removes roundings: the unfused number is counted.
  down(x, s)   F.interpolate(x, 1/s, bilinear, align_corners=False), s even: source index s d + s/2 - 1/2: the mean of the pixels s/2 - 1
               and s/2 of every cell, per axis.  The kernels form 0.5 a + 0.5 b per row, then per column: the products are exact, two
               additions: 2 U sum|0.25 x_i|, on top of the mean of the operands' own bounds.  s = 1: the identity, exact.
  up(x, s)     F.interpolate(x, s, bilinear, align_corners=False): source index (d + 1/2) / s - 1/2, clamped at 0, i1 = min(i0 + 1, n - 1);
               wy0 (wx0 a + wx1 b) + wy1 (wx0 c + wx1 d).  bil_index's weights are counted with two roundings each (l and 1 - l; for the
               power-of-two scales used they are in fact exact), each term then passes two products and two additions:
               (2 + 2 + 4) U = 8 U sum|w t|.  s = 1: a copy, exact.  The same count holds for planar4_up (x u) and t_down (/ u).
               The factors x s, / s, x u, / u are powers of two: exact.
  warp(x, f)   rife_arch.py warp(): grid_sample(border, align_corners=True) at pixel + flow: small_ops_restated.sample with R_WARP = 7,
               the coordinate chain of csrc/rife_warp.h: d = 7 U (|p| + size - 1) per axis times the local spread, + 8 U sum|tap w|; zero
               where p is further than d outside the image.  No position is excluded.
  flow update  F = F_prev + up(T[0:4]) * s: the up bound times s and one addition, U |F| (has_prev only).

TWO OUTPUTS OF ONE KERNEL.  The fused transitions write F and warp at exactly that F.  F is compared with float64 of
F_prev + up(T) s; X (A0, the frame) with a restatement that warps at the flow THE DEVICE WROTE, read back (`stages`: a later stage sees
the outputs of the earlier ones).  The flow channels of X are then down(F_dev) / s: two roundings.  final_blend without Fdbg writes no
flow: there the flow's own bound is added to the sampler's position error.

  stage X      per channel: warped channels down(warp bound) + 2 U down|.|; mask / carried features down(up bound) + 2 U down|.|;
               timestep: 0.5 t + 0.5 t = t for every float: exact; padding channels: exactly 0.
  A0           conv0.0 (3x3, stride 2, pad 1, 20 -> 32) + bias + LeakyReLU(0.2) over X at scale 1: sum|w| tol_X + gamma U (sum|w x| + |b|),
               gamma = 184: 180 products and 180 additions in any association (each term passes one product and at most 180 - 1
               additions), the addition of the two K halves, the bias, the product with the slope.  Pixels outside the image are the
               convolution's zero padding (no summand).  LeakyReLU is 1-Lipschitz.
  frame        clamp(a m + b (1 - m), 0, 1), m = sigmoid(v), v = up(T mask): m within SIGMOID_U U m + tol_v / 4, 1 - m one rounding
               more; two products and one addition: 3 U (|a m| + |b (1 - m)|); a saturated sigmoid: 2^-126 (|a| + |b|).

Where the inputs are positive (packs, T, carried features in [0.5, 1]) an expectation carries `mn`, the size of one summand (0.25 of the
largest tap of a warped centre pixel, the smallest weighted tap of an up-resize, one product of the blend, min|w| min|x| of A0), and
compare() asserts mn > tol before it looks at the result.

MUTATIONS.  `mut` names a deliberately wrong restatement (MUTATIONS below); check(case, outs, mut) must then fail.
"""
import ctypes as C
import functools
import zlib
from types import SimpleNamespace

import torch
import torch.nn.functional as Fn

import small_ops_restated as so
from small_ops_restated import FAMILIES_WARP, INF, NAN, R_WARP, SIGMOID_U, TINY, U, Buffers, Case, bilinear, compare, flow_field, sample

G_UP = 8.0        # roundings of one term of an up-resize (module docstring)
G_A0 = 184.0
SENTINEL = -7.0   # what Fdbg holds outside H x W before and after final_blend

MUTATIONS = {
    "centre": "centre offset s/2 instead of s/2 - 1",
    "mask_plane0": "the mask taken from T plane 0",
    "flow_not_div": "the flow channels of X not divided by s",
    "no_times_s": "the flow update without x s",
    "img1_F01": "img1 warped with F01",
    "swap_feat": "two feature channels swapped in the cat order",
    "align_corners": "align_corners=True weights in the up-resize",
    "drop_t": "the timestep channel dropped",
    "zero_tap": "one tap of conv0.0 zeroed",
    "blend_swapped": "a blend of m b + (1 - m) a",
}


# ---------------------------------------------------------------------------------------------------------------- layouts

def to_planar(x):
    """[B,H,W,C] -> planar4 [B,C/4,H,W,4]"""
    B, H, W, Cc = x.shape
    return x.reshape(B, H, W, Cc // 4, 4).permute(0, 3, 1, 2, 4).contiguous()


def round_up(a, b):
    return -(-a // b) * b


# ---------------------------------------------------------------------------------------------------------------- primitives (float64)

def resize(x, Ho, Wo, align_corners=False):
    """F.interpolate(x [B,H,W,C], size (Ho, Wo), bilinear) -> (value, sum|w tap|, smallest |w tap| with w > 0)"""
    _, H, W, _ = x.shape

    def index(n_in, n_out):
        d = torch.arange(n_out, dtype=torch.float64)
        if align_corners:
            src = d * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
        else:
            src = ((d + 0.5) * (n_in / n_out) - 0.5).clamp_min(0)
        i0 = src.floor().clamp_max(n_in - 1)
        l = (src - i0).clamp(0, 1)
        i0 = i0.long()
        return i0, (i0 + 1).clamp_max(n_in - 1), 1 - l, l

    y0, y1, wy0, wy1 = index(H, Ho)
    x0, x1, wx0, wx1 = index(W, Wo)
    out = M = 0.0
    small = None
    for yi, wy in ((y0, wy0), (y1, wy1)):
        for xi, wx in ((x0, wx0), (x1, wx1)):
            w = wy.view(1, -1, 1, 1) * wx.view(1, 1, -1, 1)
            term = x[:, yi][:, :, xi] * w
            out = out + term
            M = M + term.abs()
            s = torch.where(w > 0, term.abs(), torch.full_like(term, INF))
            small = s if small is None else torch.minimum(small, s)
    return out, M, small


def up(x, s, mut=None):
    """-> (value, bound, smallest summand) of the up-resize by s; s = 1: a copy"""
    if s == 1:
        return x, torch.zeros_like(x), x.abs()
    v, M, small = resize(x, x.shape[1] * s, x.shape[2] * s, mut == "align_corners")
    return v, G_UP * U * M, small


def down(x, s, tol=None, mut=None):
    """-> (value, bound, 0.25 min|x_i|) of the down-resize by s of x whose own bound is tol; s = 1: the identity"""
    tol = torch.zeros_like(x) if tol is None else tol
    if s == 1:
        return x, tol, x.abs()
    if mut == "centre":
        x, tol = x.roll((-1, -1), (1, 2)), tol.roll((-1, -1), (1, 2))
    o = s // 2 - 1
    taps = [x[:, o + dy::s, o + dx::s] for dy in (0, 1) for dx in (0, 1)]
    ttol = [tol[:, o + dy::s, o + dx::s] for dy in (0, 1) for dx in (0, 1)]
    v = 0.25 * (taps[0] + taps[1] + taps[2] + taps[3])
    M = 0.25 * (taps[0].abs() + taps[1].abs() + taps[2].abs() + taps[3].abs())
    mn = 0.25 * torch.stack([t.abs() for t in taps]).amin(0)
    return v, 0.25 * (ttol[0] + ttol[1] + ttol[2] + ttol[3]) + 2 * U * M, mn


def warp(img, f2, e2=None):
    """rife_arch.py warp() of img [B,H,W,C] at flow f2 [B,H,W,2] (x, y) -> (value, bound, largest tap).  e2: the flow's own bound, added to
    the position error of the sampler (final_blend without Fdbg)."""
    if e2 is None:
        return sample(img, f2[..., 0], f2[..., 1], True, R_WARP)
    _, H, W, _ = img.shape
    X = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    Y = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    px, py = X + f2[..., 0].double(), Y + f2[..., 1].double() + 0 * X
    out, M, big, D = bilinear(img, px, py, True)

    def pos_err(p, size, e):
        d = R_WARP * U * (p.abs() + (size - 1)) + e
        return torch.where((p < -d) | (p > size - 1 + d), torch.zeros_like(d), d)

    d = pos_err(px, W, e2[..., 0]) + pos_err(py, H, e2[..., 1])
    assert float(d.max()) < 0.5, "local_spread covers position errors below one pixel only"
    return out, d.unsqueeze(-1) * D + 8 * U * M, torch.where(M > 0, big, torch.full_like(big, INF))


def flow_update(Fprev, Tflow, s, mut=None):
    """F_prev + up(T[:, :4], s) * s (rife_arch.py :645, :698) -> (value, bound, smallest summand of the up-resize times s)"""
    v, tol, small = up(Tflow, s, mut)
    k = 1.0 if mut == "no_times_s" else float(s)
    v, tol, small = v * k, tol * k, small * k
    if Fprev is None:
        return v, tol, small
    want = Fprev + v
    return want, tol + U * want.abs(), None


def stage_x(pk0, pk1, t, F, M, Mtol, FEAT, FEATtol, s, CX, mut=None):
    """The next block's input: down(cat(warp(img0, F01), warp(img1, F23), warp(f0, F01), warp(f1, F23), timestep, mask[, carried
    features]), s) and down(F, s) / s behind it, zero padded to CX channels.  pk0 / pk1 [B,Hp,Wp,3 + 4 NF] = (rgb | features) of each
    task's two frames, t [B]; F None: block 0, cat(img0, img1, f0, f1, timestep).  -> (value, bound, summand) [B,Hs,Ws,CX]"""
    B, Hp, Wp, _ = pk0.shape
    tt = t.double().view(B, 1, 1, 1).expand(B, Hp, Wp, 1) * (0.0 if mut == "drop_t" else 1.0)
    zero1 = torch.zeros(B, Hp, Wp, 1, dtype=torch.float64)
    inf1 = torch.full_like(zero1, INF)
    if F is None:
        a, b = pk0, pk1
        ta, tb = torch.zeros_like(a), torch.zeros_like(b)
        ba, bb = a.abs(), b.abs()
    else:
        a, ta, ba = warp(pk0, F[..., 0:2])
        b, tb, bb = warp(pk1, F[..., 0:2] if mut == "img1_F01" else F[..., 2:4])
    parts = [(a[..., :3], ta[..., :3], ba[..., :3]), (b[..., :3], tb[..., :3], bb[..., :3]), (a[..., 3:], ta[..., 3:], ba[..., 3:]),
             (b[..., 3:], tb[..., 3:], bb[..., 3:]), (tt, zero1, inf1)]
    if F is not None:
        parts.append((M, Mtol, M.abs()))
        if FEAT is not None:
            parts.append((FEAT, FEATtol, FEAT.abs()))
    full, ftol, fbig = (torch.cat([p[k] for p in parts], -1) for k in range(3))
    if mut == "swap_feat":
        perm = list(range(full.shape[-1]))
        perm[6], perm[7] = 7, 6
        full, ftol, fbig = full[..., perm], ftol[..., perm], fbig[..., perm]
    v, tol, _ = down(full, s, ftol, mut)
    mn = down(fbig, s, None, mut)[2] if s > 1 else fbig
    ti = 6 + (pk0.shape[-1] - 3) * 2
    tol[..., ti], mn[..., ti] = 0.0, INF                               # the timestep: exact
    if F is not None:
        fv, ft, _ = down(F, s, None, mut)
        k = 1.0 if mut == "flow_not_div" else 1.0 / s
        v, tol, mn = torch.cat([v, fv * k], -1), torch.cat([tol, ft * k], -1), torch.cat([mn, torch.full_like(fv, INF)], -1)
    pad = CX - v.shape[-1]
    assert pad >= 0
    z = torch.zeros(*v.shape[:-1], pad, dtype=torch.float64)
    return torch.cat([v, z], -1), torch.cat([tol, z], -1), torch.cat([mn, torch.full_like(z, INF)], -1)


def blend(a, ta, b, tb, v, tv, mut=None):
    """rife_arch.py :721-723, :732 and the node's clamp: clamp(a m + b (1 - m), 0, 1), m = sigmoid(v) -> (value, bound, smaller product)"""
    m = torch.sigmoid(v)
    om = 1 - m
    if mut == "blend_swapped":
        a, ta, b, tb = b, tb, a, ta
    p0, p1 = a * m, b * om
    dm = SIGMOID_U * U * m + 0.25 * tv
    tol = a.abs() * dm + b.abs() * (dm + U * om) + m * ta + om * tb + 3 * U * (p0.abs() + p1.abs()) + TINY * (a.abs() + b.abs())
    return (p0 + p1).clamp(0, 1), tol, torch.minimum(p0.abs(), p1.abs())


# ---------------------------------------------------------------------------------------------------------------- inputs

TASKS = {
    "b1": ((0,), (1,), (0.3,)),
    "b3": ((2, 1, 2), (0, 0, 1), (0.0, 1.0, 0.3)),                      # slot1 < slot0; slots 2, 1 and 0 each used by two tasks
    "b32": (tuple(b % 4 for b in range(32)), tuple((b + 1 + b // 4) % 4 for b in range(32)), tuple(b / 31 for b in range(32))),
    "b1p": ((1,), (0,), (0.75,)),                                       # timesteps in [0.5, 1]: the A0 cases
    "b3p": ((2, 1, 2), (0, 0, 1), (0.5, 1.0, 0.625)),
}


@functools.lru_cache(None)
def _mixed(H, W, nfam):
    return flow_field(so._g(77), 2, H, W, "mixed", nfam)


def flows(g, B, H, W, kind):
    """[B,H,W,4] fp32.  'mixed': flow_field's families (integer, +-half, +-1e-6, just past either border, +-1e4, +-1e30) in F01 and in F23,
    task b's fields rolled by b pixels; 'mixed8': the same without +-1e4 and +-1e30; 'rand': N(0, 1.5); 'a0': moderate flows (2.5 .. 8 px either way, so that |F + 2 up(T)| >= 0.5 for T in
    [0.5, 1]) with whole rows and columns pushed out of the frame on every side."""
    if kind in ("mixed", "mixed8"):
        base = _mixed(H, W, len(FAMILIES_WARP) if kind == "mixed" else 8)
        return torch.stack([torch.cat([base[0].roll(b, 1), base[1].roll(b, 0)], -1) for b in range(B)])
    r = so._noise(g, B, H, W, 4, s=1.5)
    if kind == "rand":
        return r
    f = torch.where(r >= 0, torch.ones_like(r), -torch.ones_like(r)) * (2.5 + r.abs())
    f[:, 5, :, 1] = -8.0                      # row 5 of frame 0: above the top
    f[:, :, 7, 0] = float(W)                  # column 7 of frame 0: past the right edge
    f[:, H - 2, :, 3] = 6.0                   # frame 1: below the bottom
    f[:, :, 3, 2] = -9.0                      # frame 1: left of column 0
    return f


def make_T(g, kind, B, Hs, Ws, tp, junk=NAN):
    """channel-last [B,Hs,Ws,4 tp]; the components no kernel may use are `junk`"""
    Tc = so._make(g, kind, B, Hs, Ws, 4 * tp)
    Tc[..., 5:8] = junk
    if tp == 4:
        Tc[..., 5:13] = so._make(g, kind, B, Hs, Ws, 8)
        Tc[..., 13:16] = junk
    return Tc


def add_packs(B, g, P, NF):
    """the pool of frame packs and the task table -> (pk0, pk1 float64 [B,Hp,Wp,3 + 4 NF], t fp32 [B], the six leading tap arguments)"""
    s0, s1, ts = TASKS[P.tasks]
    n = max(s0 + s1) + 1
    pk = so._make(g, P.kind, n, 1 + NF, P.Hp, P.Wp, 4)
    pack = (1 + NF) * P.Hp * P.Wp * 4
    stride = pack + getattr(P, "gap", 0)
    body = torch.full((n, stride), NAN)
    body[:, :pack] = pk.reshape(n, -1)
    B.add("P", body)
    cl = torch.cat([pk[:, 0, ..., :3]] + [pk[:, 1 + j] for j in range(NF)], -1).double()
    t = torch.tensor(ts, dtype=torch.float32)
    nb = len(s0)
    args = [B.ptr("P"), stride, (C.c_int * nb)(*s0), (C.c_int * nb)(*s1), (C.c_float * nb)(*ts), nb]
    return cl[list(s0)], cl[list(s1)], t, args


def _xout(B, nb, CX, Hs, Ws):
    B.add("X", None, nb * (CX // 4) * Hs * Ws, 4, role="out")


def _pos(P):
    return P.kind == "pos"


def _planar_expect(buf, v, tol, mn=None):
    return dict(buf=buf, want=to_planar(v), tol=to_planar(tol), mn=None if mn is None else to_planar(mn))


# ---------------------------------------------------------------------------------------------------------------- ops
# op(P, B) -> SimpleNamespace(calls=[(entry point, args)], stages=[f(outs) -> expectations], options={name: value})

def op_stage_in(P, B):
    """stage_in_launch: X of a block from the packs (and, from block 1 on, F, M and the carried features FEAT)."""
    g = so._g(P.seed)
    pk0, pk1, t, targs = add_packs(B, g, P, P.NF)
    nb, Hs, Ws = len(t), P.Hp // P.s, P.Wp // P.s
    F = M = FEAT = None
    ptr = [None, None, None]
    if P.has_flow:
        F = flows(g, nb, P.Hp, P.Wp, P.flow)
        M = so._make(g, P.kind, nb, P.Hp, P.Wp, 1)
        B.add("F", F.reshape(-1, 4))
        B.add("M", M.reshape(-1, 1))
        ptr[0], ptr[1] = B.ptr("F"), B.ptr("M")
        if P.NX:
            FEAT = so._make(g, P.kind, nb, P.Hp, P.Wp, 8)
            B.add("FEAT", to_planar(FEAT).reshape(-1, 4))
            ptr[2] = B.ptr("FEAT")
    elif getattr(P, "stray_feat", False):          # FEAT without a flow is ignored by the launcher: NaN, so a read would show
        B.add("FEAT", torch.full((nb * 2 * P.Hp * P.Wp, 4), NAN))
        ptr[2] = B.ptr("FEAT")
    _xout(B, nb, P.CX, Hs, Ws)

    def st(outs, mut):
        d = lambda x: None if x is None else x.double()
        z = lambda x: None if x is None else torch.zeros_like(x, dtype=torch.float64)
        v, tol, mn = stage_x(pk0, pk1, t, d(F), d(M), z(M), d(FEAT), z(FEAT), P.s, P.CX, mut)
        return [_planar_expect("X", v, tol, mn if _pos(P) else None)]

    args = targs + ptr + [B.ptr("X"), P.Hp, P.Wp, P.s, P.CX, P.NF, int(P.has_flow)]
    return SimpleNamespace(calls=[("vfi_test_rife_stage_in", args)], stages=[st], options={})


def op_stage_in0_staged(P, B):
    """stage_in0_staged_launch: block 0's X at block scale 8 from the slots' staging images — cat(rgb0, rgb1, f0, f1, timestep, 0) per
    cell; the timestep through 0.5 t + 0.5 t twice.  A permutation: exact."""
    g = so._g(P.seed)
    s0, s1, ts = TASKS[P.tasks]
    n, nb = max(s0 + s1) + 1, len(s0)
    cells = (P.Hp // 8) * (P.Wp // 8)
    S = so._noise(g, n, 2, cells, 4)
    S[:, 0, :, 3] = NAN
    stride = 8 * cells + getattr(P, "gap", 0)
    body = torch.full((n, stride), NAN)
    body[:, :8 * cells] = S.reshape(n, -1)
    B.add("S", body)
    _xout(B, nb, 16, P.Hp // 8, P.Wp // 8)

    def st(outs, mut):
        t = torch.tensor(ts, dtype=torch.float32).view(nb, 1, 1).expand(nb, cells, 1) * (0.0 if mut == "drop_t" else 1.0)
        a, c = S[list(s0)], S[list(s1)]
        x = torch.cat([a[:, 0, :, :3], c[:, 0, :, :3], a[:, 1], c[:, 1], t, torch.zeros(nb, cells, 1)], -1)
        if mut == "swap_feat":
            perm = list(range(16))
            perm[6], perm[7] = 7, 6
            x = x[..., perm]
        return [dict(buf="X", want=to_planar(x.view(nb, 1, cells, 16)).double(), tol=None)]

    args = [B.ptr("S"), stride, (C.c_int * nb)(*s0), (C.c_int * nb)(*s1), (C.c_float * nb)(*ts), nb, B.ptr("X"), P.Hp, P.Wp]
    return SimpleNamespace(calls=[("vfi_test_rife_stage_in0_staged", args)], stages=[st], options={})


def _add_T_F(P, B, g, nb, s, tp, has_prev, inplace=True):
    Hs, Ws = P.Hp // s, P.Wp // s
    Tc = make_T(g, P.tkind, nb, Hs, Ws, tp)
    B.add("T", to_planar(Tc).reshape(-1, 4))
    Fp = flows(g, nb, P.Hp, P.Wp, P.flow) if has_prev else None
    if inplace:
        B.add("F", None if Fp is None else Fp.reshape(-1, 4), nb * P.Hp * P.Wp, 4, role="inout" if has_prev else "out")
    else:
        B.add("F", Fp.reshape(-1, 4))
    return Tc.double(), None if Fp is None else Fp.double()


def _mask_of(Td, mut):
    k = 0 if mut == "mask_plane0" else 4
    return Td[..., k:k + 1]


def _f_expect(P, Fp, Td, s, mut, buf="F"):
    v, tol, small = flow_update(Fp, Td[..., 0:4], s, mut)
    return dict(buf=buf, want=v, tol=tol, mn=small if P.tkind == "pos" and small is not None else None)


def op_flow_up(P, B):
    """flow_up_launch: F (+)= up(T[:, :4], s) * s, M = up(T[:, 4:5], s)   (rife_arch.py :262-276, :645, :698)."""
    g = so._g(P.seed)
    nb = P.B
    Td, Fp = _add_T_F(P, B, g, nb, P.s, P.tp, P.has_prev)
    B.add("M", None, nb * P.Hp * P.Wp, 1, role="out")

    def st(outs, mut):
        m, mt, ms = up(_mask_of(Td, mut), P.s, mut)
        return [_f_expect(P, Fp, Td, P.s, mut), dict(buf="M", want=m, tol=mt, mn=ms if P.tkind == "pos" else None)]

    args = [B.ptr("T"), B.ptr("F"), B.ptr("M"), nb, P.Hp, P.Wp, P.s, P.tp, int(P.has_prev)]
    return SimpleNamespace(calls=[("vfi_test_rife_flow_up", args)], stages=[st], options={})


def op_feat_up(P, B):
    """feat_up_launch: FEAT = up(T[:, 5:13], s), the 8 channels arch 4.26 carries to the next block (rife_arch.py :267-273)."""
    g = so._g(P.seed)
    nb = P.B
    Tc = make_T(g, P.tkind, nb, P.Hp // P.s, P.Wp // P.s, 4)
    B.add("T", to_planar(Tc).reshape(-1, 4))
    B.add("FEAT", None, nb * 2 * P.Hp * P.Wp, 4, role="out")

    def st(outs, mut):
        v, tol, small = up(Tc[..., 5:13].double(), P.s, mut)
        return [_planar_expect("FEAT", v, tol, small if P.tkind == "pos" else None)]

    return SimpleNamespace(calls=[("vfi_test_rife_feat_up", [B.ptr("T"), B.ptr("FEAT"), nb, P.Hp, P.Wp, P.s])], stages=[st], options={})


def _op_trans(P, B, x):
    g = so._g(P.seed)
    NF, tp, CX = (1, 4, 32) if x else (P.NF, 2, round_up(12 + 8 * P.NF, 8))
    pk0, pk1, t, targs = add_packs(B, g, P, NF)
    nb, sn = len(t), P.s_next
    Td, Fp = _add_T_F(P, B, g, nb, 2 * sn, tp, P.has_prev)
    _xout(B, nb, CX, P.Hp // sn, P.Wp // sn)

    def st_f(outs, mut):
        return [_f_expect(P, Fp, Td, 2 * sn, mut)]

    def st_x(outs, mut):
        Fd = outs["F"].view(nb, P.Hp, P.Wp, 4).double()
        m, mt, _ = up(_mask_of(Td, mut), 2 * sn, mut)
        ft, ftt = (up(Td[..., 5:13], 2 * sn, mut)[:2]) if x else (None, None)
        v, tol, mn = stage_x(pk0, pk1, t, Fd, m, mt, ft, ftt, sn, CX, mut)
        return [_planar_expect("X", v, tol, mn if _pos(P) and P.tkind == "pos" else None)]

    name = "vfi_test_rife_stage_trans_x" if x else "vfi_test_rife_stage_trans"
    args = targs + [B.ptr("T"), B.ptr("F"), B.ptr("X"), P.Hp, P.Wp, 2 * sn, sn] + ([] if x else [NF]) + [CX, int(P.has_prev)]
    return SimpleNamespace(calls=[(name, args)], stages=[st_f, st_x], options=dict(stage_quad=P.quad, xcd_bands=P.xcd))


def op_stage_trans(P, B):
    """stage_trans_launch (stage_trans_kernel / stage_trans_quad_kernel<.., 0>): flow_up of block i and stage_in of block i + 1 in one pass."""
    return _op_trans(P, B, False)


def op_stage_trans_x(P, B):
    """stage_trans_x_launch (stage_trans_x_kernel / stage_trans_quad_kernel<.., 8>): the same for arch 4.26 — the carried features
    up(T[:, 5:13]) sit between mask and flow (rife_arch.py :555-583)."""
    return _op_trans(P, B, True)


def conv0a_weights(seed):
    """OIHW [32][20][3][3] with |w| in [0.5, 1] and random signs, bias N(0, 1)"""
    g = so._g(seed)
    w = so._pos(g, 32, 20, 3, 3) * torch.where(torch.rand(32, 20, 3, 3, generator=g) < 0.5, -1.0, 1.0)
    return w, so._noise(g, 32)


def op_trans1_conv0a(P, B):
    """trans1_conv0a_launch: Fout = Fin + up(T, 2) * 2; A0 = LeakyReLU(conv0.0(X) + bias, slope) with X the scale-1 input of the last
    block at Fout (never stored)."""
    g = so._g(P.seed)
    pk0, pk1, t, targs = add_packs(B, g, P, 1)
    nb = len(t)
    Td, Fin = _add_T_F(P, B, g, nb, 2, 2, True, inplace=False)
    B.add("Fout", None, nb * P.Hp * P.Wp, 4, role="out")
    B.add("A0", None, nb * (P.Hp // 2) * (P.Wp // 2), 32, role="out")
    w, bias = conv0a_weights(P.seed + 1000)

    def st_f(outs, mut):
        return [_f_expect(P, Fin, Td, 2, mut, buf="Fout")]

    def st_a(outs, mut):
        Fd = outs["Fout"].view(nb, P.Hp, P.Wp, 4).double()
        m, mt, _ = up(_mask_of(Td, mut), 2, mut)
        x, xt, _ = stage_x(pk0, pk1, t, Fd, m, mt, None, None, 1, 20, mut)
        wd = w.double().clone()
        if mut == "zero_tap":
            wd[:, :, 2, 0] = 0
        nchw = lambda q: q.permute(0, 3, 1, 2)
        pre = Fn.conv2d(nchw(x), wd, bias.double(), 2, 1)
        tol = Fn.conv2d(nchw(xt), wd.abs(), None, 2, 1) + G_A0 * U * (Fn.conv2d(nchw(x.abs()), wd.abs(), None, 2, 1) + bias.double().abs().view(1, -1, 1, 1))
        a0 = Fn.leaky_relu(pre, P.slope)
        mn = None
        if _pos(P) and P.tkind == "pos":
            mn = torch.full_like(a0, float(w.abs().min()) * float(x.abs().amin()))
        return [dict(buf="A0", want=a0.permute(0, 2, 3, 1), tol=tol.permute(0, 2, 3, 1), mn=None if mn is None else mn.permute(0, 2, 3, 1))]

    args = targs + [B.ptr("T"), B.ptr("F"), B.ptr("Fout"), w.data_ptr(), bias.data_ptr(), B.ptr("A0"), P.Hp, P.Wp, C.c_float(P.slope)]
    return SimpleNamespace(calls=[("vfi_test_rife_trans1_conv0a", args)], stages=[st_f, st_a], options=dict(fuse0a=P.fuse0a))


def op_final_blend(P, B):
    """final_blend_launch: F = F_prev + up(T[:, :4], s) * s (to Fdbg inside H x W if given), frame = clamp(warp(img0, F01) m + warp(img1, F23)
    (1 - m), 0, 1)[:H, :W] with m = sigmoid(up(T[:, 4:5], s))."""
    g = so._g(P.seed)
    pk0, pk1, t, targs = add_packs(B, g, P, 1)
    nb, H, W = len(t), P.H, P.W
    Td, Fp = _add_T_F(P, B, g, nb, P.s, P.tp, True, inplace=False)
    B.add("out", None, nb * H * W, 3, role="out")
    if P.fdbg:
        B.add("Fdbg", torch.full((nb * P.Hp * P.Wp, 4), SENTINEL), role="inout")
    inside = torch.zeros(nb, P.Hp, P.Wp, 4, dtype=torch.bool)
    inside[:, :H, :W] = True

    def st_f(outs, mut):
        e = _f_expect(P, Fp, Td, P.s, mut, buf="Fdbg")
        e["want"] = torch.where(inside, e["want"], torch.full_like(e["want"], SENTINEL))
        e["tol"] = torch.where(inside, e["tol"], torch.zeros_like(e["tol"]))
        e["mn"] = None
        return [e]

    def st_o(outs, mut):
        if P.fdbg:
            Fd, e2a, e2b = outs["Fdbg"].view(nb, P.Hp, P.Wp, 4).double(), None, None
            Fd = torch.where(inside, Fd, torch.zeros_like(Fd))
        else:
            Fd, ft, _ = flow_update(Fp, Td[..., 0:4], P.s, mut)
            e2a, e2b = ft[..., 0:2], ft[..., 2:4]
        a, ta, _ = warp(pk0[..., :3], Fd[..., 0:2], e2a)
        b, tb, _ = warp(pk1[..., :3], Fd[..., 0:2] if mut == "img1_F01" else Fd[..., 2:4], e2a if mut == "img1_F01" else e2b)
        v, tv, _ = up(_mask_of(Td, mut), P.s, mut)
        o, tol, mn = blend(a, ta, b, tb, v, tv, mut)
        crop = lambda q: q[:, :H, :W]
        return [dict(buf="out", want=crop(o), tol=crop(tol), mn=crop(mn) if _pos(P) and P.tkind == "pos" else None)]

    args = targs + [B.ptr("T"), B.ptr("F"), B.ptr("out"), B.ptr("Fdbg") if P.fdbg else None, H, W, P.Hp, P.Wp, P.s, P.tp]
    return SimpleNamespace(calls=[("vfi_test_rife_final_blend", args)], stages=([st_f] if P.fdbg else []) + [st_o], options=dict(xcd_bands=P.xcd))


def op_planar4_up(P, B):
    """planar4_up_launch: IFBlock's F.interpolate(x, scale_factor=u) for block scales below 1 (rife_arch.py :238-248); the flow plane x u."""
    g = so._g(P.seed)
    x = so._make(g, P.kind, P.B, P.Hp, P.Wp, P.CX)
    B.add("X1", to_planar(x).reshape(-1, 4))
    B.add("X", None, P.B * (P.CX // 4) * P.u * P.Hp * P.u * P.Wp, 4, role="out")

    def st(outs, mut):
        v, tol, small = up(x.double(), P.u, mut)
        k = torch.ones(P.CX, dtype=torch.float64)
        if P.flow_plane >= 0:
            k[4 * P.flow_plane:4 * P.flow_plane + 4] = P.u
        return [_planar_expect("X", v * k, tol * k, small * k if _pos(P) else None)]

    args = [B.ptr("X1"), B.ptr("X"), P.B, P.Hp, P.Wp, P.u, P.CX, P.flow_plane]
    return SimpleNamespace(calls=[("vfi_test_rife_planar4_up", args)], stages=[st], options={})


def op_t_down(P, B):
    """t_down_launch: F.interpolate(tmp, scale_factor=1/u) of a block that ran above the frame resolution (:263-266), the flow plane / u."""
    g = so._g(P.seed)
    Tc = so._make(g, P.kind, P.B, P.u * P.Hp, P.u * P.Wp, 4 * P.tp)
    B.add("T", to_planar(Tc).reshape(-1, 4))
    B.add("T1", None, P.B * P.tp * P.Hp * P.Wp, 4, role="out")

    def st(outs, mut):
        v, M, small = resize(Tc.double(), P.Hp, P.Wp)
        k = torch.ones(4 * P.tp, dtype=torch.float64)
        k[0:4] = 1.0 / P.u
        return [_planar_expect("T1", v * k, G_UP * U * M * k, small * k if _pos(P) else None)]

    return SimpleNamespace(calls=[("vfi_test_rife_t_down", [B.ptr("T"), B.ptr("T1"), P.B, P.Hp, P.Wp, P.u, P.tp])], stages=[st], options={})


OPS = {k[3:]: v for k, v in list(globals().items()) if k.startswith("op_")}
DEFAULT_OPTIONS = dict(stage_quad=14, xcd_bands=0, fuse0a=1)


# ---------------------------------------------------------------------------------------------------------------- runners

def prepare(case, device="cpu"):
    B = Buffers(device)
    return B, OPS[case.op](SimpleNamespace(**case.p), B)


def launch(lib, case, device, stream, sync, ck):
    """One launch of the case's kernel on `device` under its options -> (op, the window of every buffer after the call); guards checked."""
    B, op = prepare(case, device)
    try:
        for k, v in op.options.items():
            assert lib.vfi_test_set_option(k.encode(), v) == 0, k
        for name, args in op.calls:
            ck(getattr(lib, name)(*args, stream), name)
        sync()
    finally:
        for k in op.options:
            lib.vfi_test_set_option(k.encode(), DEFAULT_OPTIONS[k])
    return op, B.finish()


def emulate(case):
    """What a perfect device would leave: every stage's float64 result rounded to fp32, later stages fed from the earlier ones."""
    B, op = prepare(case)
    outs = {}
    for st in op.stages:
        for e in st(outs, None):
            outs[e["buf"]] = e["want"].float().reshape(B.b[e["buf"]].px, B.b[e["buf"]].C)
    return op, outs


def expectations(run, mut=None):
    op, outs = run
    return [e for st in op.stages for e in st(outs, mut)]


def check(case, run, mut=None):
    """run: what launch() or emulate() returned -> the largest err / tol of the case; raises AssertionError as compare() does"""
    worst = 0.0
    for st in run[0].stages:
        for e in st(run[1], mut):
            if mut:
                e["mn"] = None          # the summand condition belongs to the right restatement
            r = compare(run[1][e["buf"]], e, f"{case.id}{'~' + mut if mut else ''}:{e['buf']}")
            worst = max(worst, r or 0.0)
    return worst


# ---------------------------------------------------------------------------------------------------------------- case tables

SIZES = ((64, 64), (64, 192), (192, 64), (128, 320))      # Hp x Wp: one tile; odd tile counts; counts that are no multiple of 8; partial tiles


def _case(op, tag, **p):
    p.setdefault("kind", "noise")
    p.setdefault("tasks", "b1")
    p.setdefault("gap", 0)
    return Case(op, tag, seed=zlib.crc32(f"{op}-{tag}".encode()) % 2 ** 31, **p)          # a case's inputs do not depend on the others


def _sz(i):
    return SIZES[i % 4]


STAGE_IN_CASES, i = [], 0
for hf in (0, 1):
    for s in (1, 2, 8, 16, 32):
        for NF, NX in ((1, 0), (2, 0)) + (((1, 8),) if hf else ()):
            (hp, wp), i = _sz(i), i + 1
            STAGE_IN_CASES.append(_case("stage_in", f"flow{hf}-s{s}-nf{NF}-nx{NX}-{hp}x{wp}", Hp=hp, Wp=wp, s=s, NF=NF, NX=NX, has_flow=hf, flow="mixed",
                                        CX=round_up(7 + 8 * NF + (5 + NX if hf else 0), 8), kind="pos" if i % 2 else "noise", tasks="b3" if s >= 8 and hp * wp <= 64 * 192 else "b1",
                                        gap=8 if i % 3 == 0 else 0))
STAGE_IN_CASES += [
    _case("stage_in", "flow0-s8-nf1-feat-ignored-64x64", Hp=64, Wp=64, s=8, NF=1, NX=0, has_flow=0, flow="mixed", CX=16, stray_feat=True),
    _case("stage_in", "flow1-s4-nf1-nx0-b32-64x64", Hp=64, Wp=64, s=4, NF=1, NX=0, has_flow=1, flow="mixed", CX=24, tasks="b32", gap=8),
    _case("stage_in", "flow1-s4-nf1-nx8-rand-pos-128x320", Hp=128, Wp=320, s=4, NF=1, NX=8, has_flow=1, flow="rand", CX=32, kind="pos"),
]

STAGED_CASES = [_case("stage_in0_staged", f"{tk}-{hp}x{wp}-gap{gap}", Hp=hp, Wp=wp, tasks=tk, gap=gap)
                for (hp, wp), tk, gap in ((SIZES[0], "b1", 0), (SIZES[1], "b3", 8), (SIZES[2], "b1", 8), (SIZES[3], "b3", 0), (SIZES[0], "b32", 8))]

FLOW_UP_CASES, i = [], 0
for s in (1, 2, 4, 8, 16):
    for tp in (2, 4):
        (hp, wp), i = _sz(i), i + 1
        FLOW_UP_CASES.append(_case("flow_up", f"s{s}-tp{tp}-prev-{hp}x{wp}", Hp=hp, Wp=wp, s=s, tp=tp, has_prev=1, B=1 + i % 3, flow="mixed", tkind="pos" if i % 2 else "noise"))
FLOW_UP_CASES += [_case("flow_up", f"s{s}-tp{tp}-first-{hp}x{wp}", Hp=hp, Wp=wp, s=s, tp=tp, has_prev=0, B=2, flow="mixed", tkind="pos")
                  for s, tp, (hp, wp) in ((8, 2, SIZES[1]), (16, 4, SIZES[3]), (4, 2, SIZES[2]))]
FLOW_UP_CASES.append(_case("flow_up", "s8-tp2-prev-b32-64x64", Hp=64, Wp=64, s=8, tp=2, has_prev=1, B=32, flow="mixed", tkind="noise"))

FEAT_UP_CASES = [_case("feat_up", f"s{s}-{hp}x{wp}", Hp=hp, Wp=wp, s=s, B=1 + k % 2, tkind="pos" if k % 2 else "noise")
                 for k, (s, (hp, wp)) in enumerate(((1, SIZES[0]), (2, SIZES[1]), (4, SIZES[2]), (8, SIZES[3]), (16, SIZES[1]), (16, SIZES[0])))]


def _trans_cases(op, scales, nfs):
    out, i = [], 0
    for sn in scales:
        for quad in ((0, 14) if sn > 1 else (14,)):
            for hp_ in (1, 0):
                for NF in nfs:
                    (hp, wp), i = _sz(i), i + 1
                    out.append(_case(op, f"s{sn}-q{quad}-prev{hp_}-nf{NF}-{hp}x{wp}", Hp=hp, Wp=wp, s_next=sn, NF=NF, has_prev=hp_, quad=quad, xcd=0, flow="mixed",
                                     kind="pos" if i % 2 else "noise", tkind="pos" if i % 2 else "noise", tasks="b3" if hp * wp <= 64 * 192 and sn >= 2 else "b1",
                                     gap=8 if i % 3 == 0 else 0))
            # the partial tiles of 128x320 (Ws = 320 / sn cells: 16-cell tiles end inside the row for sn >= 4) for every kernel of this scale
            out.append(_case(op, f"s{sn}-q{quad}-prev1-nf{nfs[0]}-rand-pos-128x320", Hp=128, Wp=320, s_next=sn, NF=nfs[0], has_prev=1, quad=quad, xcd=0, flow="rand",
                             kind="pos", tkind="pos"))
        if sn > 1:   # the banded workgroup order; tile counts of the quad kernels here: 64x192 -> 12 (sn 4), 4 (sn 8); 64x64 -> 4, 2;
            # 128x320 -> 40, 12: no multiples of 8 (at sn 2 every size gives one)
            for (hp, wp), hp_ in ((SIZES[1], 1), (SIZES[0], 0), (SIZES[3], 1)):
                out.append(_case(op, f"s{sn}-q14-xcd-prev{hp_}-nf{nfs[-1]}-{hp}x{wp}", Hp=hp, Wp=wp, s_next=sn, NF=nfs[-1], has_prev=hp_, quad=14, xcd=1, flow="mixed",
                                 tkind="noise", tasks="b3" if hp == 64 else "b1", gap=8))
    out.append(_case(op, f"s{scales[1]}-q14-prev1-nf{nfs[0]}-b32-64x64", Hp=64, Wp=64, s_next=scales[1], NF=nfs[0], has_prev=1, quad=14, xcd=0, flow="mixed",
                     tkind="noise", tasks="b32", gap=8))
    return out


STAGE_TRANS_CASES = _trans_cases("stage_trans", (4, 2, 1), (1, 2))
STAGE_TRANS_X_CASES = _trans_cases("stage_trans_x", (8, 4, 2, 1), (1,))

TRANS1_CASES = [_case("trans1_conv0a", f"fuse{fu}-{tk}-{hp}x{wp}", Hp=hp, Wp=wp, fuse0a=fu, slope=0.2, flow="a0", kind="pos", tkind="pos", tasks=tk, gap=gap)
                for fu, tk, (hp, wp), gap in ((1, "b1p", SIZES[0], 0), (1, "b3p", SIZES[1], 8), (1, "b1p", SIZES[2], 8), (1, "b1p", SIZES[3], 0),
                                              (2, "b1p", SIZES[0], 8), (2, "b3p", SIZES[2], 0), (2, "b1p", SIZES[3], 0))]
TRANS1_CASES += [   # the flow families at the fused kernel's F: noise inputs, no summand condition.  Every A0 element next to a 1e4 or 1e30
    # flow channel is bounded by that channel's size only: with all families (`swamped`) the case is about Fout, and only the wrong
    # restatements that move Fout apply to it; without those four families every one applies
    _case("trans1_conv0a", "fuse1-mixed8-b3-64x192", Hp=64, Wp=192, fuse0a=1, slope=0.2, flow="mixed8", tkind="noise", tasks="b3", gap=8),
    _case("trans1_conv0a", "fuse2-mixed-b1-128x320", Hp=128, Wp=320, fuse0a=2, slope=0.2, flow="mixed", tkind="noise", swamped=True),
    _case("trans1_conv0a", "fuse1-rand-b32-64x64", Hp=64, Wp=64, fuse0a=1, slope=0.2, flow="rand", tkind="noise", tasks="b32", gap=8),
    # 32 x 6 x 4 = 768 tiles: more than the two workgroups per CU the persistent launch starts, so workgroups walk on to a second tile
    _case("trans1_conv0a", "fuse1-rand-b32-64x192-persistent", Hp=64, Wp=192, fuse0a=1, slope=0.2, flow="rand", tkind="noise", tasks="b32"),
]

FINAL_BLEND_CASES = [
    _case("final_blend", f"{h}x{w}-in-{hp}x{wp}-s{s}-tp{tp}-fdbg{fd}-xcd{xcd}-{fl}", H=h, W=w, Hp=hp, Wp=wp, s=s, tp=tp, fdbg=fd, xcd=xcd, flow=fl, kind=kd, tkind=kd, tasks=tk, gap=gap)
    for h, w, hp, wp, s, tp, fd, xcd, fl, kd, tk, gap in (
        (64, 64, 64, 64, 1, 2, 1, 0, "mixed", "noise", "b1", 0), (1, 1, 64, 64, 1, 2, 1, 0, "mixed", "noise", "b3", 8), (70, 90, 128, 128, 1, 2, 1, 0, "mixed", "noise", "b3", 8),
        (70, 90, 128, 128, 1, 2, 1, 1, "mixed", "noise", "b1", 0), (1, 1, 64, 64, 2, 4, 1, 1, "mixed", "pos", "b1", 0), (64, 192, 64, 192, 2, 2, 1, 0, "mixed", "pos", "b1", 0),
        (192, 64, 192, 64, 1, 4, 0, 0, "mixed", "noise", "b1", 8), (128, 320, 128, 320, 1, 2, 0, 1, "rand", "pos", "b1", 0), (70, 90, 128, 128, 2, 2, 0, 0, "mixed", "noise", "b3", 0),
        (100, 300, 128, 320, 4, 4, 1, 1, "mixed", "pos", "b1", 8), (64, 64, 64, 64, 1, 2, 1, 0, "rand", "pos", "b32", 8))]

PLANAR4_UP_CASES = [_case("planar4_up", f"u{u}-cx{cx}-fp{fp}-{hp}x{wp}", Hp=hp, Wp=wp, u=u, CX=cx, flow_plane=fp, B=b, kind=kd)
                    for u, cx, fp, (hp, wp), b, kd in ((2, 24, 4, SIZES[1], 2, "pos"), (4, 24, 4, SIZES[0], 1, "noise"), (2, 32, 7, SIZES[2], 1, "noise"), (4, 16, -1, SIZES[0], 2, "pos"),
                                                       (2, 32, 6, SIZES[3], 1, "noise"))]
T_DOWN_CASES = [_case("t_down", f"u{u}-tp{tp}-{hp}x{wp}", Hp=hp, Wp=wp, u=u, tp=tp, B=b, kind=kd)
                for u, tp, (hp, wp), b, kd in ((2, 2, SIZES[1], 2, "pos"), (4, 2, SIZES[0], 1, "noise"), (2, 4, SIZES[3], 1, "noise"), (4, 4, SIZES[2], 2, "pos"))]

TABLES = {"stage_in": STAGE_IN_CASES, "stage_in0_staged": STAGED_CASES, "flow_up": FLOW_UP_CASES, "feat_up": FEAT_UP_CASES, "stage_trans": STAGE_TRANS_CASES,
          "stage_trans_x": STAGE_TRANS_X_CASES, "trans1_conv0a": TRANS1_CASES, "final_blend": FINAL_BLEND_CASES, "planar4_up": PLANAR4_UP_CASES, "t_down": T_DOWN_CASES}
ALL_CASES = [c for t in TABLES.values() for c in t]


def applies(mut, case):
    """whether the wrong restatement `mut` differs from the right one for this case's op and parameters"""
    p, op = case.p, case.op
    trans = op in ("stage_trans", "stage_trans_x")
    s_x = p.get("s_next") if trans else (p.get("s") if op == "stage_in" else None)          # the scale X is down-resized by
    s_up = {"flow_up": p.get("s"), "feat_up": p.get("s"), "final_blend": p.get("s"), "trans1_conv0a": 2, "planar4_up": p.get("u")}.get(op, 2 * p["s_next"] if trans else None)
    warps = trans or op in ("trans1_conv0a", "final_blend") or (op == "stage_in" and p["has_flow"])
    if p.get("swamped") and mut not in ("no_times_s", "align_corners"):
        return False
    return {
        "centre": s_x is not None and s_x > 1,
        "mask_plane0": trans or op in ("flow_up", "trans1_conv0a", "final_blend"),
        "flow_not_div": s_x is not None and s_x > 1 and warps,
        "no_times_s": op != "feat_up" and op != "planar4_up" and s_up is not None and s_up > 1,
        "img1_F01": warps,
        "swap_feat": trans or op in ("stage_in", "stage_in0_staged", "trans1_conv0a"),
        "align_corners": s_up is not None and s_up > 1 and not (op == "final_blend" and p["H"] * p["W"] == 1),      # the corner pixel: source index 0 either way
        "drop_t": trans or op in ("stage_in", "stage_in0_staged", "trans1_conv0a"),
        "zero_tap": op == "trans1_conv0a",
        "blend_swapped": op == "final_blend",
    }[mut]


NEGATIVE = [(m, c) for m in MUTATIONS for c in ALL_CASES if applies(m, c)]
