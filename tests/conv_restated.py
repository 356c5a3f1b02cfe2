"""Float64 restatement of ONE layer-object call (vfi_conv_create / _create_ex / _create_up2x2 + vfi_conv_forward / _forward_ex,
csrc/gen_ops.hip) and a data generator for which every fp32 summation order gives the same result.

Why exact data.  The layer objects reach ~60 kernel instantiations (tile variants x EXT, split-K + reduce kernel, Winograd region shapes
x epilogue MODE).  They differ in summation order, so a tolerance sized for the longest reduction hides a dropped term in a short one.
Here the inputs are chosen so that the fp32 pre-activation has NO rounding in any order, and the tolerance for it is zero:

  x         odd integers in [-X, X]
  weights   +-u * 2^-s, never zero (u = 1; u = 4 for layers that can take the Winograd kernel: G g G^T then has entries
            u * {1, 1/2, 1/4} * (sum of <= 9 signs) — integers in units of 2^-s)
  bias, residual   integers in [-15, 15] times 2^-s
  s         a power-of-two scale of the whole layer, chosen so that the pre-activation is O(1): clamp01 (act 2) sees values inside,
            below and above [0, 1], sigmoid / GELU see their curved range
  slopes, post scale   signed powers of two (products exact), including slopes outside [0, 1] (2, -0.5: they leave the kernels'
            fmaxf(v, v * slope) fast path);  post shift: an integer

Every term of the reduction is an ODD multiple of u * 2^-s: one term dropped, duplicated or read from the wrong pixel / channel changes
the sum's parity, so it always changes the result.  Every partial sum, in any order, is an integer multiple of 2^-s whose size is at most
the sum of absolute values; if that stays below 2^24 units it is representable in fp32 and no addition (or fma) rounds.  X is the largest
2^k - 1 (k <= 15) for which an a-priori bound on that sum holds, so short reductions carry 12 - 15 significant bits (a path that lost
mantissa bits cannot pass) and long ones small integers.  The CERTIFICATE — computed from the drawn data, asserted by `make` — is

  direct forms     max over outputs of  conv(|x|, |w|) + |b| + |res|  <  2^24                        (units of 2^-s)
  Winograd forms   max over outputs of  |A^T| [ sum_c (|G| |g| |G^T|) (.) (|B^T| |d| |B|) ] |A|  + |b| + |res|  <  2^24,
                   every entry of G g G^T an integer — the kernel's input transform B^T d B (sums of 4 inputs), its products with
                   U = G g G^T, their sum over channels and the output transform A^T M A are then all exact, in any association.

Host-side folds of the library stay exact with these weights: the transposed convolution as a 3x3 layer (pack_deconv_as_conv3x3) and
the 2x2 layer embedded in 3x3 only COPY weights next to zeros; vfi_conv_create_up2x2 SUMS up to four weights +-2^-s per tap in fp32 —
integers in [-4, 4] units, exact (a sum may cancel to zero: that tap then carries no term, the others stay odd multiples or become even
ones — the restatement here works on the unfolded layer, so a wrong fold still shows); pack_wino3x3 computes G g G^T in double and casts
integers of at most 9 u units.

The epilogue on top of the exact pre-activation v = conv + b (+ res):
  act 0 none, 1 LeakyReLU(slope), 2 clamp01, 3 per-channel PReLU: exact (comparison, or a product with a power of two).
  post affine y * ps + sh: ps a power of two, sh an integer — the exact real value may need more than 24 bits; the kernels compute it as
      one fma or an exact product and one addition, i.e. ONE rounding of the exact value, which is what the cast of the float64 result
      to fp32 is.  Bit-equality holds for act 0 - 3 with and without it.
  act 4 sigmoid 1 / (1 + expf(-v)): expf, the addition and the division within 8 ulp together — tol = 8 U y, the figure of the
      FLAVR gate (tests/test_gpu_flavr.py) for the same expression.
  act 5 GELU 0.5 v (1 + erff(v * 0.70710678...)): the argument's rounding (of the constant and the product, <= 1.5 U relative) moves erf
      by at most x erf'(x) * 1.5 U <= 0.49 * 1.5 U < 1 U (x erf'(x) = 2 x exp(-x^2) / sqrt(pi) peaks at 0.484 for x = 0.707); erff
      itself E_erf U (|erf| <= 1); the addition one rounding of a value <= 2; so the bracket is off by at most (E_erf + 3) U
      absolute, times 0.5 |v|; the two products round once each, relative to y:
          tol = 0.5 |v| (E_erf + 3) U + 2 U |y|.
      E_erf: the ROCm installation this was written against ships no math-function accuracy table (its share/ and documentation
      trees do not mention erff), so E_erf = 4 ulp, the figure OpenCL's full profile and CUDA's table give erff.  It is not
      fitted to the kernels; tests/test_gpu_conv_exact.py prints max err / tol of every GELU case.
  With a post affine the tolerance is scaled by |ps| and one rounding of the result is added.
"""
import math
from dataclasses import dataclass, field, replace
from typing import Optional

import torch
import torch.nn.functional as F

U = 2.0 ** -24           # unit roundoff of fp32
E_ERF = 4.0              # ulp of erff (docstring)
LIMIT = 2.0 ** 24        # certificate bound, units of 2^-s
BIAS_MAX = 15
FILL = 12345.0           # what unmapped positions of a Cin_phys window hold: finite, the interface allows it; zero weights must meet it


@dataclass(frozen=True)
class Case:
    """One layer call.  api 'ex': vfi_conv_create_ex + vfi_conv_forward_ex; 'plain': vfi_conv_create + vfi_conv_forward (FILM's 'same'
    layers, k in 1, 2, 3); 'up2': vfi_conv_create_up2x2 + vfi_conv_forward.  kind 1 = ConvTranspose2d(4, 2, 1)."""
    api: str = "ex"
    kind: int = 0
    k: int = 3
    stride: int = 1
    pad: int = 0            # 0 zero, 1 replicate, 2 reflect
    cin: int = 8
    cphys: int = 8          # Cin_phys (multiple of 8)
    cout: int = 32
    n: int = 1
    h: int = 8
    w: int = 8
    act: int = 0
    slope: float = 0.0      # act 1
    res: bool = False
    post: Optional[tuple] = None   # (scale, shift)
    cmap: bool = False      # scatter the logical channels over the Cin_phys window
    odd: bool = False       # vfi_conv_accept_odd
    wino: bool = False      # draw Winograd-exact data (u = 4) and certify the Winograd form too

    @property
    def taps(self):
        return 4 if self.kind == 1 or self.api == "up2" else self.k * self.k

    @property
    def out_hw(self):
        if self.kind == 1 or self.api == "up2":
            return 2 * self.h, 2 * self.w
        return -(-self.h // self.stride), -(-self.w // self.stride)


@dataclass
class Data:
    x: torch.Tensor                 # [N, H, W, Cin] float64, logical channels
    w: torch.Tensor                 # OIHW [Cout, Cin, k, k]; kind 1: IOHW [Cin, Cout, 4, 4]
    b: torch.Tensor                 # [Cout]
    prelu: torch.Tensor             # [Cout] per-channel slopes (used by act 3)
    res: Optional[torch.Tensor]     # [N, Ho, Wo, Cout]
    cmap: Optional[list]
    s: int
    X: int
    u: int
    cert: dict = field(default_factory=dict)


# ---- padding and the tap sums, written out (no F.conv2d here: tests/test_conv_restated_cpu.py compares the two) -----------------------
def pad_index(i, n, mode):
    """csrc/vfi_common.h: pad_index."""
    if mode == 2:
        i = -i if i < 0 else (2 * n - 2 - i if i >= n else i)
    return min(max(i, 0), n - 1)


def _pad(x, top, bottom, left, right, mode):
    """x [N, H, W, C] -> [N, top + H + bottom, left + W + right, C]; mode 0 zeros, 1 replicate, 2 reflect."""
    N, H, W, C = x.shape
    if mode == 0:
        out = x.new_zeros(N, top + H + bottom, left + W + right, C)
        out[:, top:top + H, left:left + W] = x
        return out
    rows = torch.tensor([pad_index(i, H, mode) for i in range(-top, H + bottom)])
    cols = torch.tensor([pad_index(i, W, mode) for i in range(-left, W + right)])
    return x[:, rows][:, :, cols]


def _taps_conv(xp, w, stride, Ho, Wo, y0=0):
    """out[n, oy, ox, o] = sum_{dy, dx, c} xp[n, stride oy + dy + y0, stride ox + dx, c] w[o, c, dy, dx]"""
    k = w.shape[-1]
    out = xp.new_zeros(xp.shape[0], Ho, Wo, w.shape[0])
    for dy in range(k):
        for dx in range(k):
            win = xp[:, y0 + dy:y0 + dy + stride * (Ho - 1) + 1:stride, dx:dx + stride * (Wo - 1) + 1:stride]
            out += torch.einsum("nhwc,oc->nhwo", win, w[:, :, dy, dx])
    return out


def preact(case, x, w, b, shift=0):
    """conv + bias in float64, NHWC.  shift = 1: the negative control "padding moved by one pixel" (every tap reads one row lower)."""
    Ho, Wo = case.out_hw
    if case.api == "up2":       # F.interpolate(scale 2, nearest) then Conv2d(2, 'same'): 'same' for k = 2 pads bottom / right
        up = x[:, torch.arange(2 * case.h) // 2][:, :, torch.arange(2 * case.w) // 2]
        v = _taps_conv(_pad(up, 0, 1 + shift, 0, 1, 0), w, 1, Ho, Wo, shift)
    elif case.kind == 1:
        # out[2y + py, 2x + px, o] = sum_{a, b, c} in[y + py - 1 + a, x + px - 1 + b, c] w[c, o, 3 - py - 2a, 3 - px - 2b]
        xp = _pad(x, 1, 1 + shift, 1, 1, case.pad)
        v = x.new_zeros(case.n, Ho, Wo, case.cout)
        for py in range(2):
            for px in range(2):
                for a in range(2):
                    for bb in range(2):
                        win = xp[:, py + a + shift:py + a + shift + case.h, px + bb:px + bb + case.w]
                        v[:, py::2, px::2] += torch.einsum("nhwc,co->nhwo", win, w[:, :, 3 - py - 2 * a, 3 - px - 2 * bb])
    else:
        k, st = case.k, case.stride
        if k == 3:
            lo, hi_y, hi_x = 1, st * (Ho - 1) + 2 - case.h, st * (Wo - 1) + 2 - case.w      # 1 for stride 1 and even sizes; odd sizes too
            xp = _pad(x, lo, max(hi_y, 0) + shift, lo, max(hi_x, 0), case.pad)
        elif k == 2 and st == 1:
            xp = _pad(x, 0, 1 + shift, 0, 1, 0)
        else:
            xp = _pad(x, 0, shift, 0, 0, 0)
        v = _taps_conv(xp, w, st, Ho, Wo, shift)
    return v + b


def epilogue(case, v, prelu):
    """act + post affine on v (which already holds the residual), float64."""
    if case.act == 0:
        y = v
    elif case.act == 1:
        y = torch.where(v > 0, v, v * case.slope)
    elif case.act == 2:
        y = v.clamp(0.0, 1.0)
    elif case.act == 3:
        y = torch.where(v > 0, v, v * prelu)
    elif case.act == 4:
        y = 1.0 / (1.0 + torch.exp(-v))
    else:
        y = 0.5 * v * (1.0 + torch.erf(v * math.sqrt(0.5)))
    if case.post is not None:
        y = y * case.post[0] + case.post[1]
    return y


def restate(case, d, shift=0):
    """-> (v, y): the exact pre-activation (residual included) and the layer's output, float64 [N, Ho, Wo, Cout]."""
    v = preact(case, d.x, d.w, d.b, shift)
    if d.res is not None:
        v = v + d.res
    return v, epilogue(case, v, d.prelu)


def tolerance(case, v, y):
    """Per-element bound on |fp32 kernel - float64| (docstring); zero for act 0 - 3."""
    if case.act < 4:
        return torch.zeros_like(y)
    ps = abs(case.post[0]) if case.post is not None else 1.0
    ya = (y - (case.post[1] if case.post is not None else 0.0)) / (case.post[0] if case.post is not None else 1.0)
    if case.act == 4:
        tol = 8 * U * ya.abs()
    else:
        tol = 0.5 * v.abs() * (E_ERF + 3) * U + 2 * U * ya.abs()
    tol = tol * ps
    if case.post is not None:
        tol = tol + U * y.abs()
    return tol


# ---- the host-side folds, restated for the Winograd certificate -----------------------------------------------------------------------
def deconv_as_conv3x3(w_iohw):
    """pack_deconv_as_conv3x3: ConvTranspose2d(4, 2, 1) as a 3x3 layer with channel g * Cout + co, g = 2 py + px.  Copies only."""
    cin, lo = w_iohw.shape[:2]
    w3 = w_iohw.new_zeros(4 * lo, cin, 3, 3)
    for g in range(4):
        py, px = g >> 1, g & 1
        for a in range(2):
            for b in range(2):
                w3[g * lo:(g + 1) * lo, :, py + a, px + b] = w_iohw[:, :, 3 - py - 2 * a, 3 - px - 2 * b].t()
    return w3


def embed2x2(w):
    """vfi_conv_create: the 2x2 'same' layer inside a 3x3 one, w3[1 + dy][1 + dx] = w[dy][dx]."""
    w3 = w.new_zeros(w.shape[0], w.shape[1], 3, 3)
    w3[:, :, 1:, 1:] = w
    return w3


_G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float64)
_BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
_AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


def wino_certificate(x, w3, pad, extra):
    """x [N, H, W, C], w3 [O, C, 3, 3], both in units of 2^-s.  -> (max of the absolute-value Winograd sum + extra, G g G^T integral?)"""
    N, H, W, C = x.shape
    Ug = torch.einsum("ik,ockl,jl->ocij", _G, w3, _G)
    integral = bool((Ug == Ug.round()).all())
    Ua = torch.einsum("ik,ockl,jl->ocij", _G.abs(), w3.abs(), _G.abs())
    ty, tx = -(-H // 2), -(-W // 2)
    xp = _pad(x.abs(), 1, 1, 1, 1, pad)
    xp = _pad(xp, 0, 2 * ty + 2 - xp.shape[1], 0, 2 * tx + 2 - xp.shape[2], 0)
    tiles = xp.unfold(1, 4, 2).unfold(2, 4, 2)                     # [N, ty, tx, C, 4, 4]
    V = torch.einsum("ik,ntxckl,jl->ntxcij", _BT.abs(), tiles, _BT.abs())
    worst = 0.0
    for o0 in range(0, w3.shape[0], 32):                           # by 32 output channels: bounds the temporary
        M = torch.einsum("ntxcij,ocij->ntxoij", V, Ua[o0:o0 + 32])
        Y = torch.einsum("pi,ntxoij,qj->ntxopq", _AT.abs(), M, _AT.abs())
        worst = max(worst, float(Y.max()))
    return worst + extra, integral


# ---- the data generator ----------------------------------------------------------------------------------------------------------------
def _pow2_slopes(g, n):
    vals = torch.tensor([0.25, 0.5, 2.0, -0.5, 0.125, 1.0, -2.0, 0.0625], dtype=torch.float64)
    return vals[torch.randint(0, len(vals), (n,), generator=g)]


def make(case, seed=0):
    """Draws the data of `case`, asserts its exactness certificate(s) and returns it."""
    # two streams: the LAYER (weights, bias, slopes, channel map, X, s) depends on the layer's own fields only, so calls of one layer at
    # several sizes / epilogues share one handle; the call's data (x, residual) on its size too
    gl = torch.Generator().manual_seed(seed * 7919 + case.cin * 131 + case.cout * 17 + case.k + 1000 * case.kind + 5 * case.pad)
    g = torch.Generator().manual_seed(seed * 104729 + case.cin + 3 * case.h + 7 * case.w + 11 * case.n + 13 * case.act)
    u = 4 if case.wino else 1
    # a-priori bound per input channel on sum |w| |x| / X (units): direct taps * u; Winograd u * 4 * (1 + 1.5 + 1.5)^2 = 64 u
    # (row sums of |B^T| are 2 -> |B^T||d||B| <= 4 X; of |G| 1, 1.5, 1.5, 1; an output sums rows {0, 1, 2} or {1, 2, 3} of both sides)
    per_c = max(case.taps * u, 64 * u if case.wino else 0)
    extra = 2 * BIAS_MAX          # bias + residual (whether or not this call has one: X belongs to the layer)
    kbits = 15
    while kbits > 1 and case.cin * per_c * (2 ** kbits - 1) + extra >= LIMIT:
        kbits -= 1
    X = 2 ** kbits - 1
    assert case.cin * per_c * X + extra < LIMIT, "reduction too long for exact data"
    s = max(0, round(math.log2(math.sqrt(case.taps * case.cin) * X * u)))      # pre-activation O(1)
    sc = 2.0 ** -s
    Ho, Wo = case.out_hw
    mag = 2 * torch.randint(0, (X + 1) // 2, (case.n, case.h, case.w, case.cin), generator=g) + 1
    sgn = 2 * torch.randint(0, 2, mag.shape, generator=g) - 1
    x = (mag * sgn).double()
    wshape = (case.cin, case.cout, 4, 4) if case.kind == 1 else (case.cout, case.cin, case.k, case.k)
    w = (2 * torch.randint(0, 2, wshape, generator=gl) - 1).double() * u * sc
    b = torch.randint(-BIAS_MAX, BIAS_MAX + 1, (case.cout,), generator=gl).double() * sc
    res = torch.randint(-BIAS_MAX, BIAS_MAX + 1, (case.n, Ho, Wo, case.cout), generator=g).double() * sc if case.res else None
    prelu = _pow2_slopes(gl, case.cout)
    cmap = None
    if case.cmap:
        cmap = sorted(torch.randperm(case.cphys, generator=gl)[:case.cin].tolist())
        cmap = cmap[1:] + cmap[:1]          # not monotone: a pack that ignored the map's order shows
    d = Data(x, w, b, prelu, res, cmap, s, X, u)
    # certificate, in units of 2^-s
    ab = preact(case, x.abs(), w.abs() / sc, b.abs() / sc)
    if res is not None:
        ab = ab + res.abs() / sc
    d.cert["direct"] = float(ab.max())
    assert d.cert["direct"] < LIMIT, ("direct certificate", case, d.cert)
    if case.wino:
        w3 = deconv_as_conv3x3(w / sc) if case.kind == 1 else (embed2x2(w / sc) if case.k == 2 else w / sc)
        worst, integral = wino_certificate(x, w3, case.pad, extra)
        d.cert["wino"] = worst
        assert integral, ("G g G^T not integral", case)
        assert worst < LIMIT, ("Winograd certificate", case, d.cert)
    return d


def window(case, d):
    """The Cin_phys-channel input window [N, H, W, Cin_phys] fp32: mapped channels hold x, every other position FILL."""
    xin = torch.full((case.n, case.h, case.w, case.cphys), FILL, dtype=torch.float32)
    idx = torch.tensor(d.cmap if d.cmap is not None else list(range(case.cin)))
    xin[..., idx] = d.x.float()
    return xin


# ---- the same layer through torch's own operators (the CPU suite compares; a second statement of the geometry) -----------------------
def torch_preact(case, d):
    xc = d.x.permute(0, 3, 1, 2)
    mode = {1: "replicate", 2: "reflect"}.get(case.pad)
    if case.api == "up2":
        v = F.conv2d(F.pad(F.interpolate(xc, scale_factor=2, mode="nearest"), (0, 1, 0, 1)), d.w, d.b)
    elif case.kind == 1:
        if mode is None:
            v = F.conv_transpose2d(xc, d.w, d.b, 2, 1)
        else:       # the padded border enters through a padded input; its own two output rows / columns are cropped
            v = F.conv_transpose2d(F.pad(xc, (1, 1, 1, 1), mode=mode), d.w, d.b, 2, 1)[:, :, 2:-2, 2:-2]
    elif case.k == 3:
        v = F.conv2d(F.pad(xc, (1, 1, 1, 1), mode=mode), d.w, d.b, case.stride) if mode else F.conv2d(xc, d.w, d.b, case.stride, 1)
    elif case.k == 2 and case.stride == 1:
        v = F.conv2d(F.pad(xc, (0, 1, 0, 1)), d.w, d.b)
    else:
        v = F.conv2d(xc, d.w, d.b, case.stride)
    return v.permute(0, 2, 3, 1)


def mutate(case, d, how):
    """Negative controls on the weights: 'sign' flips one weight; 'swap' exchanges two unequal weights of one output channel's
    reduction (two taps; in a 1x1 layer, whose reduction runs over channels only, two channels)."""
    w = d.w.clone()
    if how == "sign":
        w[0, 0, 0, 0] = -w[0, 0, 0, 0]
        return replace(d, w=w)
    rows = w.permute(1, 0, 2, 3) if case.kind == 1 else w          # [Cout, Cin, k, k] view
    for o in range(rows.shape[0]):
        row = rows[o].reshape(-1)
        j = (row != row[0]).nonzero()
        if len(j):
            j = int(j[0])
            c0, t0, c1, t1 = 0, 0, j // (rows.shape[2] * rows.shape[3]), j % (rows.shape[2] * rows.shape[3])
            kk = rows.shape[3]
            a, b = rows[o, c0, t0 // kk, t0 % kk].clone(), rows[o, c1, t1 // kk, t1 % kk].clone()
            rows[o, c0, t0 // kk, t0 % kk], rows[o, c1, t1 // kk, t1 % kk] = b, a
            return replace(d, w=w)
    raise AssertionError("no two unequal weights")
