"""Float64 restatements, error bounds, case tables and mutations for the M2M family: csrc/m2m_net.hip (vfi_m2m_normalize, vfi_warp_m2m,
vfi_pool_mean, vfi_m2m_cube_apply, vfi_m2m_photo, vfi_m2m_splat_inputs, vfi_m2m_combine), csrc/m2m_render.hip (vfi_m2m_warp_image4,
vfi_m2m_photo_tiles, vfi_m2m_render_fused, the staged 4-channel splat) and the summation splat of csrc/m2m_ops.hip
(vfi_softsplat_sum).  No product code is imported: every op is the mathematical function of the reference formula
(vfi_models/m2m/M2M_arch.py, cupy_ops/softsplat.py), evaluated in float64 on the fp32 inputs.  Buffers, comparison, Case, the flow
families and the bilinear sampler with its bound come from tests/small_ops_restated.py (U = 2^-24; E_EXP, SIGMOID_U as justified there).

tests/test_m2m_restated_cpu.py holds the restatements against oracle/ (fp32) within these bounds and checks every case's branch
conditions; tests/test_gpu_m2m_restated.py runs the tables on the device library.  Both use `build` / `check` below.

BACKWARP (backwarp(), M2M_arch.py:24-92: grid_sample bilinear, zeros, align_corners=True at grid + flow * 2 / (size - 1)).  In exact
arithmetic the sampling position is p = X + f on both axes, square or not.  m2m_taps reaches it through R_M2M = 8 fp32 roundings per
axis: step = 2 / (n - 1) (m2m_warp_consts), step * i and -1 + . (lin_m2m), scl = (float)(2 / (n - 1)) (m2m_warp_consts), f * scl, the
sum g, g + 1 and the product with (n - 1) / 2 (exact itself).  In pixels (h = (n - 1) / 2) these are at most U h three times, U |f|
twice, U (|p| + h), U |p| twice: U (4 h + 2 |f| + 3 |p|) <= 5 U (|p| + n - 1) since |f| <= |p| + n - 1; `sample` charges
R U (|p| + n - 1).  The value term is its 8 U sum|tap * weight| (1 - w twice, the weight product, four products, three additions:
tap_acc's order).  A non-finite coordinate drops every tap (all comparisons false): the result is 0, which the restatement gets by
moving such a flow to 1e30.

FORWARD SPLAT (softsplat_out, softsplat.py:140-192): out[q] = sum_src in[src] k(q - p_src), k(d) = max(0, 1 - |dx|) max(0, 1 - |dy|),
p = X + f in float64, non-finite p dropped (:157-158).  A contribution is continuous in p with slope at most |in| per axis, so a
position error d moves it by at most |in| (dx + dy), on whichever side of an integer p lies.  The kernels reach p through R roundings:
R = 1 for the generic splat (X + f), R = 2 for the render (tf * tm, then X + .): d = R U (|p| + |f|) per axis.  Per output pixel
    tol[q] = sum_{src: |q - p| < 1 + d per axis} |in| (dx + dy) + (n_q + c) U sum |in k|
with n_q the number of sources in that reach set and c = 4 the roundings of one contribution (x1 - p and p - x0, their product, the
product with in; the n_q - 1 additions are in n_q); the render's inputs carry two more (img * td, * e): c = 6.  Both sums are float64
scatters over the 4 x 4 pixels around floor(p); d < 0.5 is asserted for every source within 3 pixels of the image, the others
(+-1e4, +-1e30) contribute exactly zero on both sides.  `mn`: the smallest single contribution of weight >= 1/4 to a pixel (positive inputs,
pixels with at most 64 sources in reach: beyond that the bound of a sum exceeds one summand).

PHOTO (M2M_arch.py:945-1010, :559-561).  tf = flow + residual: one fp32 addition, compared BIT FOR BIT with numpy.float32 (NaN where
both are NaN).  E = exp(clip(alpha * max(1 - wei * mean_c |im - backwarp(partner, tf)|, 0.001)^2, -20, 20)), wei = sigmoid(r8) * 0.8 + 0.1:
    a_c = |im_c - w_c|      tol_a = tol_w (sampler) + U a_c                    (|.| is 1-Lipschitz)
    m = (a0 + a1 + a2) / 3  tol_m = sum tol_a / 3 + 3 U m                      (two additions, the division)
    wei                     tol_wei = (SIGMOID_U + 1) U 0.8 sig + U wei        (sigmoid, the product, the addition; 0.8f, 0.1f as fp32 values)
    x = wei m               tol_x = tol_wei m + wei tol_m + tol_wei tol_m + U x
    y = max(1 - x, 0.001f)  tol_y = tol_x + U |1 - x|                          (max is 1-Lipschitz; 0 where 1 - x + tol_y < 0.001: y IS the constant)
    s = y^2                 tol_s = 2 y tol_y + tol_y^2 + U s
    z = clip(alpha s)       tol_z = |alpha| tol_s + U |alpha s|                (clip is 1-Lipschitz; 0 where alpha s -+ tol_z is beyond +-20)
    E = exp(z)              tol_E = E (expm1(tol_z) + 2 E_EXP U)
The tile ranges and smax of vfi_m2m_photo_tiles are exact functions of the tf the device wrote (`tile_ranges`).

SPLAT INPUTS: (img * td) * e within (2 U + U^2) |y| (two roundings compound), td * e within U |y|, tf * tm exact against the rounded
float64 product.

COMBINE / RENDER (forwarp_mframe_mask :551-581, hole fill :1026-1031, de-normalisation :1033-1037).  Per branch acc += fwd + bwd,
norm += (fwd.w + c7) + (bwd.w + c7), c7 = float32(1e-7): every value passes at most 8 additions, so tol_acc = sum tol_s + 8 U sum |o_s|,
tol_norm = sum tol_s.w + 8 U norm.  v = acc / norm: (tol_acc + |v| tol_norm) / (norm - tol_norm) + U |v|.  hole = norm < float32(1e-5);
fill = t1 a + t b within 2 U (|t1 a| + |t b|), the sum one more; out = v sd + mean: two more.  A pixel whose float64 norm is within
tol_norm of the threshold may be classified either way and is left out: at most 1 % of a case's pixels, asserted from the restatement
alone.  vfi_m2m_combine alone runs on a crafted splat buffer: norm and the hole bit are then a FIXED fp32 expression (restated in
numpy.float32, no pixel left out), the rest keeps its counted bound with tol_s = 0.

CUBE / POOL / NORMALIZE.  cube_apply: 16 terms of two products, 16 additions, / 16 (exact), the product with s3: 19 U |s3| sum|term| / 16.
pool_mean: float64 accumulation (n 2^-53 mean|v|) and one conversion.  normalize (:915-931): m0, m1 one rounding each (float64 sums), their mean one;
v_k = E x^2 - m^2 in float64 from the float64 quotients (cancellation (2 n + 6) 2^-53 E x^2 + 2 |m| n 2^-53 mean|x|) and one rounding, (mean - m_k)^2 two, two additions, sqrtf (2 U), + c7:
tol_var = sum_k (dv_k + 2 U v_k + 5 U d_k^2) / 2 + 2 U var, tol_sd = tol_var / (2 sqrt(var - tol_var)) + 3 U sd (sqrt(tol_var) where var <= 4 tol_var),
tol_mean = 2 U |mean| + (dm0 + dm1) / 2 (the mean-1000 case has equal frame means: d_k = fp32(mean) - fp32(m_k) carries U |m| of each, a
genuine 1e-4 on d_k that would drown the cancellation the case is there to catch); out = (x - mean) / sd: (tol_mean + U |x - mean|) / sd + |y| tol_sd / (sd - tol_sd) + U |y|.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from small_ops_restated import E_EXP, FAMILIES, INF, NAN, SIGMOID_U, U, Buffers, Case, bilinear, compare, flow_field, local_spread, sample  # noqa: F401

R_M2M = 8
R_SPLAT, R_RENDER = 1, 2
C_SPLAT, C_RENDER = 4, 6
RT, RCAP, RK = 32, 1824, 6
C7 = float(np.float32(1e-7))
HOLE = float(np.float32(1e-5))
C08, C01, FLOOR = float(np.float32(0.8)), float(np.float32(0.1)), float(np.float32(0.001))
OPTION_DEFAULTS = {"splat_atomic": 0, "splat_spill_cap": -1}


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _img(g, kind, *shape):
    return 0.5 + 0.5 * torch.rand(*shape, generator=g) if kind == "pos" else torch.randn(*shape, generator=g)


def _finite_or_far(f):
    return torch.where(torch.isfinite(f), f, torch.full_like(f, 1e30))


def compare_bits(got, want, what):
    """fp32 tensors equal bit for bit, or NaN in both."""
    got, want = got.reshape(-1).contiguous(), want.reshape(-1).float().contiguous()
    same = (got.view(torch.int32) == want.view(torch.int32)) | (torch.isnan(got) & torch.isnan(want))
    if not bool(same.all()):
        i = int((~same).nonzero()[0])
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.numel()} elements differ from the exact result; first at {i}: got {got[i].item()!r} want {want[i].item()!r}")


def tile_ranges(tf, finite_only=True):
    """tf [8,H,W,2] (numpy fp32) -> ([8,tiles,4], [8]) as vfi_m2m_photo_tiles defines them: (fx_min, fx_max, fy_min, fy_max) over the
    finite pairs of every 32x32 tile (ceil tile counts), (3e38, -3e38, 3e38, -3e38) where none; max |tf| over the finite pairs."""
    _, H, W, _ = tf.shape
    ty, tx = -(-H // RT), -(-W // RT)
    out = np.empty((8, ty * tx, 4), np.float32)
    smax = np.zeros(8, np.float32)
    for s in range(8):
        for j in range(ty):
            for i in range(tx):
                blk = tf[s, RT * j:RT * j + RT, RT * i:RT * i + RT].reshape(-1, 2)
                ok = np.isfinite(blk).all(axis=1) if finite_only else np.ones(len(blk), bool)
                if ok.any():
                    b = blk[ok]
                    out[s, j * tx + i] = (b[:, 0].min(), b[:, 0].max(), b[:, 1].min(), b[:, 1].max())
                    smax[s] = max(smax[s], np.abs(b).max())
                else:
                    out[s, j * tx + i] = (3e38, -3e38, 3e38, -3e38)
    return out, smax


# ---------------------------------------------------------------------------------------------------------------- flow fields

def warp_flows(g, N, H, W):
    """'mixed' over all FAMILIES and +-1e30 (13 entries of flow_field's table), one NaN and one inf pixel."""
    f = flow_field(g, N, H, W, "mixed", len(FAMILIES) + 2)
    f[0, 0, W - 1, 0] = NAN
    f[N - 1, H - 1, 0, 1] = INF
    return f


def splat_field(g, N, H, W, kind, s=0):
    """[N,H,W,2] fp32, a different field per image (the 8 splats of a render are 8 images)."""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    f = torch.zeros(N, H, W, 2)
    for n in range(N):
        k = n + s
        if kind in ("mixed", "mixed8"):         # every family, +-1e30, NaN / +-inf pixels, and targets exactly on (and a quarter past) the tile edges 31, 32, 63, 64
            # (mixed8, for the render: the families up to 'just above size-1' — with a third of the sources gone per axis too many pixels would
            # sit at the hole threshold; the render's +-1e30 are the 'huge' field)
            if n == 0:
                base = flow_field(g, N, H, W, "mixed", len(FAMILIES) + 2 if kind == "mixed" else 8)      # image n: the families shifted by 3 n
            f[n] = base[n]
            for i, (y, x) in enumerate((y, x) for y in range(0, H, 3) for x in range((y // 3) % 4, W, 4)):
                T = (31.0, 32.0, 63.0, 64.0)[(i + k) % 4] + (0.0, 0.25)[(i // 4) % 2]
                ax = (i // 8) % 2
                f[n, y, x, ax] = T - (x, y)[ax]
            f[n, H - 1, W - 1, 0], f[n, 0, 1, 1], f[n, 1, 0, 0] = NAN, INF, -INF
        elif kind == "translate":
            f[n, ..., 0], f[n, ..., 1] = 2.25 * (k + 1), -1.75 * (k + 1)
        elif kind in ("noise1", "noise8"):
            f[n] = torch.randn(H, W, 2, generator=g) * (1.0 if kind == "noise1" else 8.0)
        elif kind == "smooth":
            f[n, ..., 0] = 3.0 * torch.sin(yy / 47.0 + k) + 2.5 * torch.cos(xx / 53.0) + (k - 3.5) * 1.7
            f[n, ..., 1] = 2.0 * torch.cos(yy / 43.0) - 3.0 * torch.sin(xx / 59.0 + 0.5 * k) - (k - 3.5) * 0.9
        elif kind == "wavy":
            f[n, ..., 0] = 5.0 * torch.sin(yy / 11.0 + k) + 4.5 * torch.cos(xx / 13.0) + (k - 3.5) * 1.7
            f[n, ..., 1] = 4.0 * torch.cos(yy / 9.0) - 5.0 * torch.sin(xx / 12.0 + 0.5 * k) - (k - 3.5) * 0.9
        elif kind in ("zoom", "zoom_r"):         # convergent: 1 / 0.22^2 = 20 sources per cell (_r: for the render at t = 0.5, whose flows are halved)
            m = 0.78 * (2 if kind == "zoom_r" else 1)
            f[n, ..., 0], f[n, ..., 1] = (W / 2 - xx) * m + 0.1 * k, (H / 2 - yy) * m - 0.1 * k
        elif kind in ("zoom8", "zoom8_r"):       # 1 / 0.35^2 = 8 sources per cell: more than RK, fewer than 16
            m = 0.65 * (2 if kind == "zoom8_r" else 1)
            f[n, ..., 0], f[n, ..., 1] = (W / 2 - xx) * m + 0.1 * k, (H / 2 - yy) * m - 0.1 * k
        elif kind in ("point", "point_r"):
            m = 2 if kind == "point_r" else 1
            f[n, ..., 0], f[n, ..., 1] = ((W / 3 + 0.37 * (k + 1)) - xx) * m, ((H / 2 + 0.21 * (k + 1)) - yy) * m
        elif kind == "far":          # beyond 64 px, up to 150 (as far as the image is wide), pointing INTO the image: right in its left half, left in
            top = min(150.0, W - 8.0)        # its right half; a few rows go the same way vertically where the image is high enough
            mag = 64.5 + ((xx * 7 + yy * 3 + 11 * k) % 32) * ((top - 64.5) / 31)
            f[n, ..., 0] = torch.where(xx < W / 2, mag, -mag)
            f[n, ..., 1] = 1.5 * torch.cos(xx / 7.0 + k)
            if H > 80:
                f[n, ::5, :, 1] = torch.where(yy < H / 2, 66.25, -70.5)[::5]
                f[n, ::5, :, 0] = (0.75 * torch.sin(yy / 3.0))[::5]
        elif kind == "near64":       # flows just under and just over the list path's 63 px cap, both signs
            f[n, ..., 0] = torch.where((xx + yy) % 2 == 0, 62.75, -63.25) + 0.5 * torch.sin(yy / 3.0 + k)
            f[n, ..., 1] = 0.3 * torch.cos(xx / 5.0)
        elif kind == "huge":
            f[n] = torch.where(torch.rand(H, W, 2, generator=g) < 0.5, 1e30, -1e30)
            f[n, ::2, ::2] = torch.randn(H, W, 2, generator=g)[::2, ::2]
        elif kind == "hole":         # every source of rows / columns 3..26 leaves for good: nothing lands in 5..24 at tm >= 0.25
            f[n, ..., 0], f[n, ..., 1] = 0.4 * torch.sin(yy / 7.0 + k), 0.4 * torch.cos(xx / 5.0 + k)
            f[n, 3:27, 3:27, :] = 4000.0
        else:
            raise ValueError(kind)
    return f


# ---------------------------------------------------------------------------------------------------------------- forward splat

def splat64(inp, flow, R, c, mut=None):
    """inp [N,H,W,C], flow [N,H,W,2] float64 (the exact flow) -> dict(want, tol [N,H,W,C], mn, cnt [N,H,W] sources per north-west cell,
    reach [N,H,W] n_q).  Module docstring, FORWARD SPLAT."""
    N, H, W, Cc = inp.shape
    X = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    Y = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    px, py = X + flow[..., 0], Y + flow[..., 1]
    live = torch.isfinite(px) & torch.isfinite(py)
    dx, dy = R * U * (px.abs() + flow[..., 0].abs()), R * U * (py.abs() + flow[..., 1].abs())
    near = live & (px > -3) & (px < W + 2) & (py > -3) & (py < H + 2)
    assert float(torch.where(near, dx + dy, torch.zeros_like(dx)).max()) < 0.5
    px, py, dx, dy = (torch.where(near, v, torch.zeros_like(v)) for v in (px, py, dx, dy))
    x0, y0 = px.floor(), py.floor()
    cell = torch.where(near & (x0 >= -1) & (x0 < W) & (y0 >= -1) & (y0 < H), (y0 + 1) * (W + 1) + x0 + 1, torch.full_like(x0, -1)).long()
    nb = torch.arange(N).view(N, 1, 1).expand(N, H, W)
    key = (nb * (H + 1) * (W + 1) + cell)[cell >= 0]
    counts = torch.bincount(key, minlength=N * (H + 1) * (W + 1)).view(N, H + 1, W + 1)
    if mut == "drop7th":           # the 7th source, in raster order, of every cell that holds more than 6
        flat = torch.where(cell >= 0, nb * (H + 1) * (W + 1) + cell, torch.full_like(cell, -1)).reshape(-1)
        order = torch.argsort(flat, stable=True)
        srt = flat[order]
        first = torch.searchsorted(srt, srt)
        rank = torch.empty_like(flat)
        rank[order] = torch.arange(flat.numel()) - first
        near = near & ~((rank == 6) & (flat >= 0)).view(N, H, W)
    if mut == "edge_column":       # sources whose north-west target lies on column X0 - 1 of a tile
        near = near & ~((x0 % RT) == RT - 1)
    ax, ay = px - x0, py - y0
    if mut == "swap_ne_sw":
        ax, ay = ay, ax
    want = torch.zeros(N * H * W, Cc, dtype=torch.float64)
    T1, T2 = torch.zeros_like(want), torch.zeros_like(want)
    nq = torch.zeros(N * H * W, dtype=torch.float64)
    mn = torch.full((N * H * W, Cc), INF, dtype=torch.float64)
    for oy in range(-1, 3):
        for ox in range(-1, 3):
            qx, qy = x0 + ox, y0 + oy
            ddx, ddy = (qx - x0 - ax).abs(), (qy - y0 - ay).abs()
            k = (1 - ddx).clamp_min(0) * (1 - ddy).clamp_min(0)
            ok = near & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            reach = ok & (ddx < 1 + dx) & (ddy < 1 + dy)
            idx = ((nb * H + qy.long().clamp(0, H - 1)) * W + qx.long().clamp(0, W - 1))
            i1 = idx[reach]
            a = inp[reach]
            kk = k[reach].unsqueeze(-1)
            want.index_add_(0, i1, a * kk)
            T2.index_add_(0, i1, (a * kk).abs())
            T1.index_add_(0, i1, a.abs() * (dx + dy)[reach].unsqueeze(-1))
            nq.index_add_(0, i1, torch.ones(i1.shape[0], dtype=torch.float64))
            big = reach & (k >= 0.25)
            mn.scatter_reduce_(0, idx[big].unsqueeze(-1).expand(-1, Cc), (inp[big] * k[big].unsqueeze(-1)).abs(), "amin")
    tol = T1 + (nq.unsqueeze(-1) + c) * U * T2
    mn = torch.where(nq.unsqueeze(-1) <= 64, mn, torch.full_like(mn, INF))
    sh = (N, H, W, Cc)
    return dict(want=want.view(sh), tol=tol.view(sh), mn=mn.view(sh), cnt=counts, reach=nq.view(N, H, W), cell=cell, absw=T2.view(sh))


def _add_dense(B, name, t, C, misalign=False, role="in", n=None):
    """a dense [pixels, C] tensor; misalign: as ONE row of a body that starts one float past a 16-byte boundary"""
    n = t.numel() if t is not None else n
    if misalign:
        B.add(name, t.reshape(1, n) if t is not None else None, 1, n, cs=n + 1, off=1, role=role)
    else:
        B.add(name, t.reshape(n // C, C) if t is not None else None, n // C, C, role=role)


def op_softsplat(P, B):
    """vfi_softsplat_sum: R = 1, c = 4."""
    g = _g(P.seed)
    mut = getattr(P, "mut", None)
    a = _img(g, "pos", P.N, P.H, P.W, P.C)
    f = splat_field(g, P.N, P.H, P.W, P.field)
    _add_dense(B, "in", a, P.C, P.mis)
    _add_dense(B, "flow", f, 2)
    _add_dense(B, "out", None, P.C, P.mis, role="out", n=a.numel())
    r = splat64(a.double(), f.double(), R_SPLAT, C_SPLAT, mut)
    e = dict(buf="out", want=r["want"], tol=r["tol"], mn=r["mn"] if mut is None else None)
    expects = [e]
    if P.field == "translate" and mut is None and not P.opts:          # the sequential oracle's order: bit for bit
        from oracle import m2m_oracle

        seq = m2m_oracle.softsplat_sum(a.permute(0, 3, 1, 2).contiguous().numpy(), f.permute(0, 3, 1, 2).contiguous().numpy())
        expects.append(dict(buf="out", bits=torch.from_numpy(seq).permute(0, 2, 3, 1).contiguous()))
    far = (f.abs().amax(-1) > 63) & torch.isfinite(f).all(-1)          # what splat_far_pass takes
    rf = splat64(a.double() * far.unsqueeze(-1), f.double(), R_SPLAT, C_SPLAT)
    info = dict(far_arrivals=int((rf["want"][..., 0] > r["tol"][..., 0]).sum()), cnt_max=int(r["cnt"].max()), fmax=float(_finite_or_far(f).abs().clamp(max=1e4).max()), reach_max=int(r["reach"].max()))
    return [("vfi_softsplat_sum", [B.ptr("in"), B.ptr("flow"), B.ptr("out"), P.N, P.H, P.W, P.C])], expects, dict(a=a, f=f), info


# ---------------------------------------------------------------------------------------------------------------- backwarp

def _backwarp64(img, fl, swap, mut=None):
    """img [N,H,W,C] fp32, fl [N,H,W,2] fp32 -> want, tol, big."""
    N, H, W, _ = img.shape
    src = img.double()
    if swap and mut != "noswap":
        src = src.view(N // 2, 2, *src.shape[1:]).flip(1).reshape(src.shape)
    f = _finite_or_far(fl.double())
    fy = f[..., 1] * ((H - 1) / (W - 1)) if mut == "sclx_both" else f[..., 1]
    return sample(src, f[..., 0], fy, mut == "border", R_M2M)


def op_warp_m2m(P, B):
    """vfi_warp_m2m: module docstring, BACKWARP."""
    g = _g(P.seed)
    mut = getattr(P, "mut", None)
    img = _img(g, P.kind, P.N, P.H, P.W, P.C)
    fl = warp_flows(g, P.N, P.H, P.W) if P.flow == "mixed" else torch.randn(P.N, P.H, P.W, 2, generator=g) * 1.5
    px = P.N * P.H * P.W
    B.add("in", img.reshape(px, P.C), cs=P.in_cs, off=P.in_off)
    B.add("flow", fl.reshape(px, 2), cs=P.flow_cs, off=P.flow_off)
    B.add("out", None, px, P.C, P.out_cs, P.out_off, role="out")
    want, tol, big = _backwarp64(img, fl, P.swap, mut)
    e = dict(buf="out", want=want, tol=tol, mn=big if P.kind == "pos" and mut is None else None)
    args = [B.ptr("in"), P.in_cs, P.swap, B.ptr("flow"), P.flow_cs, B.ptr("out"), P.out_cs, P.N, P.H, P.W, P.C]
    return [("vfi_warp_m2m", args)], [e], dict(img=img, fl=fl), {}


def op_warp_image4(P, B):
    """vfi_m2m_warp_image4 = vfi_warp_m2m(in_swap = 1, C = 3) from the compact plane (rgb, 1)."""
    g = _g(P.seed)
    mut = getattr(P, "mut", None)
    img = _img(g, P.kind, 2, P.H, P.W, 3)
    fl = warp_flows(g, 2, P.H, P.W)
    px = 2 * P.H * P.W
    B.add("img4", torch.cat([img, torch.ones(2, P.H, P.W, 1)], -1).reshape(px, 4))
    B.add("flow", fl.reshape(px, 2), cs=P.flow_cs, off=P.flow_off)
    B.add("out", None, px, 3, P.out_cs, P.out_off, role="out")
    want, tol, big = _backwarp64(img, fl, 1, mut)
    e = dict(buf="out", want=want, tol=tol, mn=big if P.kind == "pos" and mut is None else None)
    return [("vfi_m2m_warp_image4", [B.ptr("img4"), B.ptr("flow"), P.flow_cs, B.ptr("out"), P.out_cs, P.H, P.W])], [e], dict(img=img, fl=fl), {}


# ---------------------------------------------------------------------------------------------------------------- photo

def photo64(img, tf, logit, alpha, mut=None):
    """img [2,H,W,3] fp32, tf [8,H,W,2] fp32 (s = 2 b + d), logit [2,H,W] fp32, alpha the fp32 value -> E, tol [8,H,W]."""
    E, T, floored, floored_tight = [], [], 0, 0
    sig = torch.sigmoid(logit.double())
    wei = sig * C08 + (0.0 if mut == "wei_no_01" else C01)
    tol_wei = (SIGMOID_U + 1) * U * C08 * sig + U * wei
    for s in range(8):
        d = s & 1
        pair = torch.stack([tf[s], tf[s]])          # image slot d samples its partner; slot d ^ 1 is unused
        w, tw, _ = _backwarp64(img, pair, 1, mut)
        w, tw = w[d], tw[d]
        a = (img[d].double() - w).abs()
        ta = tw + U * a
        m = a.sum(-1) / 3
        tm_ = ta.sum(-1) / 3 + 3 * U * m
        x = wei[d] * m
        tx = tol_wei[d] * m + wei[d] * tm_ + tol_wei[d] * tm_ + U * x
        y = 1 - x
        ty = tx + U * y.abs()
        if mut != "no_floor":
            fl_ = y + ty < FLOOR          # below the floor whatever the error: the fp32 result is the constant itself
            y, ty = y.clamp_min(FLOOR), torch.where(fl_, torch.zeros_like(ty), ty)
        sq = y * y
        ts = 2 * y.abs() * ty + ty * ty + U * sq
        z = alpha * sq
        tz = abs(alpha) * ts + U * z.abs()
        if mut != "no_clip":
            tz = torch.where((z - tz > 20.0) | (z + tz < -20.0), torch.zeros_like(tz), tz)          # clipped whatever the error: exactly +-20
            z = z.clamp(-20.0, 20.0)
        e = torch.exp(z)
        te = e * (torch.expm1(tz) + 2 * E_EXP * U)
        E.append(e)
        T.append(te)
        if mut is None:
            floored += int(fl_.sum())
            floored_tight += int((fl_ & (te < 1e-4 * e)).sum())
    photo64.last = dict(floored=floored, floored_tight=floored_tight)
    return torch.stack(E), torch.stack(T)


def _photo_inputs(P):
    g = _g(P.seed)
    H, W = P.H, P.W
    d0 = torch.randn(2, H, W, P.d0_cs, generator=g)
    d0[..., 2:5] *= P.img_scale
    d0[..., 0:2] = warp_flows(g, 2, H, W) if P.flow == "mixed" else torch.randn(2, H, W, 2, generator=g) * 6.0
    r = torch.randn(2, H, W, P.r_C, generator=g)
    r[..., 0:8] *= 2.0
    r[..., 8] *= 3.0
    r[0, ::3, ::5, 8], r[1, 1::4, 2::3, 8] = 30.0, -30.0
    if P.flow == "mixed" and H >= 33:          # a whole tile (0, 0) of direction 0 without a finite flow
        d0[0, :32, :32, 0] = NAN
    return d0, r


def op_photo(P, B):
    """vfi_m2m_photo and, for P.tiles, vfi_m2m_photo_tiles on the same inputs (tf / E of both bit-identical, both against the
    restatement; ranges and smax exact functions of the device's tf)."""
    mut = getattr(P, "mut", None)
    H, W = P.H, P.W
    d0, r = _photo_inputs(P)
    hw = H * W
    B.add("d0", d0.reshape(2 * hw, P.d0_cs))
    B.add("r", r.reshape(2 * hw, P.r_C), cs=P.r_cs, off=P.r_off)
    B.add("tf", None, 8 * hw, 2, role="out")
    B.add("e", None, 8 * hw, 1, role="out")
    alpha = float(np.float32(P.alpha))
    d0n, rn = d0.numpy(), r.numpy()
    tf = np.stack([d0n[s & 1, :, :, 0:2] + rn[s & 1, :, :, 2 * (s >> 1):2 * (s >> 1) + 2] for s in range(8)]).astype(np.float32)
    tf = torch.from_numpy(tf)
    Ew, Et = photo64(d0[..., 2:5].contiguous(), tf, r[..., 8], alpha, mut)
    calls = [("vfi_m2m_photo", [B.ptr("d0"), P.d0_cs, B.ptr("r"), P.r_cs, C.c_float(P.alpha), B.ptr("tf"), B.ptr("e"), H, W])]
    expects = [dict(buf="tf", bits=tf), dict(buf="e", want=Ew, tol=Et)]
    if P.tiles:
        tiles = -(-H // RT) * -(-W // RT)
        B.add("img4", torch.cat([d0[..., 2:5], torch.ones(2, H, W, 1)], -1).reshape(2 * hw, 4))
        B.add("tf2", None, 8 * hw, 2, role="out")
        B.add("e2", None, 8 * hw, 1, role="out")
        B.add("ranges", None, 8 * tiles, 4, role="out")
        B.add("smax", None, 8, 1, role="out")
        calls.append(("vfi_m2m_photo_tiles", [B.ptr("d0"), P.d0_cs, B.ptr("r"), P.r_cs, C.c_float(P.alpha), B.ptr("img4"), B.ptr("tf2"), B.ptr("e2"),
                                              B.ptr("ranges"), B.ptr("smax"), H, W]))
        fin = mut != "ranges_all"
        expects += [dict(buf="tf2", bits=tf), dict(buf="e2", same_as="e"), dict(buf="e2", want=Ew, tol=Et),
                    dict(buf="ranges", bits_from=lambda o: torch.from_numpy(tile_ranges(o["tf2"].view(8, H, W, 2).numpy(), fin)[0])),
                    dict(buf="smax", bits_from=lambda o: torch.from_numpy(tile_ranges(o["tf2"].view(8, H, W, 2).numpy(), fin)[1]))]
    info = dict(clip=int((Ew == float(np.exp(20.0))).sum()), **(photo64.last if mut is None else {}))
    return calls, expects, dict(d0=d0, r=r, tf=tf), info


# ---------------------------------------------------------------------------------------------------------------- render

def _render_inputs(P):
    g = _g(P.seed)
    Hp, Wp = P.Hp, P.Wp
    d0 = torch.zeros(2, Hp, Wp, 8)
    d0[..., 2:5] = torch.randn(2, Hp, Wp, 3, generator=g)
    tf = splat_field(g, 8, Hp, Wp, P.field)
    e = torch.exp(torch.rand(8, Hp, Wp, generator=g) * (20.0 if P.e20 else 2.0) - (0.0 if P.e20 else 1.0))
    return d0, tf, e, torch.tensor([0.45, 0.27])


def _t_pair(t):
    t32 = np.float32(t)
    t1 = np.float32(1.0) - t32
    return float(t32), float(t1)


def render64(d0, tf, e, stats, t, H, W, mut=None, splats=None):
    """-> dict(want, tol, where [H,W,3], hole [H,W], per-splat results).  Module docstring, COMBINE / RENDER.  splats: fp32 [8,Hp,Wp,4]
    to combine instead of splatting (vfi_m2m_combine alone: norm and the hole bit are then the fixed fp32 expression)."""
    _, Hp, Wp, _ = d0.shape
    t32, t1 = _t_pair(t)
    img = d0[..., 2:5].double()
    res = []
    if splats is None:
        for s in range(8):
            d = s & 1
            td, tm = (t1, t32) if d == 0 else (t32, t1)
            if mut == "td_tm":
                td, tm = tm, td
            es = e[s].double().unsqueeze(-1)
            inp = torch.cat([img[d] * td * es, td * es], -1)
            res.append(splat64(inp[None], (tf[s].double() * tm)[None], R_RENDER, C_RENDER, mut if mut in ("drop7th", "edge_column", "swap_ne_sw") else None))
        o = torch.stack([r["want"][0] for r in res])
        to = torch.stack([r["tol"][0] for r in res])
    else:
        o, to = splats.double(), torch.zeros(8, Hp, Wp, 4, dtype=torch.float64)
    c7 = 0.0 if mut == "no_c7" else C7
    acc = o[..., :3].sum(0)
    tacc = to[..., :3].sum(0) + 8 * U * (o[..., :3].abs() + to[..., :3]).sum(0)
    norm = (o[..., 3] + c7).sum(0)
    tnorm = to[..., 3].sum(0) + 8 * U * norm.abs()
    if splats is None:
        hole = norm < HOLE
        sure = (norm - HOLE).abs() > tnorm
    else:
        w = splats[..., 3].numpy()
        n32 = np.zeros((Hp, Wp), np.float32)
        for b in range(4):
            n32 = n32 + ((w[2 * b] + np.float32(c7)) + (w[2 * b + 1] + np.float32(c7)))
        hole = torch.from_numpy(n32 <= np.float32(1e-5) if mut == "hole_le" else n32 < np.float32(1e-5))
        sure = torch.ones_like(hole)
    with np.errstate(all="ignore"):
        v = acc / norm.unsqueeze(-1)
        tv = (tacc + v.abs() * tnorm.unsqueeze(-1)) / (norm - tnorm).clamp_min(1e-300).unsqueeze(-1) + U * v.abs()
    fa, fb = t1 * img[0], t32 * img[1]
    fill = fa + fb
    tfill = 2 * U * (fa.abs() + fb.abs())
    if mut != "no_fill":
        hv = v + fill
        v = torch.where(hole.unsqueeze(-1), hv, v)
        tv = torch.where(hole.unsqueeze(-1), tv + tfill + U * hv.abs(), tv)
    sd, mean = float(stats[1]), float(stats[0])
    out = v * sd + mean
    tout = tv * abs(sd) + U * (v * sd).abs() + U * out.abs()
    where = sure.unsqueeze(-1).expand(-1, -1, 3)
    return dict(want=out[:H, :W], tol=tout[:H, :W], where=where[:H, :W], hole=hole[:H, :W], sure=sure[:H, :W], res=res)


def _render_info(r, tf, t, H, W):
    sure, hole = r["sure"], r["hole"]
    left_out = 1.0 - float(sure.double().mean())
    assert left_out <= 0.01, f"{left_out:.3%} of the pixels are within the bound of the hole threshold: choose other fields"
    info = dict(left_out=left_out, holes=int((hole & sure).sum()), solid=int((~hole & sure).sum()), cnt_max=0, cnt36=False, win_max=0)
    Hp, Wp = tf.shape[1:3]
    # render_window takes, per source block with a finite range, the block's pixels inside (tile - [f_min, f_max] tm): where every block's scaled
    # range spans more than the image both ways, every visible tile's window is the whole padded image
    rg, _ = tile_ranges(tf.numpy())
    t32, t1 = _t_pair(t)
    tmv = np.array([t32 if s % 2 == 0 else t1 for s in range(8)], np.float32).reshape(8, 1)
    info["ranges_span_image"] = bool(((rg[..., 0] * tmv <= -Wp) & (rg[..., 1] * tmv >= Wp) & (rg[..., 2] * tmv <= -Hp) & (rg[..., 3] * tmv >= Hp)).all()) and Hp * Wp > RCAP
    for s, rs in enumerate(r["res"]):
        cnt = rs["cnt"][0]
        info["cnt_max"] = max(info["cnt_max"], int(cnt.max()))
        info["cnt36"] = info["cnt36"] or bool(((cnt >= 3) & (cnt <= RK)).any())
        # the window of a visible tile holds at least the bounding box of the sources whose north-west target is one of its cells
        cell = rs["cell"][0]
        ok = cell >= 0
        cy, cx = torch.div(cell, Wp + 1, rounding_mode="floor") - 1, cell % (Wp + 1) - 1
        ys, xs = torch.meshgrid(torch.arange(Hp), torch.arange(Wp), indexing="ij")
        for ty in range(-(-H // RT)):
            for tx in range(-(-W // RT)):
                m = ok & (cy >= RT * ty - 1) & (cy < RT * ty + RT) & (cx >= RT * tx - 1) & (cx < RT * tx + RT)
                if m.any():
                    info["win_max"] = max(info["win_max"], int((ys[m].max() - ys[m].min() + 1) * (xs[m].max() - xs[m].min() + 1)))
    return info


def op_render(P, B):
    """forwarp_mframe_mask + hole fill + de-normalisation, as vfi_m2m_splat_inputs -> vfi_softsplat_sum (N = 8, C = 4) -> vfi_m2m_combine
    (P.form = 'three') or as vfi_m2m_render_fused (P.form = 'fused').  One restatement for both."""
    mut = getattr(P, "mut", None)
    d0, tf, e, stats = _render_inputs(P)
    Hp, Wp, H, W = P.Hp, P.Wp, P.H, P.W
    hw = Hp * Wp
    B.add("tf", tf.reshape(8 * hw, 2))
    B.add("e", e.reshape(8 * hw, 1))
    B.add("stats", stats.reshape(1, 2))
    B.add("out", None, H * W, 3, role="out")
    t = C.c_float(P.t)
    if P.form == "three":
        B.add("d0", d0.reshape(2 * hw, 8))
        for nm, c in (("sin", 4), ("sfl", 2), ("sout", 4)):
            B.add(nm, None, 8 * hw, c, role="scratch")
        calls = [("vfi_m2m_splat_inputs", [B.ptr("d0"), 8, B.ptr("tf"), B.ptr("e"), t, B.ptr("sin"), B.ptr("sfl"), Hp, Wp]),
                 ("vfi_softsplat_sum", [B.ptr("sin"), B.ptr("sfl"), B.ptr("sout"), 8, Hp, Wp, 4]),
                 ("vfi_m2m_combine", [B.ptr("sout"), B.ptr("d0"), 8, B.ptr("stats"), t, B.ptr("out"), Hp, Wp, H, W])]
    else:
        rg, sm = tile_ranges(tf.numpy())
        B.add("img4", torch.cat([d0[..., 2:5], torch.ones(2, Hp, Wp, 1)], -1).reshape(2 * hw, 4))
        B.add("ranges", torch.from_numpy(rg).reshape(-1, 4))
        B.add("smax", torch.from_numpy(sm).reshape(8, 1))
        calls = [("vfi_m2m_render_fused", [B.ptr("img4"), B.ptr("tf"), B.ptr("e"), B.ptr("ranges"), B.ptr("smax"), B.ptr("stats"), t, B.ptr("out"), Hp, Wp, H, W])]
    r = render64(d0, tf, e, stats, P.t, H, W, mut)
    info = _render_info(r, tf, P.t, H, W) if mut is None else {}
    return calls, [dict(buf="out", want=r["want"], tol=r["tol"], where=r["where"])], dict(d0=d0, tf=tf, e=e, stats=stats), info


def op_splat_inputs(P, B):
    """vfi_m2m_splat_inputs: in = ((img * td) * e, td * e) within ((1 + U)^2 - 1, U) |y|; flow = tf * tm, one product: exact."""
    mut = getattr(P, "mut", None)
    d0, tf, e, _ = _render_inputs(P)
    hw = P.Hp * P.Wp
    B.add("d0", d0.reshape(2 * hw, 8))
    B.add("tf", tf.reshape(8 * hw, 2))
    B.add("e", e.reshape(8 * hw, 1))
    B.add("sin", None, 8 * hw, 4, role="out")
    B.add("sfl", None, 8 * hw, 2, role="out")
    t32, t1 = _t_pair(P.t)
    win, wfl = [], []
    for s in range(8):
        td, tm = (t1, t32) if s % 2 == 0 else (t32, t1)
        if mut == "td_tm":
            td, tm = tm, td
        es = e[s].double().unsqueeze(-1)
        win.append(torch.cat([d0[s & 1, :, :, 2:5].double() * td * es, td * es], -1))
        wfl.append(tf[s].double() * tm)
    win, wfl = torch.stack(win), torch.stack(wfl)
    gam = torch.tensor([2.0 + U, 2.0 + U, 2.0 + U, 1.0], dtype=torch.float64)
    calls = [("vfi_m2m_splat_inputs", [B.ptr("d0"), 8, B.ptr("tf"), B.ptr("e"), C.c_float(P.t), B.ptr("sin"), B.ptr("sfl"), P.Hp, P.Wp])]
    with np.errstate(all="ignore"):
        bits = wfl.float()
    return calls, [dict(buf="sin", want=win, tol=gam * U * win.abs()), dict(buf="sfl", bits=bits)], dict(d0=d0, tf=tf, e=e), {}


def _craft_norm_at_threshold():
    """w such that ((w + c7) + c7) + 3 (c7 + c7) == float32(1e-5) in fp32, by bisection over the float's bit pattern"""
    c7 = np.float32(1e-7)

    def norm(w):
        n = np.float32(0)
        for b in range(4):
            n = n + (((w if b == 0 else np.float32(0)) + c7) + c7)
        return n
    lo, hi = np.float32(0).view(np.int32), np.float32(1e-5).view(np.int32)
    while hi - lo > 1:
        mid = np.int32((int(lo) + int(hi)) // 2)
        if norm(mid.view(np.float32)) < np.float32(1e-5):
            lo = mid
        else:
            hi = mid
    w = np.int32(hi).view(np.float32)
    return float(w) if norm(w) == np.float32(1e-5) else None


def op_combine(P, B):
    """vfi_m2m_combine alone on a crafted splat buffer [8,Hp,Wp,4]: random sums, a block of empty pixels (norm = 8 c7: holes), pixels whose
    norm is EXACTLY the threshold float32(1e-5) (not a hole: the test is <) and one float below it (a hole)."""
    mut = getattr(P, "mut", None)
    g = _g(P.seed)
    Hp, Wp, H, W = P.Hp, P.Wp, P.H, P.W
    hw = Hp * Wp
    d0 = torch.randn(2, Hp, Wp, 8, generator=g)
    sp = torch.randn(8, Hp, Wp, 4, generator=g)
    sp[..., 3] = torch.rand(8, Hp, Wp, generator=g) * 2.0
    sp[:, 2:9, 3:11] = 0.0
    w_thr = _craft_norm_at_threshold()
    assert w_thr is not None, "no fp32 weight puts the norm exactly on the threshold"
    n_at = 0
    for k, x in enumerate(range(0, W, 2)):
        sp[:, 0, x] = 0.0
        sp[0, 0, x, :3] = torch.randn(3, generator=g) * 1e-6
        sp[0, 0, x, 3] = w_thr if k % 2 == 0 else float(np.nextafter(np.float32(w_thr), np.float32(0)))
        n_at += k % 2 == 0
    stats = torch.tensor([0.45, 0.27])
    B.add("sp", sp.reshape(8 * hw, 4))
    B.add("d0", d0.reshape(2 * hw, 8))
    B.add("stats", stats.reshape(1, 2))
    B.add("out", None, H * W, 3, role="out")
    r = render64(d0, None, None, stats, P.t, H, W, mut, splats=sp)
    info = dict(holes=int(r["hole"].sum()), solid=int((~r["hole"]).sum()), at_threshold=n_at)
    calls = [("vfi_m2m_combine", [B.ptr("sp"), B.ptr("d0"), 8, B.ptr("stats"), C.c_float(P.t), B.ptr("out"), Hp, Wp, H, W])]
    return calls, [dict(buf="out", want=r["want"], tol=r["tol"])], dict(d0=d0, sp=sp, stats=stats), info


# ---------------------------------------------------------------------------------------------------------------- cube, pool, normalize

def op_cube_apply(P, B):
    """out = s3 * mean_k(cC[n, k C + c] cH[n, y, k] cW[n, x, k]), k < 16 (:786-795): module docstring."""
    g = _g(P.seed)
    N, H, W, Cc = P.N, P.H, P.W, P.C
    s3, cC = torch.randn(N, H, W, Cc, generator=g), torch.rand(N, 16, Cc, generator=g)
    cH, cW = torch.rand(N, H, 16, generator=g), torch.rand(N, W, 16, generator=g)
    B.add("s3", s3.reshape(-1, Cc), cs=Cc + P.pad, off=P.pad // 2)
    B.add("cC", cC.reshape(N, 16 * Cc))
    B.add("cH", cH.reshape(-1, 16), cs=16 + P.pad, off=P.pad // 2)
    B.add("cW", cW.reshape(-1, 16), cs=16 + P.pad + 1, off=P.pad // 2)
    B.add("out", None, N * H * W, Cc, Cc + P.pad + 2, P.pad // 2, role="out")
    terms = cC.double().view(N, 1, 1, 16, Cc) * cH.double().view(N, H, 1, 16, 1) * cW.double().view(N, 1, W, 16, 1)
    want = s3.double() * terms.sum(3) / 16
    tol = 19 * U * s3.double().abs() * terms.abs().sum(3) / 16
    args = [B.ptr("s3"), Cc + P.pad, B.ptr("cC"), B.ptr("cH"), 16 + P.pad, B.ptr("cW"), 16 + P.pad + 1, B.ptr("out"), Cc + P.pad + 2, N, H, W, Cc]
    return [("vfi_m2m_cube_apply", args)], [dict(buf="out", want=want, tol=tol)], dict(s3=s3, cC=cC, cH=cH, cW=cW), {}


def op_pool_mean(P, B):
    """adaptive_avg_pool2d to 1x1 / Hx1 / 1xW (:689-703): float64 accumulation, one conversion."""
    g = _g(P.seed)
    N, H, W, Cc = P.N, P.H, P.W, P.C
    x = torch.randn(N, H, W, Cc, generator=g) * P.sigma + P.mean
    B.add("in", x.reshape(-1, Cc), cs=Cc + 3, off=1)
    dims, L = {0: ((1, 2), 1), 1: ((2,), H), 2: ((1,), W)}[P.mode]
    B.add("out", None, N * L, Cc, Cc + 2, 1, role="out")
    xd = x.double()
    want = xd.mean(dims)
    n = H * W // L
    tol = U * want.abs() + (n + 2) * 2.0 ** -53 * xd.abs().mean(dims)
    if getattr(P, "mut", None) == "drop_pixel":          # the last pixel of every image left out of its sums
        xm = xd.clone()
        xm[:, -1, -1] = 0
        want = xm.mean(dims)
    return [("vfi_pool_mean", [B.ptr("in"), Cc + 3, B.ptr("out"), Cc + 2, N, H, W, Cc, P.mode])], [dict(buf="out", want=want, tol=tol)], dict(x=x), {}


def op_normalize(P, B):
    """vfi_m2m_normalize (:903-931): replicate padding, joint statistics, (x - mean) / (std + 1e-7).  Module docstring."""
    g = _g(P.seed)
    H, W, Hp, Wp, Cc = P.H, P.W, P.Hp, P.Wp, P.C
    if P.const is not None:
        f = torch.full((2, H, W, Cc), P.const)
    else:
        f = torch.randn(2, H, W, Cc, generator=g) * P.sigma + P.mean
        f[1] += P.shift
    B.add("f0", f[0].reshape(H * W, Cc))
    B.add("f1", f[1].reshape(H * W, Cc))
    B.add("out", None, 2 * Hp * Wp, 3, P.out_cs, P.out_off, role="out")
    B.add("stats", None, 1, 2, role="out")
    B.add("ws", None, 2048, 1, role="scratch", dtype=torch.float64)
    yi, xi = torch.arange(Hp).clamp(max=H - 1), torch.arange(Wp).clamp(max=W - 1)
    pd = f[:, yi][:, :, xi][..., :3].double()                  # [2,Hp,Wp,3]
    n = Hp * Wp * 3
    m = pd.mean((1, 2, 3))
    ex2 = (pd * pd).mean((1, 2, 3))
    v = ((pd - m.view(2, 1, 1, 1)) ** 2).mean((1, 2, 3))
    mean = m.mean()
    dk = (mean - m) ** 2
    var = (v + dk).mean()
    d53 = 2.0 ** -53
    dacc = (n + 2) * d53 * pd.abs().mean((1, 2, 3))             # the float64 sum / count; the fp32 conversion of m_k is charged where m_k is used
    dm = U * m.abs() + dacc
    tmean = 2 * U * mean.abs() + dm.mean()
    dv = (2 * n + 6) * d53 * ex2 + 2 * m.abs() * dacc + 2 * U * v      # v_k is formed from the float64 quotients: no rounded mean is squared
    ddk = 2 * (mean - m).abs() * (tmean + dm + U * (mean - m).abs()) + 5 * U * dk
    tvar = (dv + ddk).mean() + 2 * U * var
    root = var.sqrt()
    tsd = (tvar / (2 * (var - tvar).sqrt()) if float(var) > 4 * float(tvar) else tvar.sqrt() + root) + 3 * U * (root + C7)
    sd = root + C7
    num = pd - mean
    y = num / sd
    tol = (tmean + U * num.abs()) / sd + y.abs() * tsd / (sd - tsd).clamp_min(1e-300) + U * y.abs()
    if P.const is not None:
        tol = torch.zeros_like(tol)            # x - mean is exactly 0 for every positive divisor
    want_s = torch.stack([mean, sd]).view(1, 2)
    tol_s = torch.stack([tmean, tsd]).view(1, 2)
    args = [B.ptr("f0"), B.ptr("f1"), Cc, H, W, Hp, Wp, B.ptr("out", -P.out_off), P.out_cs, P.out_off, B.ptr("stats"), B.ptr("ws"), 2048 * 8]
    info = dict(tsd_rel=float(tsd / sd), sd=float(sd))
    return [("vfi_m2m_normalize", args)], [dict(buf="stats", want=want_s, tol=tol_s), dict(buf="out", want=y, tol=tol)], dict(f=f), info


OPS = {k[3:]: v for k, v in list(globals().items()) if k.startswith("op_")}


# ---------------------------------------------------------------------------------------------------------------- running a case

def build(case, device="cpu"):
    B = Buffers(device)
    calls, expects, ins, info = OPS[case.op](SimpleNamespace(**case.p), B)
    return B, calls, expects, ins, info


def check(outs, expects, what):
    """-> largest err / tol over the toleranced expectations (0.0 when all are exact)"""
    worst = 0.0
    for e in expects:
        got, name = outs[e["buf"]], f"{what}:{e['buf']}"
        if "bits" in e:
            compare_bits(got, e["bits"], name)
        elif "bits_from" in e:
            compare_bits(got, e["bits_from"](outs), name)
        elif "same_as" in e:
            compare_bits(got, outs[e["same_as"]], f"{name} vs {e['same_as']}")
        else:
            worst = max(worst, compare(got, e, name) or 0.0)
    return worst


def run_case(lib, case, device, stream, sync, check_rc):
    """Builds the buffers on `device`, sets the case's A/B options, calls the entry points of `lib`, restores the options, checks guards
    and results.  One synchronize."""
    B, calls, expects, _, _ = build(case, device)
    opts = case.p.get("opts") or {}
    try:
        for k, v in opts.items():
            assert lib.vfi_test_set_option(k.encode(), v) == 0
        for name, args in calls:
            check_rc(getattr(lib, name)(*args, stream), name)
        sync()
    finally:
        for k in opts:
            lib.vfi_test_set_option(k.encode(), OPTION_DEFAULTS[k])
    return check(B.finish(), expects, case.id)


# ---------------------------------------------------------------------------------------------------------------- case tables

def _w(tag, n, h, w, c, in_cs, in_off, out_cs, out_off, swap=0, kind="noise", flow="mixed"):
    return Case("warp_m2m", tag, seed=40 + c + h, N=n, H=h, W=w, C=c, in_cs=in_cs, in_off=in_off, out_cs=out_cs, out_off=out_off, flow_cs=4, flow_off=2,
                swap=swap, kind=kind, flow=flow)


# vfi_warp_m2m: vec = C % 4 == 0 && in_cs % 4 == 0 && out_cs % 4 == 0 && both pointers 16-byte aligned -> warp_m2m_kernel<true>, else <false>
WARP_CASES = []
for _h, _w_ in ((2, 2), (5, 7), (17, 17), (9, 14), (33, 47)):
    WARP_CASES += [_w(f"c3-scalar-{_h}x{_w_}-n2-swap", 2, _h, _w_, 3, 6, 1, 5, 1, swap=1), _w(f"c4-vec-{_h}x{_w_}-n4-swap", 4, _h, _w_, 4, 8, 4, 16, 8, swap=1),
                   _w(f"c8-vec-{_h}x{_w_}-n2", 2, _h, _w_, 8, 16, 4, 16, 4), _w(f"c9-scalar-{_h}x{_w_}-n4-swap", 4, _h, _w_, 9, 12, 0, 12, 1, swap=1)]
WARP_CASES += [_w("c8-vec-9x14-n4", 4, 9, 14, 8, 16, 4, 16, 4), _w("c3-scalar-33x47-n4", 4, 33, 47, 3, 6, 1, 5, 1), _w("c8-off1-scalar-9x14-n2", 2, 9, 14, 8, 16, 1, 16, 4), _w("c8-cs9-scalar-9x14-n2-swap", 2, 9, 14, 8, 9, 0, 16, 4, swap=1),
               _w("c8-out-off1-scalar-33x47-n2", 2, 33, 47, 8, 16, 4, 16, 1), _w("c3-scalar-9x14-n2-rand-pos", 2, 9, 14, 3, 6, 1, 5, 1, swap=1, kind="pos", flow="rand"),
               _w("c4-vec-33x47-n2-rand-pos", 2, 33, 47, 4, 8, 4, 8, 0, kind="pos", flow="rand")]
WARP_CASES += [Case("warp_image4", f"{h}x{w}", seed=50 + h, H=h, W=w, flow_cs=4, flow_off=2, out_cs=5, out_off=1, kind="noise")
               for h, w in ((2, 2), (5, 7), (17, 17), (9, 14), (33, 47))]

# vfi_m2m_photo / vfi_m2m_photo_tiles: vec_r = r_cs % 4 == 0 && r 16-byte aligned; x >= W || y >= H lanes of partial tiles
def _p(tag, h, w, r_cs=12, r_off=0, r_C=12, d0_cs=8, alpha=0.7, img_scale=1.0, flow="mixed", tiles=1):
    return Case("photo", tag, seed=60 + h, H=h, W=w, r_cs=r_cs, r_off=r_off, r_C=r_C, d0_cs=d0_cs, alpha=alpha, img_scale=img_scale, flow=flow, tiles=tiles)


PHOTO_CASES = [_p("2x2-vec", 2, 2), _p("37x45-vec-partial", 37, 45), _p("40x70-rcs9-scalar-partial", 40, 70, r_cs=9, r_C=9), _p("64x96-vec-d0cs6", 64, 96, d0_cs=6),
               _p("96x96-off1-scalar", 96, 96, r_cs=12, r_off=1, r_C=11), _p("37x45-alpha-clip20", 37, 45, alpha=50.0, flow="rand"),
               _p("37x45-alpha-neg-floor", 37, 45, alpha=-3.0e6, img_scale=3.0, flow="rand"), _p("40x70-alpha0", 40, 70, alpha=0.0, flow="rand"),
               _p("40x70-rand-d0cs6-rcs9", 40, 70, r_cs=9, r_C=9, d0_cs=6, flow="rand")]

# vfi_softsplat_sum (softsplat_sum_launch): splat_atomic == 3 && C == 4 && aligned -> softsplat4_kernel; c4 = C == 4 && in / out 16-byte aligned ->
# softsplat_list_kernel<4>, else softsplat_list_kernel<0> + softsplat_gather_kernel; splat_atomic == 1 -> softsplat_tile_kernel per 8 channels
# (<4> when 4 remain); list path: cells above 8 sources spill to the tail kernel, a spill list above splat_spill_cap redoes the launch with the
# tile kernel; |f| > 63 -> the far pass of the tail kernel
def _s(tag, n, h, w, c, field, mis=0, **opts):
    return Case("softsplat", tag + "".join(f"-{k.split('_')[-1]}{v}" for k, v in opts.items()), seed=70 + c + h, N=n, H=h, W=w, C=c, field=field, mis=mis, opts=opts)


SPLAT_CASES = [_s("c1-5x7-n2-mixed", 2, 5, 7, 1, "mixed"), _s("c3-33x47-n2-mixed", 2, 33, 47, 3, "mixed"), _s("c4-33x47-n1-mixed", 1, 33, 47, 4, "mixed"),
               _s("c4-off1-33x47-n2-mixed", 2, 33, 47, 4, "mixed", mis=1), _s("c8-70x90-n1-mixed", 1, 70, 90, 8, "mixed"), _s("c9-64x96-n1-mixed", 1, 64, 96, 9, "mixed"),
               _s("c12-33x47-n2-mixed", 2, 33, 47, 12, "mixed"), _s("c4-70x90-n2-translate", 2, 70, 90, 4, "translate"), _s("c3-70x90-n1-translate", 1, 70, 90, 3, "translate"),
               _s("c4-64x96-n1-noise1", 1, 64, 96, 4, "noise1"), _s("c9-33x47-n1-noise1", 1, 33, 47, 9, "noise1"), _s("c4-96x160-n1-noise8", 1, 96, 160, 4, "noise8"),
               _s("c4-64x96-n1-huge", 1, 64, 96, 4, "huge"), _s("c3-5x7-n1-point", 1, 5, 7, 3, "point")]
for _field, _c, _h, _ww in (("zoom", 4, 64, 96), ("zoom8", 4, 70, 90), ("zoom", 9, 33, 47), ("point", 4, 33, 47), ("point", 12, 33, 47), ("far", 4, 96, 160), ("far", 3, 70, 90),
                            ("near64", 4, 70, 90), ("near64", 8, 64, 96), ("noise8", 3, 64, 96), ("mixed", 4, 70, 90)):
    for _o in ({}, dict(splat_atomic=1), dict(splat_spill_cap=64)) + ((dict(splat_atomic=3),) if _c == 4 else ()):
        SPLAT_CASES.append(_s(f"c{_c}-{_h}x{_ww}-n1-{_field}", 1, _h, _ww, _c, _field, **_o))


def _r(op, tag, hp, wp, h, w, field, t, e20=0, form=None):
    return Case(op, tag, seed=80 + hp + w, Hp=hp, Wp=wp, H=h, W=w, field=field, t=t, e20=e20, **({} if form is None else dict(form=form)))


_RENDER = [("64x64-smooth-t0.5", 64, 64, 64, 64, "smooth", 0.5, 0), ("37x45-wavy-t0.25", 37, 45, 37, 45, "wavy", 0.25, 0), ("96x128-crop40x70-smooth-t0.667", 96, 128, 40, 70, "smooth", 2.0 / 3.0, 0),
           ("96x96-crop90x91-translate-t0.5", 96, 96, 90, 91, "translate", 0.5, 0), ("64x128-crop60x121-mixed-t0.5", 64, 128, 60, 121, "mixed8", 0.5, 0),
           ("64x64-smooth-t0", 64, 64, 64, 64, "smooth", 0.0, 0), ("64x64-wavy-t1", 64, 64, 64, 64, "wavy", 1.0, 0), ("96x96-crop90x91-noise8-t0.5", 96, 96, 90, 91, "noise8", 0.5, 0),
           ("64x64-zoom-t0.5", 64, 64, 64, 64, "zoom_r", 0.5, 0), ("64x64-zoom8-t0.5", 64, 64, 64, 64, "zoom8_r", 0.5, 0), ("37x45-point-t0.5", 37, 45, 37, 45, "point_r", 0.5, 0),
           ("64x64-smooth-t1", 64, 64, 64, 64, "smooth", 1.0, 0),
           ("96x128-crop40x70-far-t0.5", 96, 128, 40, 70, "far", 0.5, 0), ("64x128-crop60x121-hole-t0.5", 64, 128, 60, 121, "hole", 0.5, 0), ("64x64-hole-t0.25", 64, 64, 64, 64, "hole", 0.25, 0),
           ("37x45-mixed-t0.25", 37, 45, 37, 45, "mixed8", 0.25, 0), ("64x64-smooth-e20-t0.5", 64, 64, 64, 64, "smooth", 0.5, 1), ("96x96-crop90x91-huge-t0.667", 96, 96, 90, 91, "huge", 2.0 / 3.0, 0)]
RENDER_CASES = [_r("render", f"{form}-{c[0]}", *c[1:], form=form) for c in _RENDER for form in ("three", "fused")]
SPLAT_INPUTS_CASES = [_r("splat_inputs", c[0], *c[1:]) for c in _RENDER if c[0] in ("37x45-mixed-t0.25", "64x64-smooth-t0", "64x64-wavy-t1", "64x64-smooth-e20-t0.5", "96x128-crop40x70-smooth-t0.667")]
COMBINE_CASES = [Case("combine", f"{hp}x{wp}-crop{h}x{w}-t{t:.3g}", seed=90 + hp, Hp=hp, Wp=wp, H=h, W=w, t=t)
                 for hp, wp, h, w, t in ((64, 64, 64, 64, 0.5), (37, 45, 37, 45, 0.25), (96, 128, 40, 70, 2.0 / 3.0), (96, 96, 90, 91, 0.0), (64, 128, 60, 121, 1.0))]

CUBE_CASES = [Case("cube_apply", tag, seed=100 + c, N=n, H=h, W=w, C=c, pad=pad) for tag, n, h, w, c, pad in (("c256-7x10", 2, 7, 10, 256, 0), ("c5-1x1-window", 2, 1, 1, 5, 4), ("c5-3x2-window", 2, 3, 2, 5, 2))]
# vfi_pool_mean: mode != 0 && C <= 32 && pooled length >= 256 -> pool_mean_fewc_kernel; mode == 0 -> pool_global_kernel; else pool_mean_kernel
POOL_CASES = [Case("pool_mean", tag, seed=110 + c, N=n, H=h, W=w, C=c, mode=mode, mean=mu, sigma=sg)
              for tag, n, h, w, c, mode, mu, sg in (("global-c70-9x14", 2, 9, 14, 70, 0, 0.3, 1.0), ("global-c3-1x1", 2, 1, 1, 3, 0, 0.3, 1.0), ("global-c64-mean1000", 1, 33, 47, 64, 0, 1000.0, 0.01),
                                                    ("fewc-mode1-c3-5x300", 2, 5, 300, 3, 1, 0.3, 1.0), ("fewc-mode2-c32-256x3", 1, 256, 3, 32, 2, 0.3, 1.0), ("fewc-mode1-c4-mean1000", 1, 3, 257, 4, 1, 1000.0, 0.01),
                                                    ("rows-mode1-c33-2x300", 1, 2, 300, 33, 1, 0.3, 1.0), ("rows-mode2-c3-255x2", 2, 255, 2, 3, 2, 0.3, 1.0), ("rows-mode1-c300-3x5", 2, 3, 5, 300, 1, 0.3, 1.0),
                                                    ("rows-mode2-c70-mean1000", 1, 9, 14, 70, 2, 1000.0, 0.01))]
NORMALIZE_CASES = [Case("normalize", tag, seed=120 + h, H=h, W=w, Hp=hp, Wp=wp, C=c, mean=mu, sigma=sg, shift=sh, const=const, out_cs=8, out_off=2)
                   for tag, h, w, hp, wp, c, mu, sg, sh, const in (("1x1-to-64x64-c3", 1, 1, 64, 64, 3, 0.4, 0.2, 0.3, None), ("50x70-to-64x128-c4", 50, 70, 64, 128, 4, 0.4, 0.2, 0.1, None),
                                                                   ("50x70-to-64x128-c3-mean1000", 50, 70, 64, 128, 3, 1000.0, 1.0, 0.0, None), ("50x70-const0.5", 50, 70, 64, 128, 3, 0, 0, 0, 0.5),
                                                                   ("50x70-const0.3-c4", 50, 70, 64, 128, 4, 0, 0, 0, 0.3))]

TABLES = dict(warp=WARP_CASES, photo=PHOTO_CASES, softsplat=SPLAT_CASES, splat_inputs=SPLAT_INPUTS_CASES, combine=COMBINE_CASES, render=RENDER_CASES,
              cube=CUBE_CASES, pool=POOL_CASES, normalize=NORMALIZE_CASES)
ALL_CASES = [c for t in TABLES.values() for c in t]
_by_id = {c.id: c for c in ALL_CASES}
assert len(_by_id) == len(ALL_CASES)

# (a case, the mutation of its restatement): each must FAIL the comparison with the device result, and with the oracle's on the CPU
MUTATIONS = [(_by_id[i].but(mut=m), m) for m, ids in (
    ("drop7th", ("softsplat-c4-64x96-n1-zoom", "softsplat-c4-70x90-n1-zoom8-atomic3", "softsplat-c9-33x47-n1-zoom", "render-fused-64x64-zoom8-t0.5", "render-three-64x64-zoom-t0.5")),
    ("edge_column", ("softsplat-c4-70x90-n1-mixed", "softsplat-c8-70x90-n1-mixed", "softsplat-c4-70x90-n1-mixed-atomic3", "render-fused-64x128-crop60x121-mixed-t0.5")),
    ("swap_ne_sw", ("softsplat-c4-64x96-n1-noise1", "softsplat-c9-33x47-n1-noise1", "render-fused-64x64-smooth-t0.5", "render-three-37x45-wavy-t0.25")),
    ("td_tm", ("render-fused-37x45-wavy-t0.25", "render-three-96x128-crop40x70-smooth-t0.667", "splat_inputs-37x45-mixed-t0.25")),
    ("no_c7", ("render-fused-64x128-crop60x121-hole-t0.5", "render-three-64x64-hole-t0.25", "combine-64x64-crop64x64-t0.5")),
    ("hole_le", ("combine-64x64-crop64x64-t0.5", "combine-96x128-crop40x70-t0.667")),
    ("no_fill", ("render-fused-64x64-hole-t0.25", "render-three-64x128-crop60x121-hole-t0.5", "combine-37x45-crop37x45-t0.25")),
    ("wei_no_01", ("photo-64x96-vec-d0cs6", "photo-40x70-rand-d0cs6-rcs9")),
    ("no_floor", ("photo-37x45-alpha-neg-floor", "photo-37x45-vec-partial", "photo-64x96-vec-d0cs6")),
    ("no_clip", ("photo-37x45-alpha-clip20",)),
    ("noswap", ("photo-37x45-vec-partial", "warp_m2m-c4-vec-33x47-n4-swap", "warp_image4-9x14")),
    ("border", ("warp_m2m-c3-scalar-9x14-n2-swap", "warp_m2m-c8-vec-33x47-n2", "warp_image4-33x47", "photo-40x70-rcs9-scalar-partial")),
    ("ranges_all", ("photo-37x45-vec-partial", "photo-96x96-off1-scalar")),
    ("sclx_both", ("warp_m2m-c3-scalar-9x14-n2-swap", "warp_m2m-c8-vec-33x47-n2", "warp_image4-33x47", "photo-40x70-rand-d0cs6-rcs9")),
    ("drop_pixel", ("pool_mean-fewc-mode1-c3-5x300", "pool_mean-global-c70-9x14")),
) for i in ids]
