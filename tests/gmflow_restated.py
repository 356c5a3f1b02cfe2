"""Float64 restatements, per-element bounds, case tables and wrong restatements for the GMFlow device kernels of the GMFSS node:
csrc/attention.hip (attention_kernel<4> / <1>, attention_merge_kernel, att_row's window addressing, the key-split rule of
attention_launch_t) and csrc/gmfss_fast.hip (layernorm_wave_kernel, local_match_mfma_kernel, local_prop_coop_kernel).  Conventions
of tests/small_ops_restated.py (U, E_EXP, TINY, Buffers, compare, Case come from there); no product code is imported.  Each op is the
mathematical function of the reference formula its kernel cites (GMFSS_Fortuna_union_arch.py:367-436, 479-523, 708-803, 806-843,
846-913; the shifted-window mask :326-364) evaluated in float64 on the fp32 inputs, with a per-element bound counted from the
kernel's own sequence of roundings (each op's docstring).  No constant below was fitted to what a device returns.

SOFTMAX-WEIGHTED SUMS.  out = sum_n p_n v_n, p = softmax(t).  If the kernel's weight of key n is p_n e^(l_n) (the SAME weight in the
numerator and in the normalising sum: every kernel here computes a key's exponential once and uses it for both), then
    out' - out = sum_n p_n (e^(l_n) - 1) (v_n - out) / sum_n p_n e^(l_n)                (since sum_n p_n (v_n - out) = 0)
so |out' - out| <= sum_n p_n (e^(|l_n|) - 1) |v_n - out| / (1 - sum_n p_n |l_n|): `weighted_bound`.  With every |l_n| <= eps this is at
most (e^(2 eps) - 1) sum_n p_n |v_n - out|, the per-row form; the per-key form used here is never larger.  l_n collects the error of
the logit and of every exponential the weight passes through.  What numerator and denominator do NOT share (their own accumulation
roundings, the final reciprocal / division) is added as U * count * (sum_n p_n |v_n|  resp.  |out|).

FAST EXPONENTIAL.  attention.hip uses __expf = exp2(x * log2e): the rounded constant and the rounded product move the result by
2 |x| U relative, the instruction itself by E_EXP ulp = 2 E_EXP U (the suite's figure for expf: no accuracy table of the native
instruction exists here, and the figure is not fitted): rel_fast_exp(x).  The online softmax subtracts running maxima m_0 <= m_1 <= ..
<= M: a key of block i carries e^(x - m_i) e^(m_i - m_(i+1)) ... (and e^(m_z - M) in the merge of a key split); the arguments
telescope to x - M, so the argument roundings and the 2 |x| U terms add up to 3 U (M - x), plus 2 E_EXP U per exponential.
Terms below 2^-126 may be flushed: TINY times what they multiply.

`mn` (positive inputs only): for every dropped summand (key / tap / channel) the largest change over the row's output channels, in
units of that channel's tolerance, scaled back by the tolerance: mn > tol <=> every single summand is visible in some channel.
"""
import ctypes as C
import math
from types import SimpleNamespace

import torch

from small_ops_restated import E_EXP, INF, NAN, TINY, U, Buffers, Case, compare

ATT_C, KB = 128, 32


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def rel_fast_exp(x):
    """relative error of __expf(x) for an fp32 x (module docstring)"""
    return 2 * x.abs() * U + 2 * E_EXP * U


def weighted_bound(p, lam, v, out):
    """sum_n p_n (e^lam_n - 1) |v_n - out| / (1 - sum_n p_n lam_n).  p, lam [.., m, n]; v [.., n, c]; out [.., m, c]"""
    dev = (v.unsqueeze(-3) - out.unsqueeze(-2)).abs()                      # [.., m, n, c]
    num = ((p * torch.expm1(lam)).unsqueeze(-1) * dev).sum(-2)
    den = 1 - (p * lam).sum(-1, keepdim=True)
    assert float(den.min()) > 0.5
    return num / den


def summand_floor(p, v, out, tol, live=None):
    """mn of the module docstring: p [.., m, n], v [.., n, c], out / tol [.., m, c]; live [.., m, n]: the summands that count (a key
    behind a -100 mask or a tap at -1e9 has no weight to lose)"""
    if p.shape[-1] == 1:
        return None
    change = (p / (1 - p).clamp_min(1e-300)).unsqueeze(-1) * (v.unsqueeze(-3) - out.unsqueeze(-2)).abs()
    r = (change / tol.unsqueeze(-2).clamp_min(1e-300)).amax(-1)
    if live is not None:            # (a row with one live summand has nothing left when it is dropped)
        r = torch.where(live & (live.sum(-1, keepdim=True) > 1), r, torch.full_like(r, INF))
    r = r.amin(-1)         # [.., m]
    return tol * r.unsqueeze(-1)


# ---------------------------------------------------------------------------------------------------------------- key split

def split_rule(Lk, req):
    """attention_launch_t's rule for a requested number of key ranges: at most 8, at most one per 32-key block, then reduced so that
    no range is empty.  -> (ks, blocks per range)"""
    nblk = -(-Lk // KB)
    ks = max(1, min(req, 8, nblk))
    per = -(-nblk // ks)
    return -(-nblk // per), per


# ---------------------------------------------------------------------------------------------------------------- attention

def attention_f64(q, k, v, alpha, labels, period, ks, mut=None):
    """out[b, m] = sum_n softmax_n(alpha q[b, m] . k[b, n] + mask) v[b, n]; mask = -100 where label[b % period][m] != label[b % period][n]
    (:367-436, :806-843, :708-745).  q [nb, Lq, 128], k [nb, Lk, 128], v [nb, Lk, DV] float64, ks = the number of key ranges that ran.

    Logit: 128 exact products, fp32 sums in some association (two chains and their sum), the product with alpha:
    (K + 2) U |alpha| sum_c |q_c k_c|; with labels the mask addition rounds once more, U |t|.  Weight: module docstring, with
    1 + (blocks after the key's in its range) exponentials, one more in a split.  Not shared: the value sum (Lk + 1) U sum p |v|, its
    rescaling by the running correction once per block, nblk U sum p |v|; the normalising sum Lk + nblk roundings, the reciprocal and
    its product: (Lk + nblk + 2) U |out|; in a split one product and one addition per range on both sides, 2 ks U (sum p |v| + |out|).
    Flushed weights: TINY (sum_n |v_n| + Lk |out|)."""
    nb, Lq, _ = q.shape
    Lk, DV = v.shape[1], v.shape[2]
    nblk = -(-Lk // KB)
    a = 1.0 if mut == "alpha omitted" else alpha
    dots = torch.matmul(q, k.transpose(1, 2))
    t = dots * a
    eps = (ATT_C + 2) * U * abs(a) * torch.matmul(q.abs(), k.abs().transpose(1, 2))
    if labels is not None:
        rows = torch.arange(nb).clamp_max(period - 1) if mut == "label row b" else torch.arange(nb) % period
        lab = labels[rows].long()                                              # [nb, L]
        differ = lab[:, :, None] != lab[:, None, :]
        if mut == "mask where equal":
            differ = ~differ
        t = t + torch.where(differ, -100.0, 0.0)
        eps = eps + U * t.abs()
    keep = torch.ones(Lk, dtype=torch.bool)
    if mut == "last key dropped":
        keep[Lk - 1] = False
    if mut == "key 31 dropped":
        keep[31] = False
    if mut == "key 32 dropped":
        keep[32] = False
    t = torch.where(keep, t, torch.full_like(t, -INF))
    vv = v
    if mut == "value channels exchanged":
        vv = v.clone()
        vv[..., 4:8], vv[..., 8:12] = v[..., 8:12], v[..., 4:8]
    if mut == "padding keys counted":
        pad = nblk * KB - Lk
        t = torch.cat([t, torch.zeros(nb, Lq, pad, dtype=t.dtype)], 2)
        eps = torch.cat([eps, torch.zeros(nb, Lq, pad, dtype=t.dtype)], 2)
        vv = torch.cat([vv, torch.zeros(nb, pad, DV, dtype=t.dtype)], 1)
    n_keys = t.shape[2]
    ks, per = split_rule(Lk, ks)
    if mut == "softmax over queries":
        p = torch.softmax(t, 1)
    elif mut == "merge without rescale":
        assert ks > 1
        e = torch.zeros_like(t)
        for z in range(ks):
            sl = slice(z * per * KB, min((z + 1) * per * KB, n_keys))
            e[..., sl] = torch.exp(t[..., sl] - t[..., sl].amax(-1, keepdim=True))
        p = e / e.sum(-1, keepdim=True)
    else:
        p = torch.softmax(t, -1)
    out = torch.matmul(p, vv)
    M = t.amax(-1, keepdim=True)
    blk = torch.arange(n_keys) // KB
    last = torch.minimum((blk // per + 1) * per, torch.tensor(-(-n_keys // KB))) - 1
    n_exp = (1 + (last - blk) + (1 if ks > 1 else 0)).double()
    gap = torch.where(torch.isinf(t), torch.zeros_like(t), M - t) + 2 * eps.amax(-1, keepdim=True)
    lam = eps + U * gap + (rel_fast_exp(gap) - 2 * E_EXP * U) + 2 * E_EXP * U * n_exp
    s_abs = torch.matmul(p, vv.abs())
    split = 2 * ks if ks > 1 else 0
    tol = torch.empty_like(out)
    for b in range(nb):            # (one batch entry at a time: the [m, n, c] deviation tensor is the large one)
        tol[b] = weighted_bound(p[b], lam[b], vv[b], out[b])
    tol = tol + U * ((Lk + 1 + nblk + split) * s_abs + (Lk + nblk + 2 + split) * out.abs()) + TINY * (vv.abs().sum(1, keepdim=True) + Lk * out.abs())
    return out, tol, p, vv, t > -50


def shift_labels_restated(h, w, K, sh, sw):
    """generate_shift_window_attn_mask (:326-364) as one region label per token, int32 [K K, wh ww] in window order: the image mask
    counts the 3 x 3 regions cut by slice(0, -win), slice(-win, -shift), slice(-shift, None) on each axis; two tokens of a window
    attend to each other iff their counts are equal."""
    wh, ww = h // K, w // K
    img = torch.zeros(h, w, dtype=torch.int32)
    cnt = 0
    for hs in (slice(0, -wh), slice(-wh, -sh), slice(-sh, None)):
        for ws in (slice(0, -ww), slice(-ww, -sw), slice(-sw, None)):
            img[hs, ws] = cnt
            cnt += 1
    return img.view(K, wh, K, ww).permute(0, 2, 1, 3).reshape(K * K, wh * ww).contiguous()


def to_windows(t, K, sh, sw, swap=False, wrong_image=False):
    """[B, h, w, c] -> [B K K, wh ww, c]: roll by (-sh, -sw), split into K x K windows (:367-436, split_feature :1059-1120)"""
    B, h, w, c = t.shape
    t = torch.roll(t, (-sh, -sw), (1, 2))
    t = t.view(B, K, h // K, K, w // K, c).permute(0, 3, 1, 2, 4, 5) if swap else t.view(B, K, h // K, K, w // K, c).permute(0, 1, 3, 2, 4, 5)
    t = t.reshape(B * K * K, (h // K) * (w // K), c)
    if wrong_image:      # entry b of the batch read from image (b / K) % B instead of b / K^2
        b = torch.arange(B * K * K)
        t = t[((b // K) % B) * K * K + b % (K * K)]
    return t


def from_windows(t, B, h, w, K, sh, sw, swap=False):
    c = t.shape[-1]
    t = t.view(B, K, K, h // K, w // K, c)
    t = t.permute(0, 2, 3, 1, 4, 5) if swap else t.permute(0, 1, 3, 2, 4, 5)
    return torch.roll(t.reshape(B, h, w, c), (sh, sw), (1, 2))


# ---------------------------------------------------------------------------------------------------------------- inputs

def attention_inputs(P):
    """-> q [nb, Lq, 128], k [nb, Lk, 128], v [nb, Lk, DV] fp32.  noise: N(0, 1).  pos: [0.5, 1].  peaky: N(0, 1) * gain, near one-hot
    rows.  planted: small noise, k channel 1 = 1 for every key, k channel 0 a ramp rising with the key index, k channel 2 one-hot at
    key min(3, Lk - 1) and channel 3 one-hot at key Lk - 1; the first six queries load these channels: +300 on one key, -300 on all,
    the maximum in the first block, in the last block, rising from block to block, and the ramp downwards; v channel 0 = key index."""
    g = _g(P.seed)
    nb, Lq, Lk, DV = P.nb, P.Lq, P.Lk, P.DV
    if P.kind == "pos":
        q, k, v = (0.5 + 0.5 * torch.rand(nb, L, c, generator=g) for L, c in ((Lq, ATT_C), (Lk, ATT_C), (Lk, DV)))
    else:
        s = {"noise": 1.0, "peaky": P.gain if hasattr(P, "gain") else 7.0, "planted": 0.3}[P.kind]
        q, k = torch.randn(nb, Lq, ATT_C, generator=g) * s, torch.randn(nb, Lk, ATT_C, generator=g) * s
        v = torch.randn(nb, Lk, DV, generator=g)
    if P.kind == "planted":
        ia = 1.0 / P.alpha
        k[:, :, 0:4] = 0
        q[:, :, 0:4] = 0
        top = 8.0 * -(-Lk // KB) + 1.0                                   # logits 8 (block + 1) + (key % 32) / 32: every block tops the one before by 8
        k[:, :, 0] = (8.0 * (torch.arange(Lk) // KB + 1) + (torch.arange(Lk) % KB) / 32.0) / top
        k[:, :, 1] = 1.0
        k[:, min(3, Lk - 1), 2] = 1.0
        k[:, Lk - 1, 3] = 1.0
        plan = [(2, 300.0), (1, -300.0), (2, 25.0), (3, 25.0), (0, top), (0, -top)]
        for m, (ch, val) in enumerate(plan[:Lq]):
            q[:, m, ch] = val * ia
        v[:, :, 0] = torch.arange(Lk, dtype=torch.float32)
    return q, k, v


def attention_labels(P):
    """[period, L] int32 classes 0..2 from the seed; with 'lone' the class of token 0 is its own (a one-hot row through the -100 masks),
    with 'tail' the last min(3, L) tokens form a class of their own, confined to the tail of the last key block."""
    if not P.period:
        return None
    lab = torch.randint(0, 3, (P.period, P.Lk), generator=_g(P.seed + 77), dtype=torch.int32)
    if "lone" in P.lab:
        lab[:, 0] = 7
    if "tail" in P.lab:
        lab[:, -min(3, P.Lk):] = 9
    return lab


class _Keep:
    """an int32 operand outside `Buffers` (which is NaN-filled): guarded by a sentinel on both sides, compared bit for bit afterwards"""

    def __init__(self, t, device):
        self.host = torch.cat([torch.full((4,), -12345, dtype=torch.int32), t.reshape(-1), torch.full((4,), -12345, dtype=torch.int32)])
        self.dev = self.host.clone().to(device)

    def ptr(self):
        return self.dev.data_ptr() + 16

    def check(self):
        assert torch.equal(self.dev.cpu(), self.host), "the label map was written to"


def _vwin(P):
    """(q_cs, q_off, v_cs, v_off, out_cs, out_off) of an attention case"""
    if P.DV == 128:
        return (136, 4, 136, 4, 140, 8) if P.win else (128, 0, 128, 0, 128, 0)
    return (136, 4, P.DV + 3, 1, P.DV + 3, 1) if P.win else (128, 0, P.DV, 0, P.DV, 0)


def op_attention(P, B):
    """vfi_attention: attention_f64's docstring holds the count."""
    P.alpha = _f32(1.0 / math.sqrt(ATT_C))
    q, k, v = attention_inputs(P)
    labels = attention_labels(P)
    qcs, qoff, vcs, voff, ocs, ooff = _vwin(P)
    B.add("q", q.reshape(-1, ATT_C), cs=qcs, off=qoff)
    B.add("k", k.reshape(-1, ATT_C), cs=qcs, off=qoff)
    B.add("v", v.reshape(-1, P.DV), cs=vcs, off=voff)
    B.add("out", None, P.nb * P.Lq, P.DV, ocs, ooff, role="out")
    lab = _Keep(labels, B.device) if labels is not None else None
    if lab is not None:
        B.keep = [lab]
    want, tol, p, vv, live = attention_f64(q.double(), k.double(), v.double(), P.alpha, labels, P.period, P.ks_ran, getattr(P, "mut", None))
    mn = summand_floor(p, vv, want, tol, live) if P.kind == "pos" and getattr(P, "mut", None) is None else None
    args = [B.ptr("q"), qcs, B.ptr("k"), qcs, B.ptr("v"), vcs, B.ptr("out"), ocs, P.nb, P.Lq, P.Lk, ATT_C, P.DV, C.c_float(P.alpha),
            lab.ptr() if lab is not None else None, P.period]
    return [("vfi_attention", args)], [dict(buf="out", want=want, tol=tol, mn=mn)]


def op_window_attention(P, B):
    """vfi_window_attention: roll by (-sh, -sw), K x K windows, attention_f64 per window with the restated label map when shifted, merge,
    roll back (:367-436).  The addressing is exact; the bound is attention_f64's, carried to the pixel it belongs to."""
    P.alpha = _f32(1.0 / math.sqrt(ATT_C))
    g = _g(P.seed)
    Bn, h, w, K, sh, sw = P.B, P.h, P.w, P.K, P.sh, P.sw
    mk = (lambda: 0.5 + 0.5 * torch.rand(Bn, h, w, ATT_C, generator=g)) if P.kind == "pos" else (lambda: torch.randn(Bn, h, w, ATT_C, generator=g) * (P.gain if P.kind == "peaky" else 1.0))
    q, k, v = mk(), mk(), mk()
    labels = shift_labels_restated(h, w, K, sh, sw) if (sh or sw) else None
    cs, off = (136, 4) if P.win else (128, 0)
    for nm, t in (("q", q), ("k", k), ("v", v)):
        B.add(nm, t.reshape(-1, ATT_C), cs=cs, off=off)
    B.add("out", None, Bn * h * w, ATT_C, cs, off, role="out")
    lab = _Keep(labels, B.device) if labels is not None else None
    if lab is not None:
        B.keep = [lab]
    mut = getattr(P, "mut", None)
    s_in = (sh, sw) if mut != "roll with the opposite sign" else (-sh, -sw)
    s_out = (0, 0) if mut == "roll not undone" else s_in
    swap = mut == "wy and wx exchanged"
    tw = lambda t: to_windows(t.double(), K, s_in[0], s_in[1], swap=swap, wrong_image=mut == "image from the wrong quotient")
    o, tol, p, vv, live = attention_f64(tw(q), tw(k), tw(v), P.alpha, labels, K * K, 1, None)
    mn = summand_floor(p, vv, o, tol, live) if P.kind == "pos" and mut is None else None
    back = lambda t: from_windows(t, Bn, h, w, K, s_out[0], s_out[1], swap=swap)
    args = [B.ptr("q"), cs, B.ptr("k"), cs, B.ptr("v"), cs, B.ptr("out"), cs, Bn, h, w, K, sh, sw, ATT_C, C.c_float(P.alpha), lab.ptr() if lab is not None else None]
    return [("vfi_window_attention", args)], [dict(buf="out", want=back(o), tol=back(tol), mn=back(mn) if mn is not None else None)]


# ---------------------------------------------------------------------------------------------------------------- local match

R_MATCH = 4       # (X + d) - c, / c, + 1, * (size - 1)       (local_match_*'s caller chain and ztap_from_norm; X + d, c = (size-1)/2 and / 2 are exact)
LM_STEPS = 41     # online softmax steps of one lane of local_match_mfma_kernel (81 taps over two lanes)


def _shifted(t, dy, dx, fill):
    """t [N, H, W, ..] read at (y + dy, x + dx); `fill` outside the image"""
    N, H, W = t.shape[:3]
    out = torch.full_like(t, fill)
    if abs(dy) >= H or abs(dx) >= W:
        return out
    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    out[:, yd, xd] = t[:, ys, xs]
    return out


def local_match_f64(f0, f1, prior, r, body, mut=None):
    """flow += E[window offset] under softmax_j(f0 . f1(pixel + o_j) / sqrt(C)), o_j = (dx, dy) row-major over the (2r+1)^2 window,
    -1e9 where the position is outside the image (:846-913), at exact integer positions.  f0, f1 [N, H, W, C], prior [N, H, W, 2].

    Logit value: C exact products and their sums, the blend of up to four integer-position products (two 1 - w, the weight products,
    the four products, three additions: the sampler's 8), sqrt(C) and the division: (C + 12) U A, A = the largest sum_c |q_c k_c| / sqrt(C)
    over the position and its in-image neighbours.  Logit position: the kernel's window position goes through R_MATCH roundings of
    quantities of at most |p| + size - 1 pixels, so it is off by R_MATCH U (|p| + size - 1) per axis, times the spread of the integer-
    position products over the 3 x 3 neighbourhood (0 outside the image, as the skipped taps).  Weight: expf within E_EXP ulp of an
    argument rounded once (U times it; arguments telescope as in attention), up to LM_STEPS + 1 exponentials on its way (each online step
    rescales, the two lanes merge).  Not shared: 2 (LM_STEPS + 1) + 2 roundings on each side.  The in-place addition: U |flow|.
    body (the per-pixel form of gmfss_bodies.h): one exponential; it sums p (X + dx) and subtracts X: (2 J + 3) U sum p |X + dx| and
    U |delta|, J = (2r+1)^2."""
    N, H, W, Cc = f0.shape
    r_eff = 3 if mut == "radius 3" else r
    D = 2 * r_eff + 1
    scale = math.sqrt(Cc)
    offs = [(j % D - r_eff, j // D - r_eff) for j in range(D * D)]   # (dx, dy), row-major (:935-946, 866-876)
    # 'offsets column-major': the in-image test of entry j made at (dy, dx), the column-major reading of j, while its score and offset stay row-major
    ones = torch.ones(N, H, W, dtype=torch.float64)
    prod = {}
    for dy in range(-r_eff - 1, r_eff + 2):
        for dx in range(-r_eff - 1, r_eff + 2):
            kk = _shifted(f1, dy, dx, 0.0)
            prod[(dx, dy)] = ((f0 * kk).sum(-1) / scale, (f0.abs() * kk.abs()).sum(-1) / scale)
    X = torch.arange(W, dtype=torch.float64).view(1, 1, W).expand(N, H, W)
    Y = torch.arange(H, dtype=torch.float64).view(1, H, 1).expand(N, H, W)
    t, eps = [], []
    for dx, dy in offs:
        s, _ = prod[(dx, dy)]
        valid = _shifted(ones, dx, dy, 0.0) > 0 if mut == "offsets column-major" else _shifted(ones, dy, dx, 0.0) > 0
        nb_s = torch.stack([prod[(dx + i, dy + j)][0] for i in (-1, 0, 1) for j in (-1, 0, 1)])
        nb_a = torch.stack([prod[(dx + i, dy + j)][1] for i in (-1, 0, 1) for j in (-1, 0, 1)])
        pos = R_MATCH * U * ((X + dx).abs() + W - 1) + R_MATCH * U * ((Y + dy).abs() + H - 1)
        e = (Cc + 12) * U * nb_a.amax(0) + pos * (nb_s.amax(0) - nb_s.amin(0))
        fill = 0.0 if mut == "outside scored 0" else -1e9
        t.append(torch.where(valid, s, torch.full_like(s, fill)))
        eps.append(torch.where(valid, e, torch.zeros_like(e)))
    t, eps = torch.stack(t, -1), torch.stack(eps, -1)                            # [N, H, W, J]
    p = torch.softmax(t, -1)
    o = torch.tensor([(dy, dx) if mut == "dx and dy exchanged" else (dx, dy) for dx, dy in offs], dtype=torch.float64)     # [J, 2]
    delta = torch.matmul(p, o)
    M = t.amax(-1, keepdim=True)
    gap = M - t + 2 * eps.amax(-1, keepdim=True)
    n_exp = 1 if body else LM_STEPS + 1
    lam = eps + U * gap + 2 * E_EXP * U * n_exp
    tol = weighted_bound(p.reshape(-1, 1, D * D), lam.reshape(-1, 1, D * D), o.expand(N * H * W, D * D, 2), delta.reshape(-1, 1, 2)).reshape(N, H, W, 2)
    s_abs = torch.matmul(p, o.abs())
    if body:
        J = D * D
        ab = torch.stack([(p * torch.stack([(X + dx).abs() for dx, _ in offs], -1)).sum(-1), (p * torch.stack([(Y + dy).abs() for _, dy in offs], -1)).sum(-1)], -1)
        tol = tol + (2 * J + 3) * U * ab + U * delta.abs()
    else:
        tol = tol + (2 * (LM_STEPS + 1) + 2) * U * (s_abs + delta.abs())
    tol = tol + TINY * (o.abs().sum(0) + D * D * delta.abs())
    want = delta if mut == "prior flow not added" else prior + delta
    tol = tol + U * want.abs()
    return want, tol, p, o, delta, t > -1e8


def local_match_inputs(P):
    """noise: N(0, 1) * gain.  pos: [0.5, 1].  planted: f1 = N(0, 1) * gain (3), f0[y, x] = f1[y + dy, x + dx] where that is inside the image (noise
    elsewhere): the matching offset is the planted (dx, dy)."""
    g = _g(P.seed)
    N, H, W = P.N, P.H, P.W
    if P.kind == "pos":
        f0, f1 = 0.5 + 0.5 * torch.rand(N, H, W, 128, generator=g), 0.5 + 0.5 * torch.rand(N, H, W, 128, generator=g)
    else:
        s = P.gain if hasattr(P, "gain") else 1.0
        f0, f1 = torch.randn(N, H, W, 128, generator=g) * s, torch.randn(N, H, W, 128, generator=g) * s
    if P.kind == "planted":
        dx, dy = P.d
        sh = _shifted(f1, dy, dx, NAN)
        f0 = torch.where(torch.isnan(sh), f0, sh)
    prior = torch.randn(N, H, W, 2, generator=g) * 3
    return f0, f1, prior


def planted_inside(P):
    """pixels whose planted partner lies inside the image"""
    dx, dy = P.d
    return _shifted(torch.ones(P.N, P.H, P.W), dy, dx, 0.0) > 0


def op_local_match(P, B):
    """vfi_local_match, C 128, radius 4: local_match_f64's docstring holds the count.  The per-pixel body runs instead of the matrix-core
    kernel on the host build and where f1 is not 16-byte aligned; then its terms are the ones taken."""
    f0, f1, prior = local_match_inputs(P)
    body = bool(getattr(P, "host", False)) or P.f1_off % 4 != 0
    B.add("f0", f0.reshape(-1, 128), cs=136, off=4)
    B.add("f1", f1.reshape(-1, 128), cs=136, off=P.f1_off)
    B.add("flow", prior.reshape(-1, 2), cs=4, off=1, role="inout")
    mut = getattr(P, "mut", None)
    want, tol, p, o, delta, live = local_match_f64(f0.double(), f1.double(), prior.double(), 4, body, mut)
    mn = None
    if P.kind == "pos" and mut is None:
        J = p.shape[-1]
        tl = (tol - U * want.abs()).reshape(-1, 1, 2)
        mn = summand_floor(p.reshape(-1, 1, J), o.expand(p.numel() // J, J, 2), delta.reshape(-1, 1, 2), tl, live.reshape(-1, 1, J)).reshape(want.shape) + U * want.abs()
    args = [B.ptr("f0"), 136, B.ptr("f1"), 136, B.ptr("flow"), 4, P.N, P.H, P.W, 128, 4]
    return [("vfi_local_match", args)], [dict(buf="flow", want=want, tol=tol, mn=mn)]


# ---------------------------------------------------------------------------------------------------------------- local propagate

def local_prop_f64(q, k, flow, mut=None):
    """out = sum_j softmax_j(q . k(pixel + o_j) / sqrt(C)) flow(pixel + o_j) over the 3 x 3 window; taps outside the image score exactly 0,
    carry flow 0 and take part in the softmax (unfold's zero padding, :745-803).  q, k [N, H, W, C], flow [N, H, W, 2].
    Logit: (C + 2) U sum_c |q_c k_c| / sqrt(C) (C products and sums in some association, the root, the division), exactly 0 for a padded
    tap.  Weight: the maximum subtracted (U times the argument), one expf.  Not shared: the sum of nine (8) and the division on the
    normalising side: 9 U |out|; the product and nine additions on the value side: 10 U sum p |flow|."""
    N, H, W, Cc = q.shape
    scale = math.sqrt(Cc)
    ones = torch.ones(N, H, W, dtype=torch.float64)
    t, eps, fl, ins = [], [], [], []
    for j in range(9):
        dx, dy = j % 3 - 1, j // 3 - 1
        kk = _shifted(k, dy, dx, 0.0)
        t.append((q * kk).sum(-1) / scale)
        eps.append((Cc + 2) * U * (q.abs() * kk.abs()).sum(-1) / scale)
        inside = _shifted(ones, dy, dx, 0.0) > 0
        f = _shifted(flow, dy, dx, 0.0)
        if mut == "padded taps carry the clamped flow":
            f = torch.where(inside.unsqueeze(-1), f, flow)
        fl.append(f)
        ins.append(inside)
    t, eps, fl, ins = torch.stack(t, -1), torch.stack(eps, -1), torch.stack(fl, -2), torch.stack(ins, -1)     # [N,H,W,9], [N,H,W,9,2]
    if mut == "padded taps excluded":
        t = torch.where(ins, t, torch.full_like(t, -INF))
    p = torch.softmax(t, -1)
    out = (p.unsqueeze(-1) * fl).sum(-2)
    M = t.amax(-1, keepdim=True)
    gap = torch.where(torch.isinf(t), torch.zeros_like(t), M - t) + 2 * eps.amax(-1, keepdim=True)
    lam = eps + U * gap + 2 * E_EXP * U
    flat = lambda a, *s: a.reshape(-1, *s)
    tol = weighted_bound(flat(p, 1, 9), flat(lam, 1, 9), flat(fl, 9, 2), flat(out, 1, 2)).reshape(out.shape)
    s_abs = (p.unsqueeze(-1) * fl.abs()).sum(-2)
    tol = tol + U * (10 * s_abs + 9 * out.abs()) + TINY * (fl.abs().sum(-2) + 9 * out.abs())
    return out, tol, p, fl


def op_local_propagate(P, B):
    """vfi_local_propagate, C 128, radius 1: local_prop_f64's docstring holds the count (the cooperative kernel and the body share it)."""
    g = _g(P.seed)
    mk = (lambda c: 0.5 + 0.5 * torch.rand(P.N, P.H, P.W, c, generator=g)) if P.kind == "pos" else (lambda c: torch.randn(P.N, P.H, P.W, c, generator=g) * (P.gain if hasattr(P, "gain") else 1.0))
    q, k, flow = mk(128), mk(128), mk(2) * 3
    B.add("q", q.reshape(-1, 128), cs=136, off=4)
    B.add("k", k.reshape(-1, 128), cs=132, off=4)
    B.add("flow", flow.reshape(-1, 2), cs=5, off=3)
    B.add("out", None, P.N * P.H * P.W, 2, 4, 1, role="out")
    mut = getattr(P, "mut", None)
    want, tol, p, fl = local_prop_f64(q.double(), k.double(), flow.double(), mut)
    mn = None
    if P.kind == "pos" and mut is None:
        mn = summand_floor(p.reshape(-1, 1, 9), fl.reshape(-1, 9, 2), want.reshape(-1, 1, 2), tol.reshape(-1, 1, 2)).reshape(want.shape)
    args = [B.ptr("q"), 136, B.ptr("k"), 132, B.ptr("flow"), 5, B.ptr("out"), 4, P.N, P.H, P.W, 128, 1]
    return [("vfi_local_propagate", args)], [dict(buf="out", want=want, tol=tol, mn=mn)]


# ---------------------------------------------------------------------------------------------------------------- layer norm

def layernorm_f64(x, gamma, beta, add, mut=None):
    """nn.LayerNorm(C), eps 1e-5, biased variance (:479-523), + add.  x [tokens, C] float64.
    mean: C - 1 additions in some association and the division: dm = (C - 1) U mean|x| + U |mean|.  d_c = x_c - mean: a_c = dm + U |d_c|.
    variance: the squares carry 2 |d_c| a_c + a_c^2 and one rounding each, C - 1 additions, the division:
    dv = mean_c(2 |d_c| a_c + a_c^2) + (C + 1) U (var + mean_c(2 |d_c| a_c + a_c^2)).  v = var + eps rounds once; sqrtf and the division once
    each: rstd within rr = 2 U + h (1 + 2 h), h = (dv + U (var + eps)) / (2 (var + eps)) (asserted below 1/4).  Then two products, the
    addition of beta and of `add`: |gamma| rstd (a_c (1 + rr) + |d_c| (rr + 2 U)) + U |y| + U |y + add|.
    All of it stays finite for a constant row: var = 0, a_c = dm, the bound is |gamma| dm / sqrt(eps)."""
    Cn = x.shape[1]
    eps = _f32(1e-5)
    mean = x.mean(1, keepdim=True)
    d = x - mean
    var = (d * d).mean(1, keepdim=True)
    dm = (Cn - 1) * U * x.abs().mean(1, keepdim=True) + U * mean.abs()
    a = dm + U * d.abs()
    sq = (2 * d.abs() * a + a * a).mean(1, keepdim=True)
    dv = sq + (Cn + 1) * U * (var + sq)
    h = (dv + U * (var + eps)) / (2 * (var + eps))
    assert float(h.max()) < 0.25
    rr = 2 * U + h * (1 + 2 * h)
    if mut == "variance over C - 1":
        var = (d * d).sum(1, keepdim=True) / (Cn - 1)
    rstd = 1 / (torch.sqrt(var) + eps) if mut == "eps outside the root" else 1 / torch.sqrt(var + eps)
    ga, be = (beta, gamma) if mut == "gamma and beta exchanged" else (gamma, beta)
    if mut == "add before the affine step":
        y = (d * rstd + add) * ga + be
        full = y
    else:
        y = d * rstd * ga + be
        full = y + add if add is not None else y
    tol = ga.abs() * rstd * (a * (1 + rr) + d.abs() * (rr + 2 * U)) + U * y.abs() + (U * full.abs() if add is not None else 0)
    mn = ga.abs() * rstd * x.abs().amin(1, keepdim=True) / Cn if Cn > 1 else None
    return full, tol, mn


def op_layernorm(P, B):
    """vfi_layernorm / vfi_layernorm_add (P.add: 0 none, 1 in place on `add` with out2 a window, 2 in place with out2 null):
    layernorm_f64's docstring holds the count; the wave kernel (C <= 256) and the body (C = 257) differ only in the association."""
    g = _g(P.seed)
    T, Cn = P.tokens, P.C
    if P.kind == "pos":
        x, gamma, beta = (0.5 + 0.5 * torch.rand(*s, generator=g) for s in ((T, Cn), (Cn,), (Cn,)))
    else:
        x = torch.randn(T, Cn, generator=g) * P.sigma + P.mean
        if P.kind == "const":
            x = x[:, :1].expand(T, Cn).contiguous()
        gamma, beta = torch.randn(Cn, generator=g), torch.randn(Cn, generator=g)
    add = torch.randn(T, Cn, generator=g) if P.add else None
    mut = getattr(P, "mut", None)
    want, tol, mn = layernorm_f64(x.double(), gamma.double(), beta.double(), add.double() if P.add else None, mut)
    mn = mn if P.kind == "pos" and mut is None else None
    B.add("x", x, cs=Cn + 3, off=1)
    B.add("gamma", gamma.view(1, Cn), cs=Cn + 2, off=1)
    B.add("beta", beta.view(1, Cn), cs=Cn + 4, off=3)
    if not P.add:
        B.add("out", None, T, Cn, Cn + 5, 3, role="out")
        return [("vfi_layernorm", [B.ptr("x"), Cn + 3, Cn, T, B.ptr("gamma"), B.ptr("beta"), B.ptr("out"), Cn + 5])], [dict(buf="out", want=want, tol=tol, mn=mn)]
    B.add("add", add, cs=Cn + 1, off=1, role="inout")
    expects = [dict(buf="add", want=want, tol=tol, mn=mn)]
    o2, o2cs = None, 0
    if P.add == 1:
        B.add("out2", None, T, Cn, 2 * Cn + 1, Cn, role="out")
        o2, o2cs = B.ptr("out2"), 2 * Cn + 1
        expects.append(dict(buf="out2", want=want, tol=tol, same_as="add"))
    args = [B.ptr("x"), Cn + 3, Cn, T, B.ptr("gamma"), B.ptr("beta"), B.ptr("add"), Cn + 1, B.ptr("add"), Cn + 1, o2, o2cs]
    return [("vfi_layernorm_add", args)], expects


OPS = {k[3:]: v for k, v in list(globals().items()) if k.startswith("op_")}


# ---------------------------------------------------------------------------------------------------------------- runner

def _rc(rc, name):
    assert rc == 0, f"{name} -> {rc}"


def run_case(lib, case, device="cpu", stream=None, sync=None, check=_rc, mut=None, host=False, results=None):
    """builds the case's buffers on `device`, forces the key split the case asks for (and restores the automatic rule), calls the entry
    point, checks inputs, guards and results.  mut: compare with that wrong restatement.  results: a dict that receives every buffer's
    window as read back.  -> largest err / tol"""
    B = Buffers(device)
    B.keep = []
    P = SimpleNamespace(**case.p, mut=mut, host=host)
    calls, expects = OPS[case.op](P, B)
    forced = case.p.get("ks", 0)
    try:
        if forced:
            check(lib.vfi_test_set_option(b"att_ksplit", forced), "vfi_test_set_option")
        for name, args in calls:
            check(getattr(lib, name)(*args, stream), name)
        if sync is not None:
            sync()
    finally:
        if forced:
            lib.vfi_test_set_option(b"att_ksplit", 0)
    outs = B.finish()
    for kp in B.keep:
        kp.check()
    if results is not None:
        results.update(outs)
    worst = 0.0
    for e in expects:
        r = compare(outs[e["buf"]], e, f"{case.id}:{e['buf']}" + (f" vs '{mut}'" if mut else ""))
        worst = max(worst, r or 0.0)
        if e.get("same_as"):
            assert torch.equal(outs[e["buf"]], outs[e["same_as"]]), f"{case.id}: {e['buf']} is not the copy of {e['same_as']}"
    return worst


def expectation(case, mut=None, host=False):
    """the case's expectations alone (no library): for the CPU checks of conditions and mutations"""
    B = Buffers("cpu")
    B.keep = []
    return OPS[case.op](SimpleNamespace(**case.p, mut=mut, host=host), B)[1]


# ---------------------------------------------------------------------------------------------------------------- case tables

def _att(tag, nb, Lq, Lk, DV, kind, win=1, period=0, lab="", ks=0, ks_ran=1, reseed=0, **kw):
    return Case("attention", tag, seed=1000 * nb + 10 * Lq + Lk + DV + 100000 * reseed, nb=nb, Lq=Lq, Lk=Lk, DV=DV, kind=kind, win=win, period=period, lab=lab, ks=ks, ks_ran=ks_ran, **kw)


ATT_CASES = []
_kinds = ("planted", "pos", "noise", "peaky", "pos", "planted", "noise")
for (nb, Lq, Lk), kind in zip(((1, 1, 1), (1, 1, 33), (2, 31, 32), (1, 33, 31), (1, 128, 64), (1, 129, 65), (3, 130, 97)), _kinds):
    ATT_CASES.append(_att(f"dv128-{nb}x{Lq}x{Lk}-{kind}", nb, Lq, Lk, 128, kind))
ATT_CASES.append(_att("dv128-3x130x97-peaky", 3, 130, 97, 128, "peaky"))
ATT_CASES.append(_att("dv128-2x31x32-dense-noise", 2, 31, 32, 128, "noise", win=0))
for DV, kind in ((1, "planted"), (2, "pos"), (3, "noise"), (31, "pos"), (32, "planted")):
    ATT_CASES.append(_att(f"dv{DV}-2x33x65-rows-unaligned-{kind}", 2, 33, 65, DV, kind, win=0))
    ATT_CASES.append(_att(f"dv{DV}-1x129x33-cs{DV + 3}-off1-{kind}", 1, 129, 33, DV, kind, win=1))
# labels: period 1, 3, 4 with nb a multiple of the period and greater; a lone class (one-hot row through the masks); a class in the tail
for DV in (128, 2):
    for period, nb in ((1, 2), (3, 6), (4, 8)):
        ATT_CASES.append(_att(f"dv{DV}-labels-period{period}-nb{nb}-40x40-lone-tail-pos", nb, 40, 40, DV, "pos", period=period, lab="lone tail"))
    ATT_CASES.append(_att(f"dv{DV}-labels-period3-nb6-67x67-lone-tail-noise", 6, 67, 67, DV, "noise", period=3, lab="lone tail"))
# key split forced (option att_ksplit): 8 blocks; 9 blocks where 8 becomes 5; two blocks with one real key in the second
for DV in (128, 2):
    for period in (0, 2):
        lb = dict(period=period, lab="lone tail") if period else {}
        sq = lambda Lk: Lk if period else 129               # labels need Lq == Lk
        for ks in (2, 3, 7, 8):
            Lk = {2: 225, 3: 240, 7: 255, 8: 256}[ks]
            ran = split_rule(Lk, ks)[0]
            kind = {2: "planted", 3: "pos", 7: "noise", 8: "planted"}[ks] if not period else {2: "pos", 3: "noise", 7: "pos", 8: "noise"}[ks]
            ATT_CASES.append(_att(f"dv{DV}-split{ks}-runs{ran}-2x{sq(Lk)}x{Lk}{'-labels' if period else ''}-{kind}", 2, sq(Lk), Lk, DV, kind, ks=ks, ks_ran=ran, **lb))
        ATT_CASES.append(_att(f"dv{DV}-split8-runs5-2x{sq(257)}x257{'-labels' if period else ''}-pos", 2, sq(257), 257, DV, "pos", ks=8, ks_ran=split_rule(257, 8)[0],
                              reseed=2 if DV == 2 and not period else 0, **lb))       # (reseed: the first seeds leave a key within the bound of the 2-channel mean)
        ATT_CASES.append(_att(f"dv{DV}-split2-runs2-onekey-2x{sq(33)}x33{'-labels' if period else ''}-planted", 2, sq(33), 33, DV, "noise" if period else "planted", ks=2, ks_ran=2, **lb))
    ATT_CASES.append(_att(f"dv{DV}-split8-runs8-2x1x256-planted", 2, 1, 256, DV, "planted", ks=8, ks_ran=8))
    ATT_CASES.append(_att(f"dv{DV}-split7-runs7-2x129x224-noise", 2, 129, 224, DV, "noise", ks=7, ks_ran=split_rule(224, 7)[0]))      # 7 blocks: the one length class where 7 ranges survive the rule
    ATT_CASES.append(_att(f"dv{DV}-split-automatic-runs2-1x5x512-planted", 1, 5, 512, DV, "planted", ks=0, ks_ran=2))


def _wa(tag, B, h, w, K, sh, sw, kind, win=1, **kw):
    return Case("window_attention", f"{B}x{h}x{w}-k{K}-shift{sh}x{sw}-{tag}", seed=h * 100 + w + K, B=B, h=h, w=w, K=K, sh=sh, sw=sw, kind=kind, win=win, **kw)


WINDOW_SHAPES = ((1, 2, 2, 1, 0, 0), (1, 4, 6, 2, 1, 1), (2, 6, 10, 2, 1, 2), (1, 12, 20, 4, 1, 2), (1, 18, 34, 2, 4, 8), (1, 6, 10, 1, 2, 3))
WIN_CASES = [_wa(kind, *s, kind) for s, kind in zip(WINDOW_SHAPES, ("noise", "pos", "noise", "pos", "noise", "pos"))]
WIN_CASES.append(_wa("dense-noise", 2, 6, 10, 2, 1, 2, "noise", win=0))
WIN_CASES.append(_wa("unshifted-peaky", 2, 6, 10, 2, 0, 0, "peaky", gain=6.0))


def _lm(tag, N, H, W, kind, f1_off=4, reseed=0, **kw):
    return Case("local_match", f"{N}x{H}x{W}-{tag}", seed=H * 100 + W + 100000 * reseed, N=N, H=H, W=W, kind=kind, f1_off=f1_off, **kw)


LM_SHAPES = ((1, 2, 2), (1, 4, 8), (1, 5, 9), (1, 3, 17), (2, 9, 6))
LM_CASES = [_lm(kind, *s, kind, reseed=4 if s == (1, 3, 17) else 0) for s, kind in zip(LM_SHAPES, ("noise", "pos", "noise", "pos", "noise"))]     # (reseed: as above, a tap at the mean)
LM_CASES += [_lm("noise-f1-off1", 1, 5, 9, "noise", f1_off=1), _lm("gain3", 2, 9, 6, "noise", gain=3.0)]
LM_CASES += [_lm(f"planted-dx{dx}-dy{dy}", *s, "planted", d=(dx, dy), gain=3.0) for s, (dx, dy) in (((1, 5, 9), (2, -1)), ((2, 9, 6), (-3, 4)), ((1, 3, 17), (4, 1)), ((1, 4, 8), (-1, 2)))]
LM_CASES += [_lm("planted-dx2-dy-1-f1-off1", 1, 5, 9, "planted", d=(2, -1), f1_off=1, gain=3.0)]

LP_CASES = [Case("local_propagate", f"{N}x{H}x{W}-{kind}", seed=H * 10 + W, N=N, H=H, W=W, kind=kind)
            for (N, H, W), kind in zip(((1, 1, 1), (1, 1, 5), (1, 3, 1), (1, 2, 2), (2, 5, 7)), ("noise", "pos", "noise", "pos", "noise"))]
LP_CASES += [Case("local_propagate", "2x5x7-pos", seed=58, N=2, H=5, W=7, kind="pos"), Case("local_propagate", "2x5x7-gain3", seed=59, N=2, H=5, W=7, kind="noise", gain=3.0)]


def _ln(tag, C_, tokens, kind="noise", add=0, mean=0.3, sigma=1.0):
    return Case("layernorm", f"C{C_}-tokens{tokens}-{tag}", seed=C_ + tokens + add, C=C_, tokens=tokens, kind=kind, add=add, mean=mean, sigma=sigma)


LN_CASES = [_ln(f"{kind}{('-add-out2', '-add')[add - 1] if add else ''}", C_, tokens, kind, add)
            for (C_, tokens), kind, add in zip(((1, 3), (64, 1), (65, 5), (96, 4), (128, 37), (256, 3), (257, 5)), ("noise", "pos", "noise", "pos", "noise", "pos", "noise"), (0, 1, 2, 0, 1, 2, 1))]
LN_CASES += [_ln("noise", 128, 4), _ln("pos-add-out2", 65, 37, "pos", 1), _ln("const-row", 128, 5, "const"), _ln("const-row-add-out2", 65, 3, "const", 1), _ln("const-row", 1, 4, "const"),
             _ln("const-row-body", 257, 3, "const"), _ln("mean1000-sigma1", 128, 5, mean=1000.0), _ln("mean1000-sigma1-add", 256, 4, add=2, mean=1000.0),
             _ln("mean1000-sigma1-body-add-out2", 257, 1, add=1, mean=1000.0)]

ALL_CASES = ATT_CASES + WIN_CASES + LM_CASES + LP_CASES + LN_CASES
HOST_CASES = LM_CASES + LP_CASES + LN_CASES         # entry points the host build of the bodies exports


# ---------------------------------------------------------------------------------------------------------------- wrong restatements

def _applies(case, mut):
    p = case.p
    if case.op == "attention":
        return {
            "last key dropped": p["Lk"] > 1 and p["kind"] in ("pos", "noise"),
            "key 31 dropped": p["Lk"] >= 32 and p["kind"] in ("pos", "noise"),
            "key 32 dropped": p["Lk"] >= 33 and p["kind"] in ("pos", "noise"),
            "padding keys counted": p["Lk"] % KB != 0 and (p["kind"] in ("pos", "noise") or p["kind"] == "planted" and p["Lq"] > 1),      # (planted: the all -300 row is query 1)
            "alpha omitted": p["Lk"] > 1 and p["kind"] in ("pos", "noise", "peaky"),
            "mask where equal": bool(p["period"]),
            "label row b": p["nb"] > p["period"] > 1,
            "softmax over queries": p["Lq"] > 1 and p["Lk"] > 1 and p["kind"] in ("pos", "noise"),
            "value channels exchanged": p["DV"] >= 12,
            "merge without rescale": p["ks_ran"] > 1 and p["kind"] in ("noise", "planted"),
        }[mut]
    if case.op == "window_attention":
        shifted = bool(p["sh"] or p["sw"])
        return {"roll with the opposite sign": shifted, "roll not undone": shifted, "wy and wx exchanged": shifted and p["K"] > 1,
                "image from the wrong quotient": p["B"] > 1 and p["K"] > 1}[mut]
    if case.op == "local_match":
        big = p["H"] * p["W"] > 4
        return {"dx and dy exchanged": True, "offsets column-major": True, "outside scored 0": True, "radius 3": big and p["kind"] != "planted" or p["kind"] == "planted" and 4 in map(abs, p["d"]),
                "prior flow not added": True}[mut]
    if case.op == "local_propagate":
        return True
    if case.op == "layernorm":
        # a constant row has d = 0: its output is beta whatever the variance; mean 1000 has a bound of 1e-2 |y|, wider than 1 / (2 C)
        return {"variance over C - 1": p["C"] > 1 and p["kind"] != "const" and p["mean"] < 100, "eps outside the root": p["kind"] == "pos" and p["C"] <= 128,      # (sigma 0.14: the two differ by 2e-4 |y|; at C = 256 the bound is as wide)
                "gamma and beta exchanged": True, "add before the affine step": bool(p["add"])}[mut]
    raise KeyError(case.op)


MUTATIONS = {
    "attention": ("last key dropped", "key 31 dropped", "key 32 dropped", "padding keys counted", "alpha omitted", "mask where equal", "label row b", "softmax over queries",
                  "value channels exchanged", "merge without rescale"),
    "window_attention": ("roll with the opposite sign", "roll not undone", "wy and wx exchanged", "image from the wrong quotient"),
    "local_match": ("dx and dy exchanged", "offsets column-major", "outside scored 0", "radius 3", "prior flow not added"),
    "local_propagate": ("padded taps excluded", "padded taps carry the clamped flow"),
    "layernorm": ("variance over C - 1", "eps outside the root", "gamma and beta exchanged", "add before the affine step"),
}
NEGATIVE = [(c, m) for c in ALL_CASES for m in MUTATIONS[c.op] if _applies(c, m)]
