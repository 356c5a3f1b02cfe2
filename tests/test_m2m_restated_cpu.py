"""No device: the float64 restatements of tests/m2m_restated.py against the oracle (oracle/m2m_oracle.py: the plain-C splat pinned to the
reference's kernel text; oracle/m2m_model_oracle.py: backwarp, the cube product, forwarp_mframe_mask; the photometric, splat-input and
normalisation expressions of m2m_forward :193-235 restated line by line) evaluated in fp32, within the SAME bounds the device is held to —
so a restatement that drifts from the reference fails here, and a bound that fp32 arithmetic cannot keep shows up before a GPU is involved.
Also, from the restatement alone: the share of pixels left out at the hole threshold (<= 1 %), the branch conditions every case is in the
table for (window > RCAP, cell > RK, cells of 3..6, hole counts, far flows), `mn > tol` (inside compare), and that every mutation is
rejected.  pool_mean and normalize are compared with the reference expression evaluated in float64 and rounded once: torch's fp32 mean of
a mean-1000 input carries its own summation error, which is not what the bound is about."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import m2m_restated as mr
from oracle import m2m_model_oracle as MO
from oracle import m2m_oracle as M


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _backwarp(img, fl, swap):
    """the oracle's backwarp; a non-finite flow (every tap dropped by the kernels, never produced by the reference) is sent far outside"""
    N = img.shape[0]
    src = img.view(N // 2, 2, *img.shape[1:]).flip(1).reshape(img.shape) if swap else img
    f = torch.where(torch.isfinite(fl), fl, torch.full_like(fl, 1e6)).clamp(-1e6, 1e6)
    return _nhwc(MO.backwarp(_nchw(src), _nchw(f)))


def _splat(a, f):
    return torch.from_numpy(M.softsplat_sum(_nchw(a).numpy(), _nchw(f).numpy())).permute(0, 2, 3, 1).contiguous()


def _photo(P, ins):
    d0, r = ins["d0"], ins["r"]
    alpha = torch.tensor(P.alpha, dtype=torch.float32)
    H, W = P.H, P.W
    tf, E = torch.empty(8, H, W, 2), torch.empty(8, H, W)
    img = d0[..., 2:5].contiguous()
    wei = torch.sigmoid(r[..., 8]) * 0.8 + 0.1
    for s in range(8):
        d, b = s & 1, s >> 1
        tf[s] = d0[d, :, :, 0:2] + r[d, :, :, 2 * b:2 * b + 2]
        w = _backwarp(img, torch.stack([tf[s], tf[s]]), 1)[d]
        photo = (1.0 - (wei[d] * (img[d] - w).abs().mean(-1))).clip(0.001, None).square()
        E[s] = (alpha * photo).clip(-20.0, 20.0).exp()
    outs = dict(tf=tf.reshape(-1, 2), e=E.reshape(-1, 1))
    if P.tiles:
        rg, sm = mr.tile_ranges(tf.numpy())
        outs.update(tf2=outs["tf"], e2=outs["e"], ranges=torch.from_numpy(rg).reshape(-1, 4), smax=torch.from_numpy(sm).reshape(8, 1))
    return outs


def _render(P, ins):
    d0, tf, e, stats = ins["d0"], ins["tf"], ins["e"], ins["stats"]
    t = torch.tensor(P.t, dtype=torch.float32)
    t1 = 1.0 - t
    im = [_nchw(d0[d:d + 1, :, :, 2:5]) for d in (0, 1)]
    fl = lambda k, tm: [_nchw((tf[2 * b + k] * tm)[None]) for b in range(4)]         # noqa: E731

    def one(ten_in, flow, td, ee):          # forwarp_mframe_mask's one_fdir on e = exp(clip(metric)) itself, through the oracle's splat
        x = torch.cat([ten_in * td * ee, td * ee], 1)
        o = MO.softsplat(x.contiguous(), flow.contiguous())
        return o[:, :-1], o[:, -1:] + 0.0000001
    out, norm = 0, 0
    for b in range(4):
        of, nf = one(im[0], fl(0, t)[b], t1, e[2 * b][None, None])
        ob, nb = one(im[1], fl(1, t1)[b], t, e[2 * b + 1][None, None])
        out += of + ob
        norm += nf + nb
    mask = norm < 0.00001
    out = out / norm + mask * (t1 * im[0] + t * im[1])
    out = out * stats[1] + stats[0]
    return dict(out=_nhwc(out)[0, :P.H, :P.W].reshape(-1, 3))


def _splat_inputs(P, ins):
    d0, tf, e = ins["d0"], ins["tf"], ins["e"]
    t = torch.tensor(P.t, dtype=torch.float32)
    t1 = 1.0 - t
    sin, sfl = torch.empty(8, P.Hp, P.Wp, 4), torch.empty(8, P.Hp, P.Wp, 2)
    for s in range(8):
        td, tm = (t1, t) if s % 2 == 0 else (t, t1)
        ee = e[s].unsqueeze(-1)
        sin[s] = torch.cat([d0[s & 1, :, :, 2:5] * td * ee, td * ee], -1)
        sfl[s] = tf[s] * tm
    return dict(sin=sin.reshape(-1, 4), sfl=sfl.reshape(-1, 2))


def _combine(P, ins):
    d0, sp, stats = ins["d0"].numpy(), ins["sp"].numpy(), ins["stats"].numpy()
    t = np.float32(P.t)
    t1 = np.float32(1.0) - t
    acc, norm = np.zeros((P.Hp, P.Wp, 3), np.float32), np.zeros((P.Hp, P.Wp), np.float32)
    for b in range(4):
        acc = acc + (sp[2 * b, :, :, :3] + sp[2 * b + 1, :, :, :3])
        norm = norm + ((sp[2 * b, :, :, 3] + np.float32(1e-7)) + (sp[2 * b + 1, :, :, 3] + np.float32(1e-7)))
    v = acc / norm[..., None]
    v = v + (norm < np.float32(0.00001))[..., None] * (t1 * d0[0, :, :, 2:5] + t * d0[1, :, :, 2:5])
    out = v * stats[1] + stats[0]
    return dict(out=torch.from_numpy(np.ascontiguousarray(out[:P.H, :P.W])).reshape(-1, 3))


def _cube(P, ins):
    s3, cC, cH, cW = ins["s3"], ins["cC"], ins["cH"], ins["cW"]
    N = P.N
    c = cC.view(N, 16, P.C, 1, 1)
    h = cH.permute(0, 2, 1).reshape(N, 16, 1, P.H, 1)
    w = cW.permute(0, 2, 1).reshape(N, 16, 1, 1, P.W)
    return dict(out=_nhwc(_nchw(s3) * (c * h * w).mean(1)).reshape(-1, P.C))


def _pool(P, ins):
    size = {0: 1, 1: (None, 1), 2: (1, None)}[P.mode]
    return dict(out=_nhwc(F.adaptive_avg_pool2d(_nchw(ins["x"].double()), size)).float().reshape(-1, P.C))


def _normalize(P, ins):
    f = ins["f"][..., :3].double()
    im = [F.pad(_nchw(f[k:k + 1]), [0, P.Wp - P.W, 0, P.Hp - P.H], mode="replicate") for k in (0, 1)]
    mean_ = sum(t.mean([1, 2, 3], True) for t in im) / 2
    std_ = (sum(t.std([1, 2, 3], False, True).square() + (mean_ - t.mean([1, 2, 3], True)).square() for t in im) / 2).sqrt()
    sd = std_ + float(np.float32(1e-7))
    out = torch.cat([_nhwc((t - mean_) / sd) for t in im]).float()
    return dict(stats=torch.stack([mean_.reshape(()), sd.reshape(())]).float().view(1, 2), out=out.reshape(-1, 3))


ORACLES = dict(
    warp_m2m=lambda P, ins: dict(out=_backwarp(ins["img"], ins["fl"], P.swap).reshape(-1, P.C)),
    warp_image4=lambda P, ins: dict(out=_backwarp(ins["img"], ins["fl"], 1).reshape(-1, 3)),
    photo=_photo, softsplat=lambda P, ins: dict(out=_splat(ins["a"], ins["f"]).reshape(1, -1)), render=_render, splat_inputs=_splat_inputs,
    combine=_combine, cube_apply=_cube, pool_mean=_pool, normalize=_normalize)

_SEEN = {}


def _oracle_outs(case):
    """the oracle's result for a case's inputs, computed once (a mutated case has the same inputs as the case it was made from)"""
    from types import SimpleNamespace

    key = case.id[:-4] if case.id.endswith("-mut") else case.id
    if key not in _SEEN:
        _, _, _, ins, _ = mr.build(mr._by_id[key])
        _SEEN[key] = ORACLES[case.op](SimpleNamespace(**case.p), ins)
    return _SEEN[key]


def _cpu_cases():
    """every case once per (inputs, restatement): the A/B options of a splat case and the form of a render change neither"""
    seen, out = set(), []
    for c in mr.ALL_CASES:
        p = {k: v for k, v in c.p.items() if k not in ("opts", "form")}
        key = (c.op, repr(sorted(p.items())))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("case", _cpu_cases(), ids=lambda c: c.id)
def test_restatement_holds_the_oracle(case):
    _, _, expects, _, info = mr.build(case)
    outs = _oracle_outs(case)
    mr.check(outs, [e for e in expects if e["buf"] in outs], case.id)
    i = case.id
    if case.op == "render":
        assert info["left_out"] <= 0.01
        if "huge" in i:
            assert info["ranges_span_image"], "a block's range does not span the image: the window is not the whole image"
        if "noise8" in i:
            assert info["win_max"] > mr.RCAP, f"the largest window holds {info['win_max']} sources: one strip"
        if "smooth" in i or "translate" in i:
            assert info["win_max"] <= mr.RCAP, "meant to be a single strip"
        if "zoom" in i or "point" in i:
            assert info["cnt_max"] > mr.RK, "no cell overflows: the scan does not run"
        if "wavy" in i or "noise8" in i:
            assert info["cnt36"], "no cell of 3..6 sources: the sort does not run"
        if "hole" in i:
            assert info["holes"] >= 32 and info["solid"] >= 32, info
    if case.op == "combine":
        assert info["holes"] >= 32 and info["solid"] >= 32 and info["at_threshold"] >= 8, info
    if case.op == "softsplat":
        f = case.p["field"]
        if f == "zoom":
            assert info["cnt_max"] > 16
        if f == "zoom8":
            assert 6 < info["cnt_max"] <= 16
        if f == "point":
            assert info["cnt_max"] > 16
        if f == "far":
            assert 64 < info["fmax"] <= 150.5
            assert info["far_arrivals"] >= 300, f"only {info['far_arrivals']} pixels receive more than their tolerance from a source displaced by more than 64 px"
        if f == "near64":
            assert info["far_arrivals"] >= 300, info
        if f == "near64":
            assert 63 < info["fmax"] < 64
    if case.op == "normalize" and case.p["const"] is None:
        assert info["tsd_rel"] < 1e-5, f"tol(sd) / sd = {info['tsd_rel']:.2e}: the variance bound has lost the cancellation it is there to catch"
    if case.op == "photo":
        if "floor" in i or i in ("photo-37x45-vec-partial", "photo-64x96-vec-d0cs6"):
            assert info["floored_tight"] >= 32 and info["floored_tight"] == info["floored"], info          # floored pixels, each with tol < 1e-4 E
        if "clip20" in i:
            assert info["clip"] >= 32


@pytest.mark.parametrize("case,what", mr.MUTATIONS, ids=lambda v: v.id if isinstance(v, mr.Case) else v)
def test_mutation_is_visible_against_the_oracle(case, what):
    _, _, expects, _, _ = mr.build(case)
    outs = _oracle_outs(case)
    with pytest.raises(AssertionError, match="outside the bound|differ from the exact result"):
        mr.check(outs, [e for e in expects if e["buf"] in outs], case.id)


def test_at_least_twelve_mutations_each_with_a_case():
    kinds = {m for _, m in mr.MUTATIONS}
    assert len(kinds) >= 12
    assert {"drop7th", "edge_column", "swap_ne_sw", "td_tm", "no_c7", "hole_le", "no_fill", "wei_no_01", "no_floor", "no_clip", "noswap", "border", "ranges_all", "sclx_both"} <= kinds


def test_tile_ranges_use_ceil_tile_counts():
    tf = np.zeros((8, 37, 45, 2), np.float32)
    tf[3, 36, 44] = (5.0, -7.0)
    tf[3, 35, 44] = (np.nan, 100.0)
    rg, sm = mr.tile_ranges(tf)
    assert rg.shape == (8, 4, 4) and tuple(rg[3, 3]) == (0.0, 5.0, -7.0, 0.0) and sm[3] == 7.0 and sm[0] == 0.0


def test_restatements_hold_the_aux_tensors_of_m2m_forward():
    """tf, wei, the statistics and the frame of the oracle's own M2M_PWC.forward (m2m_forward(return_aux=True), synthetic weights, a 64x64 pair,
    t = 0.25): tf = flow + residual bit for bit in the s = 2 b + d order; the frame within the render bound at E = the photo restatement
    at the oracle's wei (its logit recovered in float64), plus what E's own bound does to a weighted mean: relative errors d_src of the weights
    move acc / norm by at most 2 sum_src d_src |in k| / norm (first order)."""
    from cfi_amd import synth

    sd = synth.m2m_synth_state_dict(1234)
    fr = synth.smooth_frames(2, 64, 64, seed=2, shift=2.0)
    x = fr.permute(0, 3, 1, 2).contiguous()
    t = 0.25
    outs, aux = MO.m2m_forward(sd, x[0:1], x[1:2], [torch.full((1, 1, 1, 1), t)], return_aux=True)
    H = W = 64
    mean, sdev = aux["mean"].reshape(()), (aux["std"] + 0.0000001).reshape(())
    im = [(x[k:k + 1] - aux["mean"]) / (aux["std"] + 0.0000001) for k in (0, 1)]
    flow = [4 * F.interpolate(aux[k], scale_factor=4, mode="bilinear", align_corners=False) for k in ("fwd", "bwd")]
    res, wei = aux["res"][0:2], aux["res"][2:4]
    d0 = torch.zeros(2, H, W, 8)
    for d in (0, 1):
        d0[d, :, :, 0:2], d0[d, :, :, 2:5] = _nhwc(flow[d])[0], _nhwc(im[d])[0]
    # tf as op_photo forms it: numpy.float32 addition, splat s = 2 b + d
    d0n, rn = d0.numpy(), [_nhwc(r)[0].numpy() for r in res]
    tf = torch.from_numpy(np.stack([d0n[s & 1, :, :, 0:2] + rn[s & 1][:, :, 2 * (s >> 1):2 * (s >> 1) + 2] for s in range(8)]).astype(np.float32))
    ten = [aux["ten_fwd"], aux["ten_bwd"]]
    want_tf = torch.stack([_nhwc(ten[s & 1][:, 2 * (s >> 1):2 * (s >> 1) + 2])[0] for s in range(8)])
    mr.compare_bits(tf, want_tf, "tf vs aux ten_fwd / ten_bwd")
    # E from the restatement at the oracle's wei
    w64 = torch.stack([wei[d][0, 0].double() for d in (0, 1)])
    sig = (w64 - mr.C01) / mr.C08
    logit = torch.log(sig / (1 - sig))
    alpha = float(sd["paramAlpha"].reshape(-1)[0])
    E, tE = mr.photo64(d0[..., 2:5].contiguous(), tf, logit, alpha)
    r = mr.render64(d0, tf, E.float(), torch.stack([mean, sdev]), t, H, W)
    t32, t1 = mr._t_pair(t)
    moved = torch.zeros(H, W, 3, dtype=torch.float64)          # sum over the sources of (relative bound of its E) |in k|, per output pixel
    for s_ in range(8):
        td, tm = (t1, t32) if s_ % 2 == 0 else (t32, t1)
        dl = (tE[s_] / E[s_] + mr.U).unsqueeze(-1)
        inp = (d0[s_ & 1, :, :, 2:5].double() * td * E[s_].unsqueeze(-1)).abs() * dl
        moved += mr.splat64(inp[None], (tf[s_].double() * tm)[None], mr.R_RENDER, mr.C_RENDER)["want"][0]
    norm = torch.stack([q["want"][0][..., 3] for q in r["res"]]).sum(0) + 8 * mr.C7
    extra = 2 * moved / norm.unsqueeze(-1) * float(sdev)
    assert 1.0 - float(r["sure"].double().mean()) <= 0.01
    got = _nhwc(outs[0])[0]
    ratio = mr.compare(got, dict(want=r["want"], tol=r["tol"] + extra, where=r["where"]), "frame vs m2m_forward")
    assert ratio is not None
