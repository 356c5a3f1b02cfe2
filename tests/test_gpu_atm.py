"""-m gpu: the ATM-lite path on the device.

Kernels, each against a float64 evaluation of the same formula on the same float32 operands, within a bound derived from the operand
magnitudes (u = 2^-24; a sum of K products in any order is within (K + 2) u of sum |a||b|, tests/test_gpu_small_ops.py's convention).  Every
case prints max err / bound.

  * vfi_atm_window_attention on the eight token maps of atm_restated.ATTN_CASES, both kinds, with the per-head offsets and, behind them,
    vfi_atm_motion_mlp.  Bound: a score is off by eps_s = (d + 4) u (scale sum |q||k| + 100); a probability by the relative 2 eps_s + (N + 8) u
    (both exponent shifts, expf, the sum, the reciprocal); an output by that times sum p |v| plus the (N + 2) u of its own sum.
  * the strided / dilated convolutions (tap gather: bit-exact; then the 1x1 layer), the k2 s2 transposed convolution at 61 channels, the
    depthwise convolution with GELU, the two synthesis kernels with flows that point outside the image.

Forward: <= 1e-3 per pixel against the reference's goldens (tests/golden/atm_net.npz, atm_node.npz) and against the float32 restatement at
every pixel: 64x64, 128x192, 192x320 directly, 100x180 and one 540x960 pair through the node; both global-motion modes; the same pair twice
gives the same bits; a workspace reused across two shapes gives the frames of a fresh object."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import atm_restated as R
import cain_restated
from gpu_util import ptr

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _ck(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _report(name, err, tol):
    ratio = float((err / tol.clamp_min(1e-300)).max())
    print(f"{name}: max err {float(err.max()):.3e}, max err / bound {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: outside the bound (err / bound {ratio:.3f})"


# ---- the attention kernel ------------------------------------------------------------------------------------------------------------

def _qkv_maps(name, cross):
    """float32 q, k, v token maps [2 h w + 1, C] (the last token is the pad token: norm1 of zeros, projected) as the network makes them"""
    p, x = R.attn_case(name, cross)
    C_ = x.shape[-1]
    tok = torch.cat([x.reshape(-1, C_), torch.zeros(1, C_)])
    xn = F.layer_norm(tok, (C_,), p["norm1.weight"], p["norm1.bias"])
    if cross:
        q, kv = F.linear(xn, p["attn.q.weight"]), F.linear(xn, p["attn.kv.weight"])
        return p, q.contiguous(), kv[:, :C_].contiguous(), kv[:, C_:].contiguous()
    qkv = F.linear(xn, p["attn.qkv.weight"])
    return p, qkv[:, :C_].contiguous(), qkv[:, C_:2 * C_].contiguous(), qkv[:, 2 * C_:].contiguous()


def _attention64(q, k, v, h, w, win, shift, cross):
    """float64 window attention on token maps (the formula of include/vfi_hip.h): -> out [2hw, C], offsets [2hw, 8, 2] and their bounds"""
    C_ = q.shape[1]
    d, N = C_ // 8, win * win
    hp, wp = math.ceil(h / win) * win, math.ceil(w / win) * win
    top, left = (hp - h) // 2, (wp - w) // 2
    idx = torch.full((hp, wp), -1, dtype=torch.long)
    idx[top:top + h, left:left + w] = torch.arange(h * w).reshape(h, w)
    idx = torch.roll(idx, (-shift, -shift), (0, 1))

    def cut(t):
        return t.reshape(hp // win, win, wp // win, win).permute(0, 2, 1, 3).reshape(-1, N)

    widx, lab = cut(idx), cut(R.region_labels(hp, wp, h, w, win, shift))
    mask = (lab[:, :, None] != lab[:, None, :]).double() * -100.0
    i = torch.arange(N)
    kx, ky = (i % win).double(), (i // win).double()
    rel = torch.stack([kx[None, :] - kx[:, None], ky[None, :] - ky[:, None]], -1)      # [query, key, 2]
    q, k, v = q.double(), k.double(), v.double()
    pad = q.shape[0] - 1
    out, offs = torch.zeros(2 * h * w, C_, dtype=torch.float64), torch.zeros(2 * h * w, 8, 2, dtype=torch.float64)
    out_tol, offs_tol = torch.zeros_like(out), torch.zeros_like(offs)
    scale = float(np.float32(1.0 / math.sqrt(d)))
    for f in (0, 1):
        fk = f ^ 1 if cross else f
        gq = torch.where(widx >= 0, widx + f * h * w, torch.full_like(widx, pad))
        gk = torch.where(widx >= 0, widx + fk * h * w, torch.full_like(widx, pad))
        Q, K, V = (t.reshape(-1, N, 8, d).transpose(1, 2) for t in (q[gq], k[gk], v[gk]))          # [windows, 8, N, d]
        s = Q @ K.transpose(-1, -2) * scale + mask[:, None]
        eps_s = ((d + 4) * U * (Q.abs() @ K.abs().transpose(-1, -2) * scale + 100.0)).amax(-1, keepdim=True)
        p = torch.softmax(s, -1)
        rel_p = 2 * eps_s + (N + 8) * U
        o = (p @ V).transpose(1, 2).reshape(-1, N, C_)
        o_tol = ((rel_p + (N + 2) * U) * (p @ V.abs())).transpose(1, 2).reshape(-1, N, C_) + 1e-30
        off = torch.einsum("whqk,qkc->wqhc", p, rel)
        off_tol = ((rel_p + (N + 4) * U) * (win - 1) + 4 * U * (win - 1)).transpose(1, 2).expand(-1, -1, -1, 2)   # [windows, N, 8, 2]
        real = widx >= 0
        out[gq[real]], out_tol[gq[real]] = o[real], o_tol[real]
        offs[gq[real]], offs_tol[gq[real]] = off[real], off_tol[real]
    return out, out_tol, offs, offs_tol


@pytest.mark.parametrize("cross", [True, False], ids=["cross", "self"])
@pytest.mark.parametrize("name", sorted(R.ATTN_CASES))
def test_window_attention_kernel(hip_lib, name, cross):
    h, w, win, shift = R.ATTN_CASES[name]
    p, q, k, v = _qkv_maps(name, cross)
    C_ = q.shape[1]
    ntok = 2 * h * w
    want, tol, woffs, offs_tol = _attention64(q, k, v, h, w, win, shift, cross)
    dq, dk, dv = q.cuda(), k.cuda(), v.cuda()
    outs = []
    for _ in range(2):
        out = torch.full((ntok, C_), float("nan"), device="cuda")
        offs = torch.full((ntok, 8, 2), float("nan"), device="cuda")
        _ck(hip_lib.vfi_atm_window_attention(ptr(dq), C_, ptr(dk), C_, ptr(dv), C_, ntok, ptr(out), C_, ptr(offs) if cross else None, h, w, C_, win,
                                             shift, int(cross), _stream()), "vfi_atm_window_attention")
        torch.cuda.synchronize()
        outs.append((out.cpu(), offs.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]), "two runs, two results"
    got, goffs = outs[0]
    assert torch.isfinite(got).all(), "a real token's row was not written"
    _report(f"attention {name} {'cross' if cross else 'self'}", (got.double() - want).abs(), tol)
    if not cross:
        return
    assert torch.equal(outs[0][1], outs[1][1]) and torch.isfinite(goffs).all()
    _report(f"offsets {name}", (goffs.double() - woffs).abs(), offs_tol)
    assert float(woffs.abs().max()) > 0.5
    # the MLP over the heads, on the device's own offsets
    w0, b0, w2, b2 = (p[f"attn.mlp.{i}.{j}"].contiguous() for i in (0, 2) for j in ("weight", "bias"))
    mot = torch.full((h * w, 4), float("nan"), device="cuda")
    dev = [t.cuda() for t in (goffs, w0, b0, w2, b2)]      # (kept alive until the synchronize)
    _ck(hip_lib.vfi_atm_motion_mlp(*[ptr(t) for t in dev], ptr(mot), 4, 2, h * w, _stream()), "vfi_atm_motion_mlp")
    torch.cuda.synchronize()
    o = goffs.double().transpose(1, 2)                                     # [tokens, 2, 8]
    hid = F.linear(o, w0.double(), b0.double())
    wantm = F.linear(F.gelu(hid), w2.double(), b2.double())[..., 0]        # [tokens, 2]
    hid_tol = 10 * U * (F.linear(o.abs(), w0.double().abs()) + b0.double().abs())
    tolm = F.linear(1.13 * hid_tol + 8 * U * hid.abs(), w2.double().abs()) + 6 * U * (F.linear(F.gelu(hid).abs(), w2.double().abs()) + b2.double().abs())
    gotm = mot.cpu().double().reshape(h * w, 2, 2).transpose(0, 1).reshape(2 * h * w, 2)       # [p][frame][coord] -> [frame p][coord]
    _report(f"motion mlp {name}", (gotm - wantm).abs(), tolm[..., 0])


# ---- the other new kernels -----------------------------------------------------------------------------------------------------------

def _layer(hip_lib, w, b, cout, cin, cin_phys, prelu=None):
    h = hip_lib.vfi_conv_create_ex(0, ptr(w), ptr(b) if b is not None else None, cout, cin, 1, 1, 0, None, cin_phys, ptr(prelu) if prelu is not None else None)
    assert h, "vfi_conv_create_ex failed"
    return h


@pytest.mark.parametrize("c,stride,dil,H,W", [(64, 2, 1, 9, 13), (32, 4, 1, 10, 14), (32, 4, 2, 11, 9), (96, 2, 1, 7, 5)])
def test_strided_dilated_convolution(hip_lib, c, stride, dil, H, W):
    g = torch.Generator().manual_seed(c + stride + dil)
    x = torch.randn((2, H, W, c), generator=g)
    wt, b = torch.randn((c, c, 3, 3), generator=g) / (3 * c ** 0.5), torch.randn((c,), generator=g) * 0.1
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    taps = torch.full((2, Ho, Wo, 9 * c), float("nan"), device="cuda")
    dx = x.cuda()
    _ck(hip_lib.vfi_atm_gather_taps(ptr(dx), c, ptr(taps), 9 * c, 2, H, W, c, stride, dil, _stream()), "vfi_atm_gather_taps")
    xp = F.pad(x.permute(0, 3, 1, 2), (dil, dil, dil, dil))
    wantt = torch.stack([xp[:, :, ky * dil:ky * dil + (Ho - 1) * stride + 1:stride, kx * dil:kx * dil + (Wo - 1) * stride + 1:stride]
                         for ky in range(3) for kx in range(3)], 1)                       # [2, 9, c, Ho, Wo]
    torch.cuda.synchronize()
    assert torch.equal(taps.cpu(), wantt.permute(0, 3, 4, 1, 2).reshape(2, Ho, Wo, 9 * c)), "the gather is a copy: bit for bit"
    w1 = wt.permute(0, 2, 3, 1).reshape(c, 9 * c).contiguous()
    L = _layer(hip_lib, w1, b, c, 9 * c, 9 * c)
    try:
        out = torch.full((2, Ho, Wo, c), float("nan"), device="cuda")
        _ck(hip_lib.vfi_conv_forward_ex(L, ptr(taps), 9 * c, Ho, Wo, ptr(out), c, 2, 0, 0.0, 0.0, 0.0, None, 0, _stream()), "vfi_conv_forward_ex")
        torch.cuda.synchronize()
    finally:
        hip_lib.vfi_conv_destroy(L)
    xd = x.double().permute(0, 3, 1, 2)
    want = F.conv2d(xd, wt.double(), b.double(), stride=stride, padding=dil, dilation=dil)
    assert want.shape[2:] == (Ho, Wo)
    tol = (9 * c + 2) * U * (F.conv2d(xd.abs(), wt.double().abs(), b.double().abs(), stride=stride, padding=dil, dilation=dil))
    _report(f"conv c{c} s{stride} d{dil} {H}x{W}", (out.cpu().double().permute(0, 3, 1, 2) - want).abs(), tol)


def test_transposed_convolution_k2s2_at_61_channels(hip_lib):
    cin, c, H, W = 117, 61, 5, 7
    g = torch.Generator().manual_seed(61)
    x = torch.zeros(1, H, W, 120)
    x[..., :cin] = torch.randn((1, H, W, cin), generator=g)
    wt, b, sl = torch.randn((cin, c, 2, 2), generator=g) / cin ** 0.5, torch.randn((c,), generator=g) * 0.1, torch.rand((c,), generator=g) * 0.5
    w1 = wt.permute(2, 3, 1, 0).reshape(4 * c, cin).contiguous()          # [(2 ky + kx) c + co][ci]
    L = _layer(hip_lib, w1, b.repeat(4), 4 * c, cin, 120, sl.repeat(4))
    try:
        t = torch.full((1, H, W, 248), float("nan"), device="cuda")
        out = torch.full((1, 2 * H, 2 * W, 64), float("nan"), device="cuda")
        dx = x.cuda()
        _ck(hip_lib.vfi_conv_forward_ex(L, ptr(dx), 120, H, W, ptr(t), 248, 1, 3, 0.0, 0.0, 0.0, None, 0, _stream()), "vfi_conv_forward_ex")
        _ck(hip_lib.vfi_atm_depth_to_space2(ptr(t), 248, ptr(out), 64, 1, H, W, c, _stream()), "vfi_atm_depth_to_space2")
        torch.cuda.synchronize()
    finally:
        hip_lib.vfi_conv_destroy(L)
    xd = x[..., :cin].double().permute(0, 3, 1, 2)
    want = F.prelu(F.conv_transpose2d(xd, wt.double(), b.double(), stride=2), sl.double())
    tol = (cin + 2) * U * F.conv_transpose2d(xd.abs(), wt.double().abs(), b.double().abs(), stride=2)
    got = out.cpu()
    assert torch.isnan(got[..., c:]).all(), "channels beyond the 61 were written"
    _report("deconv k2 s2 117 -> 61", (got[..., :c].double().permute(0, 3, 1, 2) - want).abs(), tol)


@pytest.mark.parametrize("H,W", [(3, 5), (16, 24)])
def test_depthwise_convolution_gelu(hip_lib, H, W):
    c = 448
    g = torch.Generator().manual_seed(H * W)
    x = torch.randn((2, H, W, c), generator=g) * 2
    wt, b = torch.randn((c, 1, 3, 3), generator=g) / 3, torch.randn((c,), generator=g) * 0.2
    wp = wt.reshape(c, 9).t().contiguous()
    out = torch.full((2, H, W, c), float("nan"), device="cuda")
    dx, dw, db = x.cuda(), wp.cuda(), b.cuda()
    _ck(hip_lib.vfi_atm_dwconv3x3_gelu(ptr(dx), c, ptr(dw), ptr(db), ptr(out), c, 2, H, W, c, _stream()), "vfi_atm_dwconv3x3_gelu")
    torch.cuda.synchronize()
    xd = x.double().permute(0, 3, 1, 2)
    a = F.conv2d(xd, wt.double(), b.double(), padding=1, groups=c)
    a_tol = 11 * U * F.conv2d(xd.abs(), wt.double().abs(), b.double().abs(), padding=1, groups=c)
    want = F.gelu(a)
    tol = 1.13 * a_tol + 8 * U * (a.abs() + want.abs()) + 1e-30      # gelu' <= 1.13; erff, the products of the erf form
    _report(f"dwconv {H}x{W}", (out.cpu().double().permute(0, 3, 1, 2) - want).abs(), tol)


def test_synthesis_kernels_with_flows_outside_the_image(hip_lib):
    H, W = 13, 18
    g = torch.Generator().manual_seed(7)
    src = torch.zeros(2, H, W, 8)
    src[..., :3] = torch.rand((2, H, W, 3), generator=g)
    orig = torch.zeros(2, H, W, 8)
    orig[..., :3] = torch.rand((2, H, W, 3), generator=g)
    mo = torch.zeros(H, W, 8)
    mo[..., :4] = torch.randn((H, W, 4), generator=g) * 6.0          # sigma 6 px on a 13x18 image: many taps outside
    mo[0, 0, :4] = torch.tensor([-40.0, 3.0, 1e9, -1e9])
    mo[1, 1, :4] = torch.tensor([0.0, 0.0, float(W), float(H)])
    mo[..., 4] = torch.randn((H, W), generator=g) * 3
    out = torch.full((H, W, 16), float("nan"), device="cuda")
    ds, do, dm = src.cuda(), orig.cuda(), mo.cuda()
    _ck(hip_lib.vfi_atm_blend_warps(ptr(ds), ptr(ds[1]), 8, ptr(do), ptr(do[1]), 8, ptr(dm), 8, ptr(out), 16, H, W, _stream()), "vfi_atm_blend_warps")
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got[..., 0:3], orig[0, ..., :3]) and torch.equal(got[..., 6:9], orig[1, ..., :3]) and torch.isnan(got[..., 15]).all()
    fl = mo.double().permute(2, 0, 1)[None]
    imgs = src[..., :3].double().permute(0, 3, 1, 2)
    w0, w1 = R.warp(imgs[0:1], fl[:, 0:2].clamp(-1e6, 1e6)), R.warp(imgs[1:2], fl[:, 2:4].clamp(-1e6, 1e6))
    m = torch.sigmoid(fl[:, 4:5])
    want = torch.cat([w0, w1, m * w0 + (1 - m) * w1], 1)[0].permute(1, 2, 0)
    # a coordinate is off by 8 u (|coordinate| + size) after the normalise / un-normalise round trip; a tap value moves by at most max |img| per pixel
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    cerr = [8 * U * ((xx + fl[0, 2 * k]).abs() + W + (yy + fl[0, 2 * k + 1]).abs() + H) for k in (0, 1)]
    wt = [(2 * cerr[k].clamp(max=1.0) + 8 * U)[..., None].expand(H, W, 3) for k in (0, 1)]
    tol = torch.cat([wt[0], wt[1], wt[0] + wt[1] + 8 * U], -1)
    _report("blend", (got[..., [3, 4, 5, 9, 10, 11, 12, 13, 14]].double() - want).abs(), tol)
    assert float((want[..., :3] == 0).all(-1).double().mean()) > 0.1, "the case has flows that leave the image"
    # the last step, on a crop
    res = torch.randn((H, W, 8), generator=g) * 2
    final = torch.full((H - 3, W - 5, 3), float("nan"), device="cuda")
    dres = res.cuda()
    _ck(hip_lib.vfi_atm_refine_out(ptr(out[..., 12:]), 16, ptr(dres), 8, ptr(final), H, W, 2, 3, H - 3, W - 5, _stream()), "vfi_atm_refine_out")
    torch.cuda.synchronize()
    wantf = (got[..., 12:15].double() + (2 * torch.sigmoid(res[..., :3].double()) - 1)).clamp(0, 1)[2:H - 1, 3:W - 2]
    _report("refine_out", (final.cpu().double() - wantf).abs(), torch.full_like(wantf, 8 * U))


# ---- the forward ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def engine(hip_lib):
    from cfi_amd import atm, atm_spec

    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    eng = atm.AtmEngine(atm_spec.seeded_state_dict(R.SEED))
    yield eng
    eng.close()


def _device_frame(eng, f0, f1, gm):
    one = lambda f: f[0].permute(1, 2, 0).contiguous().cuda()      # noqa: E731
    out = eng.forward(one(f0), one(f1), gm)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("mode", sorted(R.MODES))
@pytest.mark.parametrize("shape_name", sorted(R.NET_SHAPES))
def test_forward_matches_the_reference_and_the_restatement(engine, shape_name, mode, golden_dir):
    golden = np.load(os.path.join(golden_dir, "atm_net.npz"))
    gm = R.MODES[mode]
    f0, f1 = R.frames_of(shape_name)
    out = _device_frame(engine, f0, f1, gm)
    again = _device_frame(engine, f0, f1, gm)
    assert torch.equal(out, again), "the same pair twice, two results"
    d, sums_ok = cain_restated.compare(out, golden, f"{shape_name}_{'on' if gm else 'off'}_", R.NET_STRIDE, R.TOL)
    with torch.no_grad():
        want = R.atm_forward(R.state_dict_as(torch.float32), f0, f1, gm)[0].permute(1, 2, 0)
    dr = float((out - want).abs().max())
    print(f"ATM-lite {shape_name} {mode}: max |d| vs the reference's golden {d:.3e}, vs the float32 restatement at every pixel {dr:.3e}")
    assert d <= R.TOL and sums_ok and dr <= R.TOL


@pytest.mark.parametrize("case", ["odd_on", "odd_off"])
def test_node_on_a_100x180_clip(engine, case, golden_dir, monkeypatch):
    golden = np.load(os.path.join(golden_dir, "atm_node.npz"))
    R.check_node_case(case, R.run_node(case, monkeypatch, engine), golden)


def test_node_on_a_540x960_pair(engine, monkeypatch):
    import cfi_amd
    from cfi_amd import atm

    monkeypatch.setattr(atm, "load_file_from_github_release", lambda model_type, ckpt: ckpt)
    monkeypatch.setattr(atm, "cached_engine", lambda model_type, path, build: (engine, True))
    frames = cain_restated.seeded_frames(2, 540, 960, 3, 77)
    out = cfi_amd.ATM_VFI().vfi("atm-vfi-lite.pt", frames, 10, 2, "On")[0]
    assert out.shape == (3, 540, 960, 3) and torch.equal(out[0], frames[0]) and torch.equal(out[2], frames[1])
    x = frames.permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        want = R.atm_frame(R.state_dict_as(torch.float32), x[0:1], x[1:2], True)[0].permute(1, 2, 0)
    d = float((out[1] - want).abs().max())
    print(f"ATM-lite 540x960 through the node: max |d| vs the float32 restatement {d:.3e}; workspace {engine.workspace_bytes() / 2 ** 20:.0f} MiB")
    assert d <= R.TOL


def test_workspace_reused_across_shapes_gives_a_fresh_objects_frames(engine):
    from cfi_amd import atm, atm_spec

    a0, a1 = R.frames_of("128x192")
    b0, b1 = R.frames_of("64x64")
    _device_frame(engine, a0, a1, True)
    reused = [_device_frame(engine, b0, b1, True), _device_frame(engine, a0, a1, False)]
    fresh = atm.AtmEngine(atm_spec.seeded_state_dict(R.SEED))
    try:
        assert fresh.workspace_bytes() == 0
        assert torch.equal(_device_frame(fresh, b0, b1, True), reused[0])
        fresh.release_workspace()
        assert fresh.workspace_bytes() == 0
        assert torch.equal(_device_frame(fresh, a0, a1, False), reused[1])
        assert fresh.workspace_bytes() > 0
    finally:
        fresh.close()


def test_oversized_frame_is_refused_before_any_launch(engine):
    from cfi_amd import atm

    with pytest.raises(ValueError, match="index arithmetic"):
        atm.check_frame_size(2176, 3840)          # what AtmEngine.forward and the node call first
    before = engine.workspace_bytes()
    rc = engine.lib.vfi_atm_forward(engine.handle, ptr(torch.zeros(8, device="cuda")), ptr(torch.zeros(8, device="cuda")), 3, 2176, 3840, 1,
                                    ptr(torch.zeros(8, device="cuda")), _stream())
    from cfi_amd import _lib

    assert rc != 0 and "size limit" in _lib.last_error() and engine.workspace_bytes() == before
