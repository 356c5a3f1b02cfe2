"""-m gpu: the ATM-base path on the device (config.yaml's ``atm_base`` key patched on where the Python side asks for it).

  1. vfi_atm_window_attention at ATM-base's head widths, 48 (C = 384, window 8) and 84 (C = 672, window 12), on the eight token maps of
     ATTN_CASES, both kinds: against the float64 evaluation and within the float64 rounding bound of tests/test_gpu_atm.py (its
     ``_attention64``, imported, not copied), with the per-head offsets and vfi_atm_motion_mlp behind them; and the whole block finished from
     the device's attention output against the reference's block goldens (tests/golden/atm_base_attn.npz, atm_base_attn_self.npz), the
     motion read-out included.
  2. The shared ops at base's widths, each against float64 with the bound of its lite-width counterpart in the existing GPU tests:
     vfi_layernorm at 384 and 672 (both beyond the one-wave-per-token path's 256; 2e-5, tests/test_gpu_gmfss_ops.py), the depthwise
     convolution at 1536 and 2688 channels on a 5x7 and an 8x8 map, the k2 s2 transposed convolution at 101 channels (tests/test_gpu_atm.py).
  3. The forward: <= 1e-3 per pixel against tests/golden/atm_base_net.npz and against the float32 restatement at every pixel, three shapes,
     both modes; the maxima are printed.
  4. The node with the key on: the node cases against atm_base_node.npz, one 270x480 pair against the restatement, twice the same bits.
  5. The object: a workspace reused across shapes, the per-object size limit, a lite state dict handed to the base variant's create.
  6. A lite engine created after a base engine still meets atm_net.npz."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import atm_base_restated as B
import atm_restated
import cain_restated
import test_gpu_atm as lite      # the bounds of the same kernels at lite's widths
from gpu_util import ptr

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
_ck, _stream, _report = lite._ck, lite._stream, lite._report


@pytest.fixture(autouse=True)
def base_on(monkeypatch):
    from cfi_amd import ckpt

    monkeypatch.setattr(ckpt, "load_config", B.config_with(True))


# ---- 1. the attention kernel ---------------------------------------------------------------------------------------------------------

def _qkv_maps(name, cross):
    """lite._qkv_maps over the base cases: float32 q, k, v token maps [2 h w + 1, C], the last token the pad token; also norm1(x)"""
    p, x = B.attn_case(name, cross)
    C_ = x.shape[-1]
    tok = torch.cat([x.reshape(-1, C_), torch.zeros(1, C_)])
    xn = F.layer_norm(tok, (C_,), p["norm1.weight"], p["norm1.bias"])
    if cross:
        q, kv = F.linear(xn, p["attn.q.weight"]), F.linear(xn, p["attn.kv.weight"])
        return p, xn, q.contiguous(), kv[:, :C_].contiguous(), kv[:, C_:].contiguous()
    qkv = F.linear(xn, p["attn.qkv.weight"])
    return p, xn, qkv[:, :C_].contiguous(), qkv[:, C_:2 * C_].contiguous(), qkv[:, 2 * C_:].contiguous()


@pytest.mark.parametrize("cross", [True, False], ids=["cross", "self"])
@pytest.mark.parametrize("name", sorted(B.ATTN_CASES))
def test_window_attention_kernel_at_base_widths(hip_lib, name, cross, golden_dir):
    h, w, win, shift = B.ATTN_CASES[name]
    p, xn, q, k, v = _qkv_maps(name, cross)
    C_ = q.shape[1]
    assert C_ == (384 if win == 8 else 672)
    ntok = 2 * h * w
    want, tol, woffs, offs_tol = lite._attention64(q, k, v, h, w, win, shift, cross)
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
    kind = "cross" if cross else "self"
    _report(f"ATM-base attention {name} {kind}", (got.double() - want).abs(), tol)
    # the block finished from the device's attention output, against the reference's own block
    golden = np.load(os.path.join(golden_dir, B.attn_golden_file(cross)))
    with torch.no_grad():
        y = xn[:ntok] + F.linear(got, p["attn.proj.weight"], p["attn.proj.bias"])
        blk = B.mlp_block(p, y.reshape(2, h, w, C_))
    d = float((blk[..., ::B.ATTN_CH_STRIDE] - torch.from_numpy(golden[f"{name}_{kind}_x"])).abs().max())
    print(f"ATM-base block {name} {kind}: max |d| vs the reference's block {d:.3e}")
    if not cross:
        assert d <= B.TOL
        return
    assert torch.equal(outs[0][1], outs[1][1]) and torch.isfinite(goffs).all()
    _report(f"ATM-base offsets {name}", (goffs.double() - woffs).abs(), offs_tol)
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
    _report(f"ATM-base motion mlp {name}", (gotm - wantm).abs(), tolm[..., 0])
    dm = float((gotm.float().reshape(2, h, w, 2) - torch.from_numpy(golden[f"{name}_cross_motion"])).abs().max())
    print(f"ATM-base block {name} cross: motion read-out max |d| vs the reference's {dm:.3e}")
    assert d <= B.TOL and dm <= B.TOL


@pytest.mark.parametrize("C_,win", [(224, 12), (352, 8), (384, 12), (672, 8), (448, 8), (768, 12)])
def test_every_other_width_and_window_pair_is_refused(hip_lib, C_, win):
    from cfi_amd import _lib

    t = torch.zeros(8 * 8 * 2 + 1, C_, device="cuda")
    rc = hip_lib.vfi_atm_window_attention(ptr(t), C_, ptr(t), C_, ptr(t), C_, 128, ptr(t), C_, None, 8, 8, C_, win, 0, 0, _stream())
    msg = _lib.last_error()
    assert rc != 0 and all(s in msg for s in ("224 / 8", "352 / 12", "384 / 8", "672 / 12")), msg


# ---- 2. the shared ops at base's widths ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tokens,c", [(2 * 5 * 7 + 1, 384), (2 * 4 * 4 + 1, 672), (1030, 672)])
def test_layernorm_at_384_and_672(hip_lib, tokens, c):
    g = torch.Generator().manual_seed(tokens + c)
    x = torch.randn(tokens, c, generator=g) * 3 + 1
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    want = F.layer_norm(x.double(), (c,), gamma.double(), beta.double(), 1e-5)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    out = torch.full((tokens, c + 8), float("nan"), device="cuda")
    _ck(hip_lib.vfi_layernorm(ptr(xd), c, c, tokens, ptr(gd), ptr(bd), ptr(out), c + 8, _stream()), "vfi_layernorm")
    torch.cuda.synchronize()
    got = out.cpu()
    d = float((got[:, :c].double() - want).abs().max())
    print(f"layernorm C = {c}, {tokens} tokens: max err {d:.3e} (bound 2e-5)")
    assert d <= 2e-5 and torch.isnan(got[:, c:]).all()


@pytest.mark.parametrize("H,W", [(5, 7), (8, 8)])
@pytest.mark.parametrize("c", [1536, 2688])
def test_depthwise_convolution_gelu_at_base_widths(hip_lib, c, H, W):
    g = torch.Generator().manual_seed(c + H * W)
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
    tol = 1.13 * a_tol + 8 * U * (a.abs() + want.abs()) + 1e-30      # as tests/test_gpu_atm.py: gelu' <= 1.13; erff, the products of the erf form
    _report(f"dwconv C = {c} {H}x{W}", (out.cpu().double().permute(0, 3, 1, 2) - want).abs(), tol)


def test_transposed_convolution_k2s2_at_101_channels(hip_lib):
    cin, c, H, W = 197, 101, 5, 7                      # upsample_pyramid.2 of ATM-base: 197 -> 101, strides r8(197) = 200, r8(404) = 408, r8(101) = 104
    g = torch.Generator().manual_seed(101)
    x = torch.zeros(1, H, W, 200)
    x[..., :cin] = torch.randn((1, H, W, cin), generator=g)
    wt, b, sl = torch.randn((cin, c, 2, 2), generator=g) / cin ** 0.5, torch.randn((c,), generator=g) * 0.1, torch.rand((c,), generator=g) * 0.5
    w1 = wt.permute(2, 3, 1, 0).reshape(4 * c, cin).contiguous()          # [(2 ky + kx) c + co][ci]
    L = lite._layer(hip_lib, w1, b.repeat(4), 4 * c, cin, 200, sl.repeat(4))
    try:
        t = torch.full((1, H, W, 408), float("nan"), device="cuda")
        out = torch.full((1, 2 * H, 2 * W, 104), float("nan"), device="cuda")
        dx = x.cuda()
        _ck(hip_lib.vfi_conv_forward_ex(L, ptr(dx), 200, H, W, ptr(t), 408, 1, 3, 0.0, 0.0, 0.0, None, 0, _stream()), "vfi_conv_forward_ex")
        _ck(hip_lib.vfi_atm_depth_to_space2(ptr(t), 408, ptr(out), 104, 1, H, W, c, _stream()), "vfi_atm_depth_to_space2")
        torch.cuda.synchronize()
    finally:
        hip_lib.vfi_conv_destroy(L)
    xd = x[..., :cin].double().permute(0, 3, 1, 2)
    want = F.prelu(F.conv_transpose2d(xd, wt.double(), b.double(), stride=2), sl.double())
    tol = (cin + 2) * U * F.conv_transpose2d(xd.abs(), wt.double().abs(), b.double().abs(), stride=2)
    got = out.cpu()
    assert torch.isnan(got[..., c:]).all(), "channels beyond the 101 were written"
    _report("deconv k2 s2 197 -> 101", (got[..., :c].double().permute(0, 3, 1, 2) - want).abs(), tol)


# ---- 3. - 6. the forward, the node, the object ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def engine(hip_lib):
    from cfi_amd import atm, ckpt

    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    real = ckpt.load_config
    ckpt.load_config = B.config_with(True)      # (the function-scoped patch is not up yet when a module fixture is built)
    try:
        eng = atm.AtmEngine(B.state_dict_as(torch.float32), "base")
    finally:
        ckpt.load_config = real
    yield eng
    eng.close()


def _device_frame(eng, f0, f1, gm):
    one = lambda f: f[0].permute(1, 2, 0).contiguous().cuda()      # noqa: E731
    out = eng.forward(one(f0), one(f1), gm)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("mode", sorted(B.MODES))
@pytest.mark.parametrize("shape_name", sorted(B.NET_SHAPES))
def test_forward_matches_the_reference_and_the_restatement(engine, shape_name, mode, golden_dir):
    golden = np.load(os.path.join(golden_dir, "atm_base_net.npz"))
    gm = B.MODES[mode]
    f0, f1 = B.frames_of(shape_name)
    out = _device_frame(engine, f0, f1, gm)
    d, sums_ok = cain_restated.compare(out, golden, f"{shape_name}_{'on' if gm else 'off'}_", B.NET_STRIDE, B.TOL)
    dr = float((out - B.restated32(shape_name, mode)).abs().max())
    print(f"ATM-base {shape_name} {mode}: max |d| vs the reference's golden {d:.3e}, vs the float32 restatement at every pixel {dr:.3e}")
    assert d <= B.TOL and sums_ok and dr <= B.TOL


@pytest.mark.parametrize("case", sorted(B.NODE_CASES))
def test_node_cases_match_the_reference_node(engine, case, golden_dir, monkeypatch):
    golden = np.load(os.path.join(golden_dir, "atm_base_node.npz"))
    B.check_node_case(case, B.run_node(case, monkeypatch, engine), golden)


def test_node_on_a_270x480_pair_twice(engine, monkeypatch):
    import cfi_amd
    from cfi_amd import atm

    monkeypatch.setattr(atm, "load_file_from_github_release", lambda model_type, ckpt: ckpt)
    monkeypatch.setattr(atm, "cached_engine", lambda model_type, path, build: (engine, True))
    frames = cain_restated.seeded_frames(2, 270, 480, 3, 77)
    out = cfi_amd.ATM_VFI().vfi("atm-vfi-base-pct.pt", frames, 10, 2, "On")[0]
    again = cfi_amd.ATM_VFI().vfi("atm-vfi-base-pct.pt", frames, 10, 2, "On")[0]
    assert out.shape == (3, 270, 480, 3) and torch.equal(out[0], frames[0]) and torch.equal(out[2], frames[1])
    assert torch.equal(out, again), "the same pair twice, two results"
    x = frames.permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        want = B.atm_frame(B.state_dict_as(torch.float32), x[0:1], x[1:2], True)[0].permute(1, 2, 0)
    d = float((out[1] - want).abs().max())
    print(f"ATM-base 270x480 through the node: max |d| vs the float32 restatement {d:.3e}; workspace {engine.workspace_bytes() / 2 ** 20:.0f} MiB")
    assert d <= B.TOL


def test_workspace_reused_across_shapes_gives_a_fresh_objects_frames(engine):
    from cfi_amd import atm

    a0, a1 = B.frames_of("128x192")
    b0, b1 = B.frames_of("64x64")
    _device_frame(engine, a0, a1, True)
    reused = [_device_frame(engine, b0, b1, True), _device_frame(engine, a0, a1, False)]
    fresh = atm.AtmEngine(B.state_dict_as(torch.float32), "base")
    try:
        assert fresh.workspace_bytes() == 0
        assert torch.equal(_device_frame(fresh, b0, b1, True), reused[0])
        fresh.release_workspace()
        assert fresh.workspace_bytes() == 0
        assert torch.equal(_device_frame(fresh, a0, a1, False), reused[1])
        assert fresh.workspace_bytes() > 0
    finally:
        fresh.close()


def test_oversized_frame_is_refused_before_any_launch_and_the_limits_agree(engine, hip_lib):
    from cfi_amd import _lib, atm

    assert atm.MAX_PADDED_PIXELS_BASE == engine.max_padded_pixels() == hip_lib.vfi_atm_object_max_padded_pixels(engine.handle) == (2 ** 31 - 1) // 512
    assert atm.MAX_PADDED_PIXELS == hip_lib.vfi_atm_max_padded_pixels() == (2 ** 31 - 1) // 320 > atm.MAX_PADDED_PIXELS_BASE
    assert 2176 * 3840 > atm.MAX_PADDED_PIXELS_BASE >= 1472 * 2560
    with pytest.raises(ValueError, match="index arithmetic"):
        atm.check_frame_size(2176, 3840, "base")          # what AtmEngine.forward and the node call first
    before = engine.workspace_bytes()
    z = torch.zeros(8, device="cuda")
    for H, W in ((2176, 3840), (1600, 3000)):      # the second fits lite's limit and not base's
        rc = engine.lib.vfi_atm_forward(engine.handle, ptr(z), ptr(z), 3, H, W, 1, ptr(z), _stream())
        assert rc != 0 and "size limit of ATM-base" in _lib.last_error() and engine.workspace_bytes() == before


def test_a_lite_state_dict_to_the_base_create_fails_with_a_message(hip_lib):
    from cfi_amd import _lib, atm_spec

    sd = atm_spec.seeded_state_dict(B.SEED)
    keys = list(atm_spec.weight_shapes())
    tensors = [sd[k].contiguous() for k in keys]
    ptrs = (C.c_void_p * len(keys))(*[t.data_ptr() for t in tensors])
    numels = (C.c_int64 * len(keys))(*[t.numel() for t in tensors])
    assert not hip_lib.vfi_atm_create_variant(ptrs, numels, len(keys), 1)
    msg = _lib.last_error()
    assert "ATM-base" in msg and "tensor 0 has 432 elements, expected 648" in msg, msg
    assert not hip_lib.vfi_atm_create_variant(ptrs, numels, len(keys), 2) and "variant 2" in _lib.last_error()
    h = hip_lib.vfi_atm_create_variant(ptrs, numels, len(keys), 0)      # and the same tensors are ATM-lite's
    assert h
    hip_lib.vfi_atm_destroy(h)


@pytest.mark.parametrize("mode", sorted(atm_restated.MODES))
def test_a_lite_engine_after_a_base_engine_still_meets_its_goldens(engine, mode, golden_dir):
    from cfi_amd import atm, atm_spec

    golden = np.load(os.path.join(golden_dir, "atm_net.npz"))
    gm = atm_restated.MODES[mode]
    f0, f1 = atm_restated.frames_of("128x192")
    _device_frame(engine, *B.frames_of("128x192"), gm)      # the base object has run in this process
    eng = atm.AtmEngine(atm_spec.seeded_state_dict(atm_restated.SEED))
    try:
        assert eng.variant == "lite" and eng.max_padded_pixels() == atm.MAX_PADDED_PIXELS
        out = _device_frame(eng, f0, f1, gm)
    finally:
        eng.close()
    d, sums_ok = cain_restated.compare(out, golden, f"128x192_{'on' if gm else 'off'}_", atm_restated.NET_STRIDE, atm_restated.TOL)
    print(f"ATM-lite 128x192 {mode} after ATM-base: max |d| vs the reference's golden {d:.3e}")
    assert d <= atm_restated.TOL and sums_ok
