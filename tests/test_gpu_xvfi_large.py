"""XVFI on frames up to 13 421 772 padded pixels (config.yaml's ``xvfi_large_frames``), on the device.

3. Forced, through the net: with the key on and the test option large_image_bytes at 1 byte every layer of the forward takes the large-image
   form of its kernel; the golden cases must come out bit-identical to the default path (hence within the 1e-3 gate of the goldens).
4. 2160x3840, both configurations: shape, finite, replay bit-identical, kept pair state equal to a fresh object's, the workspace figure of
   docs/design/xvfi.md, and the kernel family of every X4K layer with an operand of 2 GiB or more.  Whole-network parity at this size is
   deliberately not asked for (docs/design/xvfi.md: splat targets within 1e-4 of an integer in the reference itself).
5. The non-layer kernels that touch a buffer of 2 GiB or more at 2160x3840 (xvfi_assemble writes, xvfi_blend reads the 80-float RefineUNet
   input of the Vimeo configuration; the nearest x2 pass writes the 64-channel full-resolution map of X4K's last decoder layer), one call
   each at that size, sampled pixels in the last rows and around the row where the byte offset crosses 2^31.
6. The limits with the key on and off.

Bounds of 5, u = 2^-24 (the style of tests/test_gpu_xvfi_ops.py).
  assemble   channels copied from the features, the warped features and the frames: exact.  The flow field is constant with power-of-two
             components, so its bilinear x2 upscale is exact too (the weights are multiples of 1/4 and sum to 1).  The two image warps: the
             sampling position goes through the same fp32 chain in kernel and restatement, the corner weights are exact differences, an output
             is 4 products of three factors summed, at most 6 roundings over sum w |x| <= max|x|: 8 u max|x| (as bwarp's bound there).
  blend      occ0 = 1 / (1 + expf(-r)) within 8 u relative (the figure used for the same expression in tests/conv_restated.py), occ1 = 1 - occ0
             within 8 u occ0 + u absolute; the result is a weighted mean of w0 and w1 plus the residual: an absolute error d in a normalised
             weight moves the mean by at most d |w0 - w1| <= 2 d max|w|, d <= 2 (9 u) + 3 u for the products and the sum of the denominator;
             numerator, division and the final addition round 5 times over values <= max|w| + |res|:  (2 * 21 + 5) u max|w| + 2 u |out|.
  nearest    a copy: every element compared on the device.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cain_restated
import xvfi_restated as xr

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TWO31 = 2 ** 31
LARGE_DEFAULT = 2 ** 31 - 1
GEN2, WINO = 2, 3
# docs/design/xvfi.md, "Size limit": the workspace of one 2160x3840 pair after a forward at one timestep and one at another
WORKSPACE_BYTES = {xr.V: 31145472048, xr.X: 22032988208}


def _ck(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


def _rec(lib):
    r = (C.c_int32 * 8)()
    assert lib.vfi_test_last_conv_launch(r, 8) == 8
    return list(r)


@pytest.fixture
def key_on(monkeypatch):
    from cfi_amd import ckpt

    real = ckpt.load_config
    monkeypatch.setattr(ckpt, "load_config", lambda: dict(real(), xvfi_large_frames=True))


def _engine(config, seed, gain=1.0):
    from cfi_amd import xvfi, xvfi_spec

    return xvfi.XvfiEngine(xvfi_spec.seeded_state_dict(config, seed, gain), config)


# ---- 3. forced, through the net --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(xr.NET_CASES))
def test_forced_large_path_through_the_net_is_bit_identical(hip_lib, name, golden_dir, monkeypatch):
    from cfi_amd import ckpt

    golden = np.load(os.path.join(golden_dir, "xvfi_net.npz"))
    scale, S, h, w, gain = xr.NET_CASES[name]
    seed = int(golden[f"{name}_seed"])
    f = cain_restated.seeded_frames(2, h, w, 3, xr.FRAME_SEED).cuda()
    plain, forced = _engine((scale, S), seed, gain), _engine((scale, S), seed, gain)
    real = ckpt.load_config
    try:
        for t in xr.NET_TS:                                   # 0.5 first, then 0.2 on the kept pair state, on both objects
            want = plain.forward(f[0], f[1], t)
            assert plain.max_padded_pixels() == 6710886
            with monkeypatch.context() as mp:
                mp.setattr(ckpt, "load_config", lambda: dict(real(), xvfi_large_frames=True))
                assert hip_lib.vfi_test_set_option(b"large_image_bytes", 1) == 0
                try:
                    got = forced.forward(f[0], f[1], t)
                    torch.cuda.synchronize()
                    rec = _rec(hip_lib)
                finally:
                    hip_lib.vfi_test_set_option(b"large_image_bytes", LARGE_DEFAULT)
                assert forced.max_padded_pixels() == 13421772
            # the forward's last layer (the RefineUNet's 3x3, 64 -> 4) ran in its large form, Winograd store 3 or second-generation direct
            # form 3 - or, at the smallest sizes, on the first-generation tile s1_m1n1, which indexes floats and has one form only
            assert (rec[0] == WINO and rec[3] == 3) or (rec[0] == GEN2 and rec[2] == 3) or (rec[0] == 1 and h * w < 20000), rec
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"{name} t={t}: the large path differs from the default path"
            d, sums_ok = cain_restated.compare(got.cpu(), golden, f"{name}_t{t}_", xr.NET_STRIDE, xr.TOL)
            assert d <= xr.TOL and sums_ok, (name, t, d, sums_ok)
    finally:
        plain.close()
        forced.close()


# ---- 4. 2160x3840 -----------------------------------------------------------------------------------------------------------------------------

def _smooth_pair(H, W):
    """Two smooth frames in [0, 1] made on the device: sums of two waves per channel, the second frame's phases moved"""
    y = torch.arange(H, device="cuda", dtype=torch.float32).view(H, 1)
    x = torch.arange(W, device="cuda", dtype=torch.float32).view(1, W)
    frames = []
    for i in range(2):
        ch = []
        for c in range(3):
            a, b, q, r = 0.011 + 0.003 * c, 0.007 + 0.002 * c, 0.017 - 0.004 * c, 0.005 + 0.003 * c
            ch.append(0.5 + 0.3 * torch.sin(a * y + b * x + 0.3 * c + 0.05 * i) + 0.2 * torch.cos(q * y - r * x + 0.1 * c - 0.04 * i))
        frames.append(torch.stack(ch, -1).contiguous())
    return frames


@pytest.mark.parametrize("ckpt_name", [xr.V, xr.X])
def test_4k_forward(hip_lib, key_on, ckpt_name):
    from cfi_amd import xvfi_spec

    H, W = 2160, 3840
    f0, f1 = _smooth_pair(H, W)
    assert xvfi_spec.padded_size(H, W, ckpt_name)[0] * xvfi_spec.padded_size(H, W, ckpt_name)[1] > 6710886
    kept = _engine(ckpt_name, 7)
    try:
        a = kept.forward(f0, f1, 0.5).clone()
        rec = _rec(hip_lib)
        assert a.shape == (H, W, 3) and bool(torch.isfinite(a).all())
        b = kept.forward(f0, f1, 0.5)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the same pair twice differs"
        c = kept.forward(f0, f1, 0.2).clone()                 # the kept pair state, another timestep
        assert bool(torch.isfinite(c).all()) and not torch.equal(a, c)
        assert kept.workspace_bytes() == WORKSPACE_BYTES[ckpt_name], kept.workspace_bytes()
        if ckpt_name == xr.X:      # the last layer, 64 -> 4 on the 2.68 GB map: the Winograd kernel's large form (docs/design/xvfi.md)
            assert rec[0] == WINO and rec[3] == 3, rec
        kept.release_workspace()
        fresh = _engine(ckpt_name, 7)
        try:
            d = fresh.forward(f0, f1, 0.2)
            assert torch.equal(c.view(torch.int32), d.view(torch.int32)), "t = 0.2 after t = 0.5 differs from a fresh object's t = 0.2"
        finally:
            fresh.close()
    finally:
        kept.close()


def test_x4k_layers_with_an_operand_of_2gib_or_more(hip_lib):
    """The three layers of the X4K configuration that meet a 64-channel map of 2560 x 4096 pixels (2.68 GB), as the object creates and calls
    them: channel_converter writes one (its input is small: the second-generation direct kernel as before, whose stores are 64-bit),
    rec_ext_ds reads one (second-generation direct, large form), the RefineUNet's last layer reads one (Winograd, large form)."""
    Hp, Wp = 2560, 4096
    assert Hp * Wp * 64 * 4 >= TWO31
    big = torch.zeros((Hp, Wp, 64), device="cuda")
    small = torch.zeros((Hp, Wp, 8), device="cuda")
    half = torch.zeros((Hp // 2, Wp // 2, 64), device="cuda")
    g = torch.Generator().manual_seed(1)
    cases = [("channel_converter", 64, 3, 8, 3, 1, small, 8, big, 64, (GEN2, 32, 0, 0)),
             ("rec_ext_ds", 64, 64, 64, 3, 2, big, 64, half, 64, (GEN2, 39, 3, 0)),
             ("refine_unet dec3", 4, 64, 64, 3, 1, big, 64, small, 8, (WINO, 8, 0, 3))]
    for name, cout, cin, cphys, k, stride, src, ics, dst, ocs, expect in cases:
        wt, b = torch.randn((cout, cin, k, k), generator=g) * 0.05, torch.zeros(cout)
        handle = hip_lib.vfi_conv_create_ex(0, wt.data_ptr(), b.data_ptr(), cout, cin, k, stride, 0, None, cphys, None)
        assert handle
        try:
            _ck(hip_lib.vfi_conv_forward_ex(handle, src.data_ptr(), ics, Hp, Wp, dst.data_ptr(), ocs, 1, 1, 0.0, 0.0, 0.0, None, 0, None), name)
            torch.cuda.synchronize()
            rec = _rec(hip_lib)
            print(f"X4K {name}: launch {rec}")
            assert tuple(rec[:4]) == expect, (name, rec)
        finally:
            hip_lib.vfi_conv_destroy(handle)


# ---- 5. XVFI's own kernels at 2160x3840 ---------------------------------------------------------------------------------------------------------

def _warp_ref(img, n, X, Y, fx, fy):
    """bwarp of image n [.,H,W,cs] (device) at pixel (X, Y) with flow (fx, fy): the position in fp32 as the kernel computes it, taps in float64.
    -> (3 channel values float64, the sampled mask)"""
    f32 = np.float32
    H, W = img.shape[1], img.shape[2]
    gx = f32(2.0) * (f32(X) + f32(fx)) / f32(max(W - 1, 1)) - f32(1.0)
    gy = f32(2.0) * (f32(Y) + f32(fy)) / f32(max(H - 1, 1)) - f32(1.0)
    ix = float(((gx + f32(1.0)) / f32(2.0)) * f32(W - 1))
    iy = float(((gy + f32(1.0)) / f32(2.0)) * f32(H - 1))
    x0, y0 = int(np.floor(ix)), int(np.floor(iy))
    val, mask = np.zeros(3), 0.0
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            wgt = ((ix - x0) if dx else (x0 + 1 - ix)) * ((iy - y0) if dy else (y0 + 1 - iy))
            if 0 <= xx < W and 0 <= yy < H:
                val += img[n, yy, xx, :3].double().cpu().numpy() * wgt
                mask += wgt
    assert not (0.998 < mask < 0.9999), "a sampled mask next to the gate"
    return (val if mask >= 0.999 else np.zeros(3)), mask


def _sample_pixels(Hp, Wp, row_bytes):
    cross = TWO31 // row_bytes
    rows = [0, cross - 1, cross, cross + 1, Hp - 2, Hp - 1]
    cols = [0, 1, Wp // 2 - 1, Wp // 2, (TWO31 % row_bytes) // (row_bytes // Wp), Wp - 2, Wp - 1]
    return [(y, x) for y in rows for x in cols]


@pytest.fixture(scope="module")
def unet_input_4k(hip_lib):
    """vfi_xvfi_assemble at the Vimeo configuration's 2160x3840: the 80-float RefineUNet input, 2 654 208 000 bytes, shared by two tests"""
    h, w, s = 1080, 1920, 2
    Hp, Wp = h * s, w * s
    torch.manual_seed(11)
    feat = torch.randn((2, h, w, 128), device="cuda")
    warped = torch.randn((2, h, w, 64), device="cuda")
    img = torch.rand((2, Hp, Wp, 8), device="cuda")
    flow = torch.tensor([1.0, -2.0, 0.5, 4.0, 0.0, 0.0, 0.0, 0.0], device="cuda").repeat(h, w, 1).contiguous()
    out = torch.full((Hp, Wp, 80), float("nan"), device="cuda")
    assert out.numel() * 4 >= TWO31
    _ck(hip_lib.vfi_xvfi_assemble(feat.data_ptr(), 128, warped.data_ptr(), 64, flow.data_ptr(), 8, img.data_ptr(), 8, out.data_ptr(), 80, h, w, s, None), "assemble")
    torch.cuda.synchronize()
    yield dict(feat=feat, warped=warped, img=img, out=out, h=h, w=w, s=s, fl=(2.0, -4.0, 1.0, 8.0))
    del feat, warped, img, out
    torch.cuda.empty_cache()


def test_assemble_at_4k(unet_input_4k):
    u = unet_input_4k
    h, w, s, out, img = u["h"], u["w"], u["s"], u["out"], u["img"]
    Hp, Wp = h * s, w * s
    assert not bool(torch.isnan(out[-1]).any()) and not bool(torch.isnan(out[0]).any())
    tol = 8 * U * 1.0                                         # the frames are in [0, 1)
    worst = 0.0
    for Y, X in _sample_pixels(Hp, Wp, Wp * 80 * 4):
        got = out[Y, X].cpu()
        sub = (Y % s) * s + X % s
        for c in range(64):
            ch = c * s * s + sub
            m, cc = ch >> 6, ch & 63
            want = u["feat"][m, Y // s, X // s, cc] if m < 2 else u["warped"][m - 2, Y // s, X // s, cc]
            assert got[c].item() == want.item(), (Y, X, c)
        assert torch.equal(got[64:67], img[0, Y, X, :3].cpu()) and torch.equal(got[67:70], img[1, Y, X, :3].cpu()), (Y, X)
        assert got[76:80].tolist() == list(u["fl"]), (Y, X, got[76:80].tolist())
        for n, base, (fx, fy) in ((0, 70, u["fl"][:2]), (1, 73, u["fl"][2:])):
            want, _ = _warp_ref(img, n, X, Y, fx, fy)
            err = float(np.abs(got[base:base + 3].double().numpy() - want).max())
            worst = max(worst, err / tol)
            assert err <= tol, (Y, X, n, err, tol)
    print(f"assemble 2160x3840: warps max err / bound = {worst:.3f}")


def test_blend_at_4k(hip_lib, unet_input_4k):
    """vfi_xvfi_blend_out reads the warped frames out of the 2.65 GB buffer (channels 70..75, stride 80)"""
    u = unet_input_4k
    Hp, Wp, U80 = u["h"] * u["s"], u["w"] * u["s"], u["out"]
    torch.manual_seed(12)
    ro = torch.randn((Hp, Wp, 8), device="cuda") * 2
    out = torch.full((Hp, Wp, 3), float("nan"), device="cuda")
    t = 0.3
    _ck(hip_lib.vfi_xvfi_blend_out(ro.data_ptr(), 8, U80.data_ptr() + 4 * 70, 80, t, out.data_ptr(), Hp, Wp, Hp, Wp, None), "blend_out")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[-1]).any())
    t32 = float(np.float32(t))
    worst = 0.0
    for Y, X in _sample_pixels(Hp, Wp, Wp * 80 * 4):
        r = ro[Y, X].double().cpu().numpy()
        wv = U80[Y, X, 70:76].double().cpu().numpy()
        occ0 = 1.0 / (1.0 + np.exp(-r[0]))
        a, b = (1.0 - t32) * occ0, t32 * (1.0 - occ0)
        want = (a * wv[:3] + b * wv[3:]) / (a + b) + r[1:4]
        got = out[Y, X].double().cpu().numpy()
        tol = 47 * U * float(np.abs(wv).max()) + 2 * U * np.abs(want)
        ratio = float((np.abs(got - want) / tol).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (Y, X, got, want)
    print(f"blend 2160x3840: max err / bound = {worst:.3f}")


def test_nearest_x2_at_4k(hip_lib):
    """The nearest x2 pass in front of X4K's last decoder layer: [1280, 2048, 64] -> [2560, 4096, 64], 2 684 354 560 bytes; a copy, so every
    element is compared (on the device)."""
    h, w, c = 1280, 2048, 64
    torch.manual_seed(13)
    src = torch.randn((h, w, c), device="cuda")
    dst = torch.full((2 * h, 2 * w, c), float("nan"), device="cuda")
    assert dst.numel() * 4 >= TWO31
    _ck(hip_lib.vfi_upsample_nearest(src.data_ptr(), c, dst.data_ptr(), c, 1, h, w, 2 * h, 2 * w, c, None), "upsample_nearest")
    torch.cuda.synchronize()
    v = dst.view(h, 2, w, 2, c)
    for dy in (0, 1):
        for dx in (0, 1):
            assert torch.equal(v[:, dy, :, dx].view(torch.int32), src.view(torch.int32)), (dy, dx)


# ---- 6. limits ----------------------------------------------------------------------------------------------------------------------------------

def test_limits_with_the_key_on_and_off(hip_lib, monkeypatch):
    from cfi_amd import _lib, ckpt, xvfi

    eng = _engine(xr.X, 7)
    tiny = torch.zeros(16, 16, 3, device="cuda")
    real = ckpt.load_config
    try:
        # key off: as before
        assert eng.max_padded_pixels() == xvfi.MAX_PADDED_PIXELS == 6710886 == hip_lib.vfi_xvfi_max_padded_pixels()
        assert hip_lib.vfi_xvfi_object_max_padded_pixels(eng.handle) == 6710886
        eng.forward(tiny, tiny, 0.5)
        before = eng.workspace_bytes()
        assert before > 0
        with pytest.raises(ValueError, match="index arithmetic"):
            big = torch.empty((2176, 3840, 3), device="cuda")
            eng.forward(big, big, 0.5)
        rc = hip_lib.vfi_xvfi_forward(eng.handle, tiny.data_ptr(), tiny.data_ptr(), 3, 2176, 3840, 0.5, tiny.data_ptr(), None)
        assert rc != 0 and "size limit" in _lib.last_error() and "2 GiB" in _lib.last_error()
        assert eng.workspace_bytes() == before
        # key on
        monkeypatch.setattr(ckpt, "load_config", lambda: dict(real(), xvfi_large_frames=True))
        assert eng.max_padded_pixels() == xvfi.LARGE_MAX_PADDED_PIXELS == 13421772 == hip_lib.vfi_xvfi_large_max_padded_pixels()
        assert hip_lib.vfi_xvfi_object_max_padded_pixels(eng.handle) == 13421772
        with pytest.raises(ValueError, match="index arithmetic"):
            big = torch.empty((3072, 4608, 3), device="cuda")
            eng.forward(big, big, 0.5)
        # the C entry point itself: the size is checked before the frames are touched (16x16 buffers stand behind a 3072x4608 claim)
        rc = hip_lib.vfi_xvfi_forward(eng.handle, tiny.data_ptr(), tiny.data_ptr(), 3, 3072, 4608, 0.5, tiny.data_ptr(), None)
        assert rc != 0 and "size limit" in _lib.last_error() and "4 GiB" in _lib.last_error()
        assert eng.workspace_bytes() == before
        # and off again: read at call time
        monkeypatch.setattr(ckpt, "load_config", real)
        assert eng.max_padded_pixels() == 6710886
        rc = hip_lib.vfi_xvfi_forward(eng.handle, tiny.data_ptr(), tiny.data_ptr(), 3, 2176, 3840, 0.5, tiny.data_ptr(), None)
        assert rc != 0 and "size limit" in _lib.last_error()
        assert eng.workspace_bytes() == before
    finally:
        eng.close()
