"""ATM on frames up to 13 421 772 (lite) / 8 388 607 (base) padded pixels (config.yaml's ``atm_large_frames``), on the device.

1. Forced, through the net: with the key on and the test option large_image_bytes at 1 byte every layer of the forward that has a large-image
   form takes it (the log of LARGE launches, vfi_test_large_launches, must hold the full-resolution PReLU layers of docs/design/atm.md's
   table); the golden cases come out bit-identical to the default path, lite and base, both modes, one ensemble case each.
2. 2160x3840, both variants, "On": shape, finite, replay bit-identical, the workspace figure of docs/design/atm.md, the kernel family of every
   layer whose operand holds 2 GiB or more; without the key the same call is refused.  One ensemble forward, on lite.
3. ATM's own kernels that touch a buffer of 2 GiB or more at that size, one call each at the real size: atm_blend (writes ATM-base's 120-float
   refinement input, 4.01 GB, and reads its motion channels out of it), atm_out (reads it), atm_depth_to_space (408-float taps at half
   resolution, 3.41 GB, into the 104-float map, 3.48 GB).  Sampled pixels in the last rows and around the row where the byte offset crosses
   2^31 against float64; the interleave is a copy, so every element is compared on the device.  ATM-lite once at 2880x4608, next to its limit.
4. The limits with the key on and off, from a live object.

Bounds of 3, u = 2^-24 (the style of tests/test_gpu_xvfi_large.py).
  warp       the sampling position goes through the same fp32 chain in kernel and restatement (the file is built without contraction), the corner
             weights are fp32 products of exact differences, restated alike; an output is 4 products summed: 4 roundings of terms whose
             magnitudes sum to <= max|x|, and 3 additions: 7 u max|x|.
  blend      m = 1 / (1 + expf(-l)) within 8 u relative (the figure of tests/conv_restated.py for this expression), 1 - m within 8 u m + u
             absolute; I_t = m w0 + (1 - m) w1: the weights' errors move it by (16 u + u) max|w|, the two products and the sum round 3 times
             over values <= max|w|, the warps bring 7 u max|x| each weighted by m and 1 - m: (17 + 3 + 7) u max|x| = 27 u max|x|.
  out        s = sigmoid(r) within 8 u; 2 s - 1 within 16 u + u; + I_t rounds once over |I_t| + 1; the clamp is 1-Lipschitz: 18 u + u |I_t|,
             asked as 20 u (1 + |I_t|).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import atm_base_restated as B
import atm_ensemble_restated as E
import atm_restated as R
import cain_restated
from cfi_amd import ckpt as _ckpt

_REAL_CONFIG = _ckpt.load_config      # the package's own config.yaml, whatever a test has patched in since

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TWO31 = 2 ** 31
LARGE_DEFAULT = 2 ** 31 - 1
GEN2, WINO = 2, 3
LIMITS = {"lite": (6710886, 13421772), "base": (4194303, 8388607)}
HP, WP = 2176, 3840
# docs/design/atm.md, "4K": the workspace of one 2160x3840 pair after one "On" forward on a fresh object
WORKSPACE_BYTES = {"lite": 37764648960, "base": 65944227840}
# ... and the layers that meet an operand image of 2 GiB or more there, as the LARGE log names them: (family, Hin, Win, in_cs, Cin_p, Cout)
LARGE_LAYERS = {"lite": {(WINO, HP, WP, 80, 80, 32)},                                                       # proj
                "base": {(WINO, HP, WP, 104, 104, 101),                                                     # up[2].c1 and up[2].c2
                         (WINO, HP, WP, 120, 120, 64), (GEN2, HP, WP, 128, 64, 64), (WINO, HP, WP, 128, 128, 64)}}      # proj, down1, rh[0]


def _ck(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


def _large_log(lib):
    buf = (C.c_int32 * (6 * 256))()
    n = lib.vfi_test_large_launches(buf, 256)
    return [tuple(buf[6 * i:6 * i + 6]) for i in range(min(n, 256))]


def _config(**keys):
    return lambda: dict(_REAL_CONFIG(), atm_base=True, atm_ensemble=True, **keys)


@pytest.fixture
def keys_off(monkeypatch):
    from cfi_amd import ckpt

    monkeypatch.setattr(ckpt, "load_config", _config())


def _engine(variant):
    from cfi_amd import atm

    return atm.AtmEngine(E.state_dict_as(variant, torch.float32), variant)


def _device_frame(eng, f0, f1, gm):
    one = lambda f: f[0].permute(1, 2, 0).contiguous().cuda()      # noqa: E731
    out = eng.forward(one(f0), one(f1), gm)
    torch.cuda.synchronize()
    return out


# ---- 1. forced, through the net --------------------------------------------------------------------------------------------------------------

def _net_cases():
    cases = []
    for variant in ("lite", "base"):
        for shape in sorted(R.NET_SHAPES):
            for mode in sorted(R.MODES):
                cases.append((variant, shape, mode))
    cases += [("lite", "128x192_s4", E.ENSEMBLE), ("base", "128x192_s1", E.ENSEMBLE)]
    return cases


@pytest.mark.parametrize("variant,shape,mode", _net_cases())
def test_forced_large_path_through_the_net_is_bit_identical(hip_lib, keys_off, variant, shape, mode, golden_dir, monkeypatch):
    from cfi_amd import atm, ckpt

    ens = mode == E.ENSEMBLE
    M = B if variant == "base" else R
    if ens:
        golden = np.load(os.path.join(golden_dir, E.GOLDEN_PREFIX[variant] + "_net.npz"))
        f0, f1 = E.frames_of(variant, shape)
        gm, prefix = atm.ENSEMBLE, shape + "_"
    else:
        golden = np.load(os.path.join(golden_dir, "atm_base_net.npz" if variant == "base" else "atm_net.npz"))
        f0, f1 = M.frames_of(shape)
        gm = R.MODES[mode]
        prefix = f"{shape}_{'on' if gm else 'off'}_"
    h, w = f0.shape[2:]
    hp, wp = atm.padded_size(h, w)
    plain, forced = _engine(variant), _engine(variant)
    try:
        want = _device_frame(plain, f0, f1, gm)
        assert plain.max_padded_pixels() == LIMITS[variant][0]
        with monkeypatch.context() as mp:
            mp.setattr(ckpt, "load_config", _config(atm_large_frames=True))
            assert hip_lib.vfi_test_set_option(b"large_image_bytes", 1) == 0
            try:
                _large_log(hip_lib)
                got = _device_frame(forced, f0, f1, gm)
                log = _large_log(hip_lib)
            finally:
                hip_lib.vfi_test_set_option(b"large_image_bytes", LARGE_DEFAULT)
            assert forced.max_padded_pixels() == LIMITS[variant][1]
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"ATM-{variant} {shape} {mode}: the large path differs from the default path"
        d, sums_ok = cain_restated.compare(got.cpu(), golden, prefix, R.NET_STRIDE, R.TOL)
        assert d <= R.TOL and sums_ok, (variant, shape, mode, d, sums_ok)
        # the full-resolution PReLU layers of the table: up[2].c1, proj, rh[0] (3x3 stride 1: either kernel) and ATM-base's down1 (stride 2,
        # the direct kernel's tile 39; ATM-lite's, 32 output channels, runs on the first-generation tile s2_m1n1, which has one form only)
        keyed = {(e[1], e[2], e[3], e[5]): e[0] for e in log}
        hid, cl = (64, 384) if variant == "base" else (32, 224)
        rcs, uc = (cl // 4 + 5 + 15 + 7) // 8 * 8, cl // 4 + 5
        need = [(hp, wp, (uc + 7) // 8 * 8, uc), (hp, wp, rcs, hid), (hp, wp, 2 * hid, hid)]
        if variant == "lite" and hp * wp < 20000:      # 32 output channels on a map this small: the first-generation tile s1_m1n1, one form only
            need = need[:1]
        for key in need:
            assert keyed.get(key) in (GEN2, WINO), f"ATM-{variant} {shape} {mode}: no LARGE launch for layer {key}; the log has {len(log)}: {sorted(set(log))}"
        if variant == "base":
            assert (GEN2, hp, wp, 128, 64, 64) in log, sorted(set(log))
        print(f"ATM-{variant} {shape} {mode}: {len(log)} LARGE launches, max |d| vs the golden {d:.3e}")
    finally:
        plain.close()
        forced.close()


# ---- 2. 2160x3840 -----------------------------------------------------------------------------------------------------------------------------

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


@pytest.mark.parametrize("variant", ["lite", "base"])
def test_4k_forward(hip_lib, keys_off, variant, monkeypatch):
    from cfi_amd import _lib, atm, ckpt

    H, W = 2160, 3840
    assert atm.padded_size(H, W) == (HP, WP) and HP * WP > LIMITS[variant][0]
    torch.cuda.empty_cache()
    f0, f1 = _smooth_pair(H, W)
    eng = _engine(variant)
    out = torch.empty((H, W, 3), device="cuda")
    try:
        # without the key: refused by the engine and by the C entry point, nothing allocated
        with pytest.raises(ValueError, match="index arithmetic"):
            eng.forward(f0, f1, True)
        rc = hip_lib.vfi_atm_forward(eng.handle, f0.data_ptr(), f1.data_ptr(), 3, H, W, 1, out.data_ptr(), None)
        assert rc != 0 and "size limit of ATM-" + variant in _lib.last_error() and "2 GiB" in _lib.last_error(), _lib.last_error()
        assert eng.workspace_bytes() == 0
        monkeypatch.setattr(ckpt, "load_config", _config(atm_large_frames=True))
        _large_log(hip_lib)
        a = eng.forward(f0, f1, True).clone()
        torch.cuda.synchronize()
        log = _large_log(hip_lib)
        ws = eng.workspace_bytes()
        print(f"ATM-{variant} 2160x3840 On: workspace {ws} bytes; LARGE launches {log}")
        assert a.shape == (H, W, 3) and bool(torch.isfinite(a).all())
        assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0 and float(a.std()) > 0.01
        b = eng.forward(f0, f1, True)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the same pair twice differs"
        assert set(log) == LARGE_LAYERS[variant], (sorted(set(log)), sorted(LARGE_LAYERS[variant]))
        assert ws == WORKSPACE_BYTES[variant], ws
        if variant == "lite":      # one ensemble forward, on the smaller model only
            c = eng.forward(f0, f1, atm.ENSEMBLE)
            assert c.shape == (H, W, 3) and bool(torch.isfinite(c).all())
            losses, level = eng.ensemble_record()
            assert all(np.isfinite(losses)) and level in (0, 1, 2)
            print(f"ATM-lite 2160x3840 ensemble: losses {losses}, level {level}, workspace {eng.workspace_bytes()} bytes")
    finally:
        eng.close()


def test_lite_forward_next_to_its_limit(hip_lib, keys_off, monkeypatch):
    """ATM-lite at 2880x4608 = 13 271 040 padded pixels, the largest multiple-of-64 frame of that width below its 13 421 772: the buffers that
    are still under 2 GiB at 2160x3840 are over it here (docs/design/atm.md "4K": up_d2 / up_c2 and rf_c6, 64 floats, 3.40 GB; the level-2
    taps, 248 floats at half resolution, 3.29 GB), and their layers take the large forms."""
    from cfi_amd import ckpt

    H, W = 2880, 4608
    assert H * W <= LIMITS["lite"][1] < (H + 64) * W and H * W * 64 * 4 >= TWO31 and (H // 2) * (W // 2) * 248 * 4 >= TWO31
    torch.cuda.empty_cache()
    f0, f1 = _smooth_pair(H, W)
    monkeypatch.setattr(ckpt, "load_config", _config(atm_large_frames=True))
    eng = _engine("lite")
    try:
        _large_log(hip_lib)
        a = eng.forward(f0, f1, True).clone()
        torch.cuda.synchronize()
        log = _large_log(hip_lib)
        print(f"ATM-lite {H}x{W} On: workspace {eng.workspace_bytes()} bytes; LARGE launches {log}")
        assert a.shape == (H, W, 3) and bool(torch.isfinite(a).all()) and float(a.std()) > 0.01
        b = eng.forward(f0, f1, True)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the same pair twice differs"
        # up[2].c1 and up[2].c2 (one entry: same shape), proj, rh[0]; down1 (32 output channels, stride 2) runs on the first-generation
        # tile, which indexes floats
        assert set(log) == {(WINO, H, W, 64, 64, 61), (WINO, H, W, 80, 80, 32), (WINO, H, W, 64, 64, 32)}, sorted(set(log))
    finally:
        eng.close()


# ---- 3. ATM's own kernels at 2160x3840 -----------------------------------------------------------------------------------------------------------

def _sample_pixels(Hp, Wp, row_bytes):
    cross = TWO31 // row_bytes
    rows = [0, cross - 1, cross, cross + 1, Hp - 2, Hp - 1]
    cols = [0, 1, Wp // 2 - 1, Wp // 2, (TWO31 % row_bytes) // (row_bytes // Wp), Wp - 2, Wp - 1]
    return [(y, x) for y in rows for x in cols]


def _warp_ref(img, X, Y, fx, fy):
    """atm_net.hip's warp3 of image [H,W,cs] (device) at pixel (X, Y) with flow (fx, fy): position and weights in fp32 as the kernel computes
    them, the four taps summed in float64 -> 3 channel values"""
    f32 = np.float32
    H, W = img.shape[0], img.shape[1]
    gx = f32(2.0) * (f32(X) + f32(fx)) / f32(W - 1) - f32(1.0)
    gy = f32(2.0) * (f32(Y) + f32(fy)) / f32(H - 1) - f32(1.0)
    gx, gy = min(max(gx, f32(-4.0)), f32(4.0)), min(max(gy, f32(-4.0)), f32(4.0))
    px, py = ((gx + f32(1.0)) / f32(2.0)) * f32(W - 1), ((gy + f32(1.0)) / f32(2.0)) * f32(H - 1)
    x0, y0 = int(np.floor(px)), int(np.floor(py))
    wx, wy = f32(px - f32(x0)), f32(py - f32(y0))
    e, s = f32(1.0) - wx, f32(1.0) - wy
    val = np.zeros(3)
    for yy, xx, wgt in ((y0, x0, e * s), (y0, x0 + 1, wx * s), (y0 + 1, x0, e * wy), (y0 + 1, x0 + 1, wx * wy)):
        if 0 <= xx < W and 0 <= yy < H:
            val += img[yy, xx, :3].double().cpu().numpy() * float(wgt)
    return val


@pytest.fixture(scope="module")
def refine_input_4k(hip_lib):
    """vfi_atm_blend_warps as ATM-base's forward calls it at 2160x3840: the 120-float refinement input (4 010 803 200 bytes) holds the motion
    (channels 96..100) and receives the 15 synthesis channels (101..115).  Shared by two tests."""
    rcs, fc = 120, 101
    torch.manual_seed(21)
    src = torch.rand((2, HP, WP, 8), device="cuda")
    orig = torch.rand((2, HP, WP, 8), device="cuda")
    R_ = torch.full((HP, WP, rcs), float("nan"), device="cuda")
    assert R_.numel() * 4 == 4010803200
    R_[..., fc - 5:fc - 1] = torch.randn((HP, WP, 4), device="cuda") * 3.0
    R_[..., fc - 1] = torch.randn((HP, WP), device="cuda") * 2.0
    base = R_.data_ptr()
    _ck(hip_lib.vfi_atm_blend_warps(src.data_ptr(), src.data_ptr() + 4 * HP * WP * 8, 8, orig.data_ptr(), orig.data_ptr() + 4 * HP * WP * 8, 8,
                                    base + 4 * (fc - 5), rcs, base + 4 * fc, rcs, HP, WP, None), "blend_warps")
    torch.cuda.synchronize()
    yield dict(R=R_, src=src, orig=orig, rcs=rcs, fc=fc)
    del R_, src, orig
    torch.cuda.empty_cache()


def test_blend_at_4k(refine_input_4k):
    u = refine_input_4k
    R_, src, orig, fc = u["R"], u["src"], u["orig"], u["fc"]
    assert not bool(torch.isnan(R_[-1, :, fc - 5:fc + 15]).any()) and not bool(torch.isnan(R_[0, :, fc - 5:fc + 15]).any())
    assert bool(torch.isnan(R_[-1, :, :fc - 5]).all()) and bool(torch.isnan(R_[-1, :, fc + 15:]).all()), "a channel beside the 15 was written"
    worst = 0.0
    for Y, X in _sample_pixels(HP, WP, WP * u["rcs"] * 4):
        px = R_[Y, X].double().cpu().numpy()
        mo, got = px[fc - 5:fc], px[fc:fc + 15]
        assert np.array_equal(got[0:3], orig[0, Y, X, :3].double().cpu().numpy()) and np.array_equal(got[6:9], orig[1, Y, X, :3].double().cpu().numpy()), (Y, X)
        w0, w1 = _warp_ref(src[0], X, Y, mo[0], mo[1]), _warp_ref(src[1], X, Y, mo[2], mo[3])
        m = 1.0 / (1.0 + np.exp(-mo[4]))
        want = np.concatenate([w0, w1, m * w0 + (1.0 - m) * w1])
        have = np.concatenate([got[3:6], got[9:12], got[12:15]])
        tol = np.concatenate([np.full(6, 7 * U), np.full(3, 27 * U)])      # max|x| = 1: the sources are in [0, 1)
        ratio = float((np.abs(have - want) / tol).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (Y, X, have, want)
    print(f"blend 2176x3840 into the 120-float buffer: max err / bound = {worst:.3f}")


def test_out_at_4k(hip_lib, refine_input_4k):
    """vfi_atm_refine_out reads I_t out of the 4.01 GB buffer (channels 113..115, stride 120) and crops 2176 -> 2160 rows"""
    u = refine_input_4k
    R_, rcs, fc = u["R"], u["rcs"], u["fc"]
    H, W, top = 2160, 3840, 8
    torch.manual_seed(22)
    res = torch.randn((HP, WP, 8), device="cuda") * 2
    out = torch.full((H, W, 3), float("nan"), device="cuda")
    _ck(hip_lib.vfi_atm_refine_out(R_.data_ptr() + 4 * (fc + 12), rcs, res.data_ptr(), 8, out.data_ptr(), HP, WP, top, 0, H, W, None), "refine_out")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())
    worst = 0.0
    for Yp, X in _sample_pixels(HP, WP, WP * rcs * 4):
        Y = min(max(Yp - top, 0), H - 1)
        it = R_[Y + top, X, fc + 12:fc + 15].double().cpu().numpy()
        r = res[Y + top, X, :3].double().cpu().numpy()
        want = np.clip(it + 2.0 / (1.0 + np.exp(-r)) - 1.0, 0.0, 1.0)
        got = out[Y, X].double().cpu().numpy()
        tol = 20 * U * (1.0 + np.abs(it))
        ratio = float((np.abs(got - want) / tol).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (Y, X, got, want)
    print(f"out 2160x3840 from the 120-float buffer: max err / bound = {worst:.3f}")


def test_depth_to_space_at_4k(hip_lib):
    """ATM-base's last up-sampling level: taps [1088, 1920, 408] (3 409 182 720 bytes) -> [2176, 3840, 104] (3 476 029 440 bytes), 101
    channels; a copy, so every element is compared (on the device)."""
    h, w, c, ics, ocs = HP // 2, WP // 2, 101, 408, 104
    torch.manual_seed(23)
    src = torch.randn((h, w, ics), device="cuda")
    dst = torch.full((2 * h, 2 * w, ocs), float("nan"), device="cuda")
    assert src.numel() * 4 == 3409182720 and dst.numel() * 4 == 3476029440
    _ck(hip_lib.vfi_atm_depth_to_space2(src.data_ptr(), ics, dst.data_ptr(), ocs, 1, h, w, c, None), "depth_to_space2")
    torch.cuda.synchronize()
    v = dst.view(h, 2, w, 2, ocs)
    for ky in (0, 1):
        for kx in (0, 1):
            t = 2 * ky + kx
            assert torch.equal(v[:, ky, :, kx, :c], src[..., t * c:(t + 1) * c]), (ky, kx)
            assert bool(torch.isnan(v[:, ky, :, kx, c:]).all()), "a channel beyond the 101 was written"


# ---- 4. limits ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["lite", "base"])
def test_limits_with_the_key_on_and_off(hip_lib, keys_off, variant, monkeypatch):
    from cfi_amd import _lib, atm, ckpt

    off, on = LIMITS[variant]
    first_refused = (3328, 4096) if variant == "lite" else (2048, 4096)
    eng = _engine(variant)
    tiny = torch.zeros(64, 64, 3, device="cuda")
    try:
        assert eng.max_padded_pixels() == off == hip_lib.vfi_atm_object_max_padded_pixels(eng.handle) == atm.max_padded_pixels(variant)
        eng.forward(tiny, tiny, True)
        before = eng.workspace_bytes()
        assert before > 0
        rc = hip_lib.vfi_atm_forward(eng.handle, tiny.data_ptr(), tiny.data_ptr(), 3, 2176, 3840, 1, tiny.data_ptr(), None)
        assert rc != 0 and "size limit" in _lib.last_error() and "2 GiB" in _lib.last_error()
        assert eng.workspace_bytes() == before
        # key on
        monkeypatch.setattr(ckpt, "load_config", _config(atm_large_frames=True))
        assert eng.max_padded_pixels() == on == hip_lib.vfi_atm_large_max_padded_pixels(atm.VARIANTS.index(variant)) == atm.max_padded_pixels(variant)
        assert hip_lib.vfi_atm_object_max_padded_pixels(eng.handle) == on
        with pytest.raises(ValueError, match="index arithmetic"):
            big = torch.empty(first_refused + (3,), device="cuda")
            eng.forward(big, big, True)
        # the C entry points themselves: the size is checked before the frames are touched (64x64 buffers stand behind the claim)
        rc = hip_lib.vfi_atm_forward(eng.handle, tiny.data_ptr(), tiny.data_ptr(), 3, *first_refused, 1, tiny.data_ptr(), None)
        assert rc != 0 and "size limit" in _lib.last_error() and "with large frames on" in _lib.last_error() and "4 GiB" in _lib.last_error()
        rc = hip_lib.vfi_atm_forward_ensemble(eng.handle, tiny.data_ptr(), tiny.data_ptr(), 3, *first_refused, tiny.data_ptr(), None)
        assert rc != 0 and "4 GiB" in _lib.last_error()
        assert eng.workspace_bytes() == before
        # and off again: read at call time
        monkeypatch.setattr(ckpt, "load_config", _config())
        assert eng.max_padded_pixels() == off
        rc = hip_lib.vfi_atm_forward(eng.handle, tiny.data_ptr(), tiny.data_ptr(), 3, 2176, 3840, 1, tiny.data_ptr(), None)
        assert rc != 0 and "size limit" in _lib.last_error() and "2 GiB" in _lib.last_error()
        assert eng.workspace_bytes() == before
    finally:
        eng.close()
