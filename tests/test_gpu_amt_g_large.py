"""AMT-G on frames up to 12 201 611 padded pixels (config.yaml's ``amt_large_frames``), on the device.

1. Forced, through the net: with the key on and the test option large_image_bytes at 1 byte every layer of the forward that has a large-image
   form takes it; every golden case of tests/golden/amt_g_net.npz comes out bit-identical to a default engine, and the log of LARGE launches
   (vfi_test_large_launches) holds decoder1's five ResBlock layers, the residual + PReLU one among them.  AMT-S / AMT-L with the switch on:
   bit-identical, and the same launches as with it off (the switch sets nothing on them).
2. 2160x3840, seeded weights, one pair, t = 0.5: shape, finite, a replay bit-identical, the workspace figure and the set of LARGE layers of
   docs/design/amt.md ("4K"); without the switch the same call is refused before any launch.  (The comparison with the host restatement at
   this size is tools/amt_bench.py --uhd --parity's.)
3. AMT's own kernels at buffers of 2 GiB and more, one call each at 1408x2160 (the half resolution of 2816x4320, next to the limit) and at
   the width the net uses there.  amt_add_kernel through the test tap vfi_test_amt_add (include/vfi_hip_test_amt.h): the copy of dec_in's
   first 84 channels into the window at +192 of the 280-float upd_in, the in-place sum dec_in += dn, the reps form, the stride-2 copy;
   all compared exactly on the device.  amt_warp_kernel through vfi_test_amt_warp: a pyramid level warped by the flow window at +252 of
   dec_in into its window at +84.  vfi_amt_upsample_lrelu, vfi_conv7x7 on that flow window, vfi_resize_bilinear_ratio.  The last four are
   sampled in the last rows and around the row where the byte offset crosses 2^31, against float64.  One forward next to the limit.
4. The limits from a live object, switch on and off, S / L / G, against amt.py's constants.

Bounds, u = 2^-24 (the style of tests/test_gpu_atm_large.py).
  upsample   GAMMA_UPSAMPLE = 6 roundings over M = sum |term| (tests/amt_g_restated.py derives it: weights exact for scale 2 and 4, two
             products, two sums, the slope): |d| <= 6 u M.
  resize     the taps' weights come from one fp32 chain shared by kernel and restatement (bil_src); the blend is w0 (w0' a + w1' b) +
             w1 (w0' c + w1' d): 4 products and 2 sums inside, 2 products and a sum outside, then post_mul: 10 roundings of values whose
             magnitudes sum to <= M = max |tap| * post_mul: |d| <= 10 u M, asked with the weights restated in float64 from the kernel's ratio
             (their own rounding, 2 u relative each on two levels, adds 4 u M): 14 u M.
  conv7x7    49 Cin + 3 roundings over M = sum |term|, as tests/test_gpu_amt.py: Cin = 4 -> 199 u M.
  add        one fp32 addition per element, correctly rounded: the result IS torch's a + b in fp32, so it is compared with torch.equal.
  warp       the sampling position goes through the same fp32 chain in kernel and restatement (rife_warp.h: warp_taps; the file is built
             without contraction), the corner weights are fp32 products of exact differences, restated alike; an output is 4 products
             and 3 additions over M = sum weight |tap|: 7 u M.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import amt_restated
import cain_restated
from amt_g_restated import GAMMA_UPSAMPLE, SEED
from amt_restated import NET_SHAPES, NET_STRIDE, NET_TS, TOL, frames_of
from cfi_amd import ckpt as _ckpt

_REAL_CONFIG = _ckpt.load_config      # the package's own config.yaml, whatever a test has patched in since

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TWO31 = 2 ** 31
LARGE_DEFAULT = 2 ** 31 - 1
GEN2, WINO = 2, 3
G_OFF, G_ON, SL = 6100805, 12201611, 2 ** 23 - 1
H4, W4 = 2160, 3840
# docs/design/amt.md, "4K": the workspace of one 2160x3840 pair after one single-timestep forward on a fresh AMT-G object
WORKSPACE_BYTES_4K = 53794592784
# ... and the layers that meet an input image of 2 GiB or more there, as the LARGE log names them (family, Hin, Win, in_cs, Cin_p, Cout):
# decoder1's rb[1] / rb[3] (the 84 side channels out of the 352-float pixel), rb[2] / rb[4] (the whole pixel; rb[4] is residual + PReLU),
# update2_high's gru.0 (the 280-float upd_in).  rb[0] reads the 256-float dec_r0, 2 123 366 400 bytes: just below the mark.
LARGE_LAYERS_4K = {(WINO, H4 // 2, W4 // 2, 352, 88, 84), (WINO, H4 // 2, W4 // 2, 352, 352, 252), (WINO, H4 // 2, W4 // 2, 280, 280, 192)}
# next to the limit: 2816x4320 = 12 165 120 padded pixels (both sides multiples of 16, so the pad adds nothing)
HL, WL = 2816, 4320


def _ck(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


def _large_log(lib):
    buf = (C.c_int32 * (6 * 256))()
    n = lib.vfi_test_large_launches(buf, 256)
    return [tuple(buf[6 * i:6 * i + 6]) for i in range(min(n, 256))]


def _config(**keys):
    return lambda: dict(_REAL_CONFIG(), amt_g=True, **keys)


@pytest.fixture
def keys_off(monkeypatch):
    from cfi_amd import ckpt

    monkeypatch.setattr(ckpt, "load_config", _config())


def _engine(variant):
    from cfi_amd import amt, amt_spec

    return amt.AmtEngine(amt_spec.seeded_state_dict(variant, SEED))


def hwc(f):
    return f[0].permute(1, 2, 0).contiguous().cuda()


# ---- 1. forced, through the net --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", sorted(NET_SHAPES))
def test_forced_large_path_through_the_net_is_bit_identical(hip_lib, keys_off, shape, golden_dir, monkeypatch):
    from cfi_amd import amt, ckpt

    golden = np.load(os.path.join(golden_dir, "amt_g_net.npz"))
    f0, f1 = frames_of(shape)
    h, w = f0.shape[2:]
    hp, wp = amt.padded_size(h, w)
    plain = _engine("G")
    try:
        want = plain.forward(hwc(f0), hwc(f1), NET_TS).clone()
        torch.cuda.synchronize()
        assert plain.max_padded_pixels() == G_OFF
        with monkeypatch.context() as mp:
            mp.setattr(ckpt, "load_config", _config(amt_large_frames=True))
            forced = _engine("G")      # created with the key on: the engine gives the object the switch
            try:
                assert hip_lib.vfi_amt_object_max_padded_pixels(forced.handle) == G_ON
                assert hip_lib.vfi_test_set_option(b"large_image_bytes", 1) == 0
                try:
                    got = forced.forward(hwc(f0), hwc(f1), NET_TS).clone()
                    torch.cuda.synchronize()
                    _large_log(hip_lib)      # the log keeps 256 launches: one timestep's worth is read, of a call of its own
                    forced.forward(hwc(f0), hwc(f1), NET_TS[:1])
                    torch.cuda.synchronize()
                    log = _large_log(hip_lib)
                finally:
                    hip_lib.vfi_test_set_option(b"large_image_bytes", LARGE_DEFAULT)
            finally:
                forced.close()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"AMT-G {shape}: the large path differs from the default path"
        for i, t in enumerate(NET_TS):
            d, sums_ok = cain_restated.compare(got[i].cpu(), golden, f"G_{shape}_t{t}_", NET_STRIDE, TOL)
            assert d <= TOL and sums_ok, (shape, t, d, sums_ok)
        # decoder1's ResBlock at half resolution: rb[0] (dec_r0, 256 floats -> 252), rb[1] / rb[3] (84 of the 352-float pixel), rb[2] / rb[4]
        # (the whole 352-float pixel -> 252; rb[4] with the residual), once per timestep each
        h2, w2 = hp // 2, wp // 2
        count = {k: sum(1 for e in log if e[1:] == k) for k in ((h2, w2, 256, 256, 252), (h2, w2, 352, 88, 84), (h2, w2, 352, 352, 252))}
        n = 1
        assert len(log) < 256, "the log is full: its tail, where decoder1 runs, is missing"
        # (dec_in is 256 floats wide as well, and decoder1's c0 maps it to the same 252 channels: c0 and rb[0] share an entry)
        assert count[(h2, w2, 256, 256, 252)] == 2 * n and count[(h2, w2, 352, 88, 84)] == 2 * n and count[(h2, w2, 352, 352, 252)] == 2 * n, \
            f"AMT-G {shape}: decoder1's ResBlock layers in the LARGE log: {count}; the log has {len(log)}: {sorted(set(log))}"
        print(f"AMT-G {shape}: {len(log)} LARGE launches, {len(set(log))} distinct")
    finally:
        plain.close()


def test_forced_without_the_switch_keeps_the_residual_prelu_layers_plain(hip_lib, keys_off):
    """An AMT-G object as created, under the forced mark: the layers that take a large form on their own do, residual + PReLU does not — the
    log holds rb[2] once per timestep where the switched object has rb[2] and rb[4] — and the bits are the same."""
    f0, f1 = frames_of("128x128")
    eng = _engine("G")
    try:
        want = eng.forward(hwc(f0), hwc(f1), [0.5]).clone()
        assert hip_lib.vfi_test_set_option(b"large_image_bytes", 1) == 0
        try:
            _large_log(hip_lib)
            got = eng.forward(hwc(f0), hwc(f1), [0.5]).clone()
            torch.cuda.synchronize()
            log = _large_log(hip_lib)
        finally:
            hip_lib.vfi_test_set_option(b"large_image_bytes", LARGE_DEFAULT)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert sum(1 for e in log if e[1:] == (64, 64, 352, 352, 252)) == 1, sorted(set(log))
    finally:
        eng.close()


@pytest.mark.parametrize("variant", ["S", "L"])
def test_s_and_l_with_the_switch_on_launch_what_they_launched(hip_lib, keys_off, variant, golden_dir, monkeypatch):
    """Bit-identical golden cases and the same LARGE log (forced mark, so that a permission given by mistake would show) as with it off"""
    from cfi_amd import ckpt

    golden = np.load(os.path.join(golden_dir, "amt_net.npz"))
    runs = {}
    for key in (False, True):
        with monkeypatch.context() as mp:
            mp.setattr(ckpt, "load_config", _config(amt_large_frames=key))
            eng = _engine(variant)
            try:
                assert eng.max_padded_pixels() == SL == hip_lib.vfi_amt_object_max_padded_pixels(eng.handle)
                outs, logs = [], []
                for mark in (LARGE_DEFAULT, 1):
                    assert hip_lib.vfi_test_set_option(b"large_image_bytes", mark) == 0
                    try:
                        for shape in sorted(NET_SHAPES):
                            f0, f1 = frames_of(shape)
                            _large_log(hip_lib)
                            outs.append(eng.forward(hwc(f0), hwc(f1), NET_TS).cpu())
                            logs.append(_large_log(hip_lib))
                    finally:
                        hip_lib.vfi_test_set_option(b"large_image_bytes", LARGE_DEFAULT)
                runs[key] = (outs, logs)
            finally:
                eng.close()
    for a, b in zip(runs[False][0], runs[True][0]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"AMT-{variant}: the switch moved a bit"
    assert runs[False][1] == runs[True][1], f"AMT-{variant}: the switch changed the LARGE launches"
    assert all(not lg for lg in runs[True][1][:len(NET_SHAPES)]), "a LARGE launch under the default mark at golden sizes"
    for k, shape in enumerate(sorted(NET_SHAPES)):
        for i, t in enumerate(NET_TS):
            d, sums_ok = cain_restated.compare(runs[True][0][k][i], golden, f"{variant}_{shape}_t{t}_", NET_STRIDE, TOL)
            assert d <= TOL and sums_ok, (variant, shape, t, d)


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


def test_4k_forward(hip_lib, keys_off, monkeypatch):
    from cfi_amd import _lib, amt, ckpt

    assert amt.padded_size(H4, W4) == (H4, W4) and G_OFF < H4 * W4 <= G_ON
    torch.cuda.empty_cache()
    f0, f1 = _smooth_pair(H4, W4)
    eng = _engine("G")
    out = torch.empty((1, H4, W4, 3), device="cuda")
    ts = (C.c_float * 1)(0.5)
    try:
        # without the key: refused by the engine and by the C entry point, nothing allocated
        with pytest.raises(ValueError, match="amt_large_frames"):
            eng.forward(f0, f1, [0.5])
        rc = hip_lib.vfi_amt_forward(eng.handle, f0.data_ptr(), f1.data_ptr(), 3, H4, W4, ts, 1, out.data_ptr(), None)
        assert rc != 0 and "size limit of AMT-G" in _lib.last_error() and "2 GiB" in _lib.last_error(), _lib.last_error()
        assert eng.workspace_bytes() == 0
        monkeypatch.setattr(ckpt, "load_config", _config(amt_large_frames=True))
        _large_log(hip_lib)
        a = eng.forward(f0, f1, [0.5]).clone()
        torch.cuda.synchronize()
        log = _large_log(hip_lib)
        ws = eng.workspace_bytes()
        print(f"AMT-G 2160x3840 t = 0.5: workspace {ws} bytes; LARGE launches {log}")
        assert a.shape == (1, H4, W4, 3) and bool(torch.isfinite(a).all())
        assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0 and float(a.std()) > 0.01
        b = eng.forward(f0, f1, [0.5])
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the same pair twice differs"
        assert set(log) == LARGE_LAYERS_4K, (sorted(set(log)), sorted(LARGE_LAYERS_4K))
        assert ws == WORKSPACE_BYTES_4K, ws
    finally:
        eng.close()


# ---- 3. AMT's own kernels at buffers of 2 GiB and more -----------------------------------------------------------------------------------------

def test_forward_next_to_the_limit(hip_lib, keys_off, monkeypatch):
    """2816x4320: the half-resolution 256-float buffers (dec_in, dec_r0, dec_r5, upd_cf, updh_c1) hold 3 114 270 720 bytes here, so the net's
    own amt_add (copies into upd_in's windows, the sums into dec_in), amt_warp (into dec_in's windows) and the transposed convolution's input
    cross 2 GiB as well.  Shape, finiteness, a bit-identical replay, and the layers the log must at least hold."""
    from cfi_amd import amt, ckpt

    assert amt.padded_size(HL, WL) == (HL, WL) and HL * WL == 12165120 <= G_ON < (HL + 16) * WL
    assert (HL // 2) * (WL // 2) * 256 * 4 == 3114270720 >= TWO31
    torch.cuda.empty_cache()
    f0, f1 = _smooth_pair(HL, WL)
    monkeypatch.setattr(ckpt, "load_config", _config(amt_large_frames=True))
    eng = _engine("G")
    try:
        _large_log(hip_lib)
        a = eng.forward(f0, f1, [0.5]).clone()
        torch.cuda.synchronize()
        log = _large_log(hip_lib)
        print(f"AMT-G {HL}x{WL} t = 0.5: workspace {eng.workspace_bytes()} bytes; LARGE launches {sorted(set(log))}")
        assert a.shape == (1, HL, WL, 3) and bool(torch.isfinite(a).all()) and float(a.std()) > 0.01
        b = eng.forward(f0, f1, [0.5])
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the same pair twice differs"
        h2, w2 = HL // 2, WL // 2
        need = {(h2, w2, 352, 88, 84), (h2, w2, 352, 352, 252), (h2, w2, 280, 280, 192),      # as at 2160x3840
                (h2, w2, 256, 256, 252),                                                        # decoder1's c0 (dec_in) and rb[0] (dec_r0)
                (h2, w2, 256, 256, 188),                                                        # update2_high's conv over upd_cf
                (h2, w2, 256, 256, 192)}                                                        # ... and its convc2 over updh_c1
        have = {e[1:] for e in log}
        assert need <= have, (sorted(need - have), sorted(have))
    finally:
        eng.close()


H2, W2 = HL // 2, WL // 2      # 1408 x 2160: the half-resolution map next to the limit


def _sample_pixels(Hh, Ww, row_bytes):
    cross = TWO31 // row_bytes
    rows = [0, cross - 1, cross, cross + 1, Hh - 2, Hh - 1]
    cols = [0, 1, Ww // 2 - 1, Ww // 2, (TWO31 % row_bytes) // (row_bytes // Ww), Ww - 2, Ww - 1]
    return [(y, x) for y in rows for x in cols]


def _bil(o, ratio, n):
    """csrc/bilinear_src.h: source taps and weights of output index o (torch's align_corners=False rule), the position in fp32 as the kernel"""
    f32 = np.float32
    s = max(f32(ratio) * (f32(o) + f32(0.5)) - f32(0.5), f32(0.0))
    i0 = min(int(s), n - 1)
    i1 = min(i0 + 1, n - 1)
    w1 = float(f32(s) - f32(i0))
    return i0, i1, 1.0 - w1, w1


def test_upsample_lrelu_into_a_buffer_over_2_gib(hip_lib):
    """update2_high's convc1 output, [352, 540, 256] at 1/8 resolution, up-sampled x4 into updh_c1 [1408, 2160, 256] (3.11 GB)"""
    h8, w8, c = H2 // 4, W2 // 4, 256
    torch.manual_seed(31)
    src = torch.randn((h8, w8, c), device="cuda")
    dst = torch.full((H2, W2, c), float("nan"), device="cuda")
    assert dst.numel() * 4 == 3114270720
    _ck(hip_lib.vfi_amt_upsample_lrelu(src.data_ptr(), c, dst.data_ptr(), c, 1, h8, w8, c, 4, C.c_float(0.1), None), "upsample_lrelu")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dst[-1]).any()) and not bool(torch.isnan(dst[0]).any())
    worst = 0.0
    for Y, X in _sample_pixels(H2, W2, W2 * c * 4):
        y0, y1, wy0, wy1 = _bil(Y, 0.25, h8)
        x0, x1, wx0, wx1 = _bil(X, 0.25, w8)
        a, b, cc, d = (src[yy, xx].double().cpu().numpy() for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
        v = wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * cc + wx1 * d)
        M = wy0 * (wx0 * np.abs(a) + wx1 * np.abs(b)) + wy1 * (wx0 * np.abs(cc) + wx1 * np.abs(d))
        want = np.where(v > 0, v, 0.1 * v)
        got = dst[Y, X].double().cpu().numpy()
        ratio = float((np.abs(got - want) / (GAMMA_UPSAMPLE * U * M + 1e-300)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (Y, X)
    print(f"upsample x4 into [1408, 2160, 256]: max err / bound = {worst:.3f}")


@pytest.fixture(scope="module")
def dec_in_at_the_limit(hip_lib):
    """dec_in of decoder1 next to the limit: [1408, 2160, 256] (3.11 GB), random values in every channel; shared by the two tests below"""
    torch.manual_seed(32)
    t = torch.randn((H2, W2, 256), device="cuda")
    assert t.numel() * 4 == 3114270720
    yield t
    del t
    torch.cuda.empty_cache()


def test_conv7x7_on_the_flow_window_of_a_256_float_pixel(hip_lib, dec_in_at_the_limit):
    """update2_high's convf1: 4 -> 128, LeakyReLU, reading the flow window at +252 of dec_in"""
    din = dec_in_at_the_limit
    g = torch.Generator().manual_seed(33)
    w = (torch.rand(128, 4, 7, 7, generator=g) * 2 - 1) / 14.0
    b = torch.rand(128, generator=g) - 0.5
    wp = amt_restated.pack7x7(w).cuda()
    bd = b.cuda()
    out = torch.full((H2, W2, 128), float("nan"), device="cuda")
    _ck(hip_lib.vfi_conv7x7(din.data_ptr() + 4 * 252, 256, wp.data_ptr(), bd.data_ptr(), None, C.c_float(0.1), 1, 4, 128, out.data_ptr(), 128, 1, H2, W2, None),
        "conv7x7")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[-1]).any()) and not bool(torch.isnan(out[0]).any())
    worst = 0.0
    for Y, X in _sample_pixels(H2, W2, W2 * 256 * 4):
        patch = torch.zeros(4, 7, 7, dtype=torch.float64)
        ya, yb, xa, xb = max(Y - 3, 0), min(Y + 4, H2), max(X - 3, 0), min(X + 4, W2)
        patch[:, ya - (Y - 3):yb - (Y - 3), xa - (X - 3):xb - (X - 3)] = din[ya:yb, xa:xb, 252:256].double().cpu().permute(2, 0, 1)
        v = (w.double() * patch).sum((1, 2, 3)) + b.double()
        M = (w.double().abs() * patch.abs()).sum((1, 2, 3)) + b.double().abs()
        want = torch.where(v > 0, v, 0.1 * v)
        got = out[Y, X].double().cpu()
        ratio = float(((got - want).abs() / ((49 * 4 + 3) * U * M)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (Y, X)
    print(f"conv7x7 4 -> 128 from the window at +252 of [1408, 2160, 256]: max err / bound = {worst:.3f}")


def test_resize_out_of_a_256_float_pixel(hip_lib, dec_in_at_the_limit):
    """The flow's way up (amt_forward: resize(din + 3 ch, ..., 0.5, 2.0)): 4 channels at +252 of dec_in -> [2816, 4320, 4], times 2"""
    din = dec_in_at_the_limit
    out = torch.full((HL, WL, 4), float("nan"), device="cuda")
    _ck(hip_lib.vfi_resize_bilinear_ratio(din.data_ptr() + 4 * 252, 256, out.data_ptr(), 4, 1, H2, W2, HL, WL, 4, C.c_float(0.5), C.c_float(0.5), C.c_float(2.0), None),
        "resize_bilinear_ratio")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())
    worst = 0.0
    for y, x in _sample_pixels(H2, W2, W2 * 256 * 4):
        for Y, X in ((2 * y, 2 * x), (2 * y + 1, 2 * x + 1)):
            y0, y1, wy0, wy1 = _bil(Y, 0.5, H2)
            x0, x1, wx0, wx1 = _bil(X, 0.5, W2)
            a, b, cc, d = (din[yy, xx, 252:256].double().cpu().numpy() for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
            want = 2.0 * (wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * cc + wx1 * d))
            M = 2.0 * max(np.abs(a).max(), np.abs(b).max(), np.abs(cc).max(), np.abs(d).max())
            got = out[Y, X].double().cpu().numpy()
            ratio = float((np.abs(got - want) / (14 * U * M)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (Y, X, got, want)
    print(f"resize x2 of the window at +252 of [1408, 2160, 256]: max err / bound = {worst:.3f}")


def test_add_kernel_copies_and_sums_at_buffers_over_2_gib(hip_lib, dec_in_at_the_limit):
    """amt_add_kernel as the forward calls it in update2_high next to the limit, every result compared exactly on the device"""
    din = dec_in_at_the_limit
    ch = 84
    # 1. Run::copy: dec_in's first 84 channels into the window at +192 of upd_in (280 floats: 3 406 233 600 bytes)
    upd = torch.full((H2, W2, 280), float("nan"), device="cuda")
    assert upd.numel() * 4 == 3406233600
    _ck(hip_lib.vfi_test_amt_add(din.data_ptr(), 256, W2, 1, None, 0, upd.data_ptr() + 4 * 192, 280, H2, W2, ch, 1, None), "amt_add (copy)")
    torch.cuda.synchronize()
    assert torch.equal(upd[..., 192:192 + ch], din[..., :ch]), "the copy differs"
    assert bool(torch.isnan(upd[..., :192]).all()) and bool(torch.isnan(upd[..., 192 + ch:]).all()), "a channel beside the window was written"
    del upd
    # 2. the stride-2 copy in front of a 1x1 stride-2 layer, out of the 3.11 GB buffer
    sub = torch.full((H2 // 2, W2 // 2, 64), float("nan"), device="cuda")
    _ck(hip_lib.vfi_test_amt_add(din.data_ptr(), 256, W2, 2, None, 0, sub.data_ptr(), 64, H2 // 2, W2 // 2, 64, 1, None), "amt_add (stride 2)")
    torch.cuda.synchronize()
    assert torch.equal(sub, din[::2, ::2, :64]), "the stride-2 copy differs"
    del sub
    # 3. in place, dec_in[.., :84] += dn (88-float pixels), and 4. the reps form on the flow window: dec_in[.., 252 + 2 r + c] += up[.., c]
    work = din.clone()
    torch.manual_seed(34)
    dn = torch.randn((H2, W2, 88), device="cuda")
    up = torch.randn((H2, W2, 4), device="cuda")
    _ck(hip_lib.vfi_test_amt_add(work.data_ptr(), 256, W2, 1, dn.data_ptr(), 88, work.data_ptr(), 256, H2, W2, ch, 1, None), "amt_add (sum)")
    _ck(hip_lib.vfi_test_amt_add(work.data_ptr() + 4 * 252, 256, W2, 1, up.data_ptr() + 4 * 2, 4, work.data_ptr() + 4 * 252, 256, H2, W2, 2, 2, None), "amt_add (reps)")
    torch.cuda.synchronize()
    assert torch.equal(work[..., :ch], din[..., :ch] + dn[..., :ch]), "the sum differs from the fp32 addition"
    assert torch.equal(work[..., 252:256], din[..., 252:256] + up[..., 2:4].repeat(1, 1, 2)), "the reps form differs"
    assert torch.equal(work[..., ch:252], din[..., ch:252]), "a channel beside the windows was written"
    del work, dn, up
    torch.cuda.empty_cache()


def _warp_ref(img, X, Y, fx, fy, C_):
    """rife_warp.h's warp_taps at pixel (X, Y) of an [H, W, cs] image with flow (fx, fy): position and weights in fp32 as the kernel computes
    them, the four taps summed in float64 -> (C_ values, M = sum weight |tap|)"""
    f32 = np.float32
    H, W = img.shape[0], img.shape[1]

    def lin11(i, n, step):
        return f32(-1.0) + step * f32(i) if i < n // 2 else f32(1.0) - step * f32(n - 1 - i)

    stepx, stepy = f32(2.0) / f32(W - 1), f32(2.0) / f32(H - 1)
    halfw, halfh = f32((W - 1.0) / 2.0), f32((H - 1.0) / 2.0)
    nx, ny = lin11(X, W, stepx) + f32(fx) / halfw, lin11(Y, H, stepy) + f32(fy) / halfh
    px, py = (nx + f32(1.0)) * halfw, (ny + f32(1.0)) * halfh
    px, py = min(f32(W - 1), max(px, f32(0.0))), min(f32(H - 1), max(py, f32(0.0)))
    x0f, y0f = np.floor(px), np.floor(py)
    w, n = f32(px - x0f), f32(py - y0f)
    e, s = f32(1.0) - w, f32(1.0) - n
    x0, y0 = int(x0f), int(y0f)
    x1, y1 = x0 + (1 if x0 < W - 1 else 0), y0 + (1 if y0 < H - 1 else 0)
    val, M = np.zeros(C_), np.zeros(C_)
    for yy, xx, wgt in ((y0, x0, s * e), (y0, x1, s * w), (y1, x0, n * e), (y1, x1, n * w)):
        t = img[yy, xx, :C_].double().cpu().numpy()
        val += t * float(f32(wgt))
        M += np.abs(t) * float(f32(wgt))
    return val, M


def test_warp_kernel_into_a_window_of_a_buffer_over_2_gib(hip_lib):
    """decoder1's input next to the limit: warp(pyramid level 0 (88-float pixels), flow0) into the window at +84 of dec_in, the flow read from
    its window at +252 — both in the 3.11 GB buffer"""
    ch = 84
    torch.manual_seed(35)
    pyr = torch.randn((H2, W2, 88), device="cuda")
    din = torch.full((H2, W2, 256), float("nan"), device="cuda")
    din[..., 252:256] = torch.randn((H2, W2, 4), device="cuda") * 3.0
    assert din.numel() * 4 == 3114270720
    _ck(hip_lib.vfi_test_amt_warp(pyr.data_ptr(), 88, din.data_ptr() + 4 * 252, 256, din.data_ptr() + 4 * ch, 256, H2, W2, ch, None), "amt_warp")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(din[..., ch:2 * ch]).any())
    assert bool(torch.isnan(din[..., :ch]).all()) and bool(torch.isnan(din[..., 2 * ch:252]).all()), "a channel beside the window was written"
    worst = 0.0
    for Y, X in _sample_pixels(H2, W2, W2 * 256 * 4):
        fl = din[Y, X, 252:254].cpu().numpy()
        want, M = _warp_ref(pyr, X, Y, fl[0], fl[1], ch)
        got = din[Y, X, ch:2 * ch].double().cpu().numpy()
        ratio = float((np.abs(got - want) / (7 * U * M + 1e-300)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (Y, X)
    print(f"warp into the window at +84 of [1408, 2160, 256]: max err / bound = {worst:.3f}")
    del pyr, din
    torch.cuda.empty_cache()


# ---- 4. limits ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant,off,on", [("S", SL, SL), ("L", SL, SL), ("G", G_OFF, G_ON)])
def test_limits_with_the_key_on_and_off(hip_lib, keys_off, variant, off, on, monkeypatch):
    from cfi_amd import _lib, amt, ckpt

    idx = ("S", "L", "G").index(variant)
    eng = _engine(variant)
    tiny = torch.zeros(128, 128, 3, device="cuda")
    ts = (C.c_float * 1)(0.5)
    first_refused = (2832, 4320) if variant == "G" else (2048, 4096)
    try:
        assert eng.max_padded_pixels() == off == hip_lib.vfi_amt_object_max_padded_pixels(eng.handle) == amt.max_padded_pixels(variant)
        assert off == (amt.MAX_PADDED_PIXELS_G if variant == "G" else amt.MAX_PADDED_PIXELS)
        eng.forward(tiny, tiny, [0.5])
        before = eng.workspace_bytes()
        assert before > 0
        # key on: the node's check follows it at once; the object follows at its next frame over the old limit, or when it is told
        monkeypatch.setattr(ckpt, "load_config", _config(amt_large_frames=True))
        assert amt.max_padded_pixels(variant) == on == hip_lib.vfi_amt_large_max_padded_pixels(idx) and eng.max_padded_pixels() == off
        eng.set_large_frames(True)
        assert eng.max_padded_pixels() == on == hip_lib.vfi_amt_object_max_padded_pixels(eng.handle)
        fresh = _engine(variant)      # an engine created with the key on has the switch from the start
        try:
            assert fresh.max_padded_pixels() == on
        finally:
            fresh.close()
        assert on == (amt.LARGE_MAX_PADDED_PIXELS_G if variant == "G" else amt.MAX_PADDED_PIXELS)
        with pytest.raises(ValueError, match="index arithmetic"):
            big = torch.empty(first_refused + (3,), device="cuda")
            eng.forward(big, big, [0.5])
        # the C entry point itself: the size is checked before the frames are touched (128x128 buffers stand behind the claim)
        rc = hip_lib.vfi_amt_forward(eng.handle, tiny.data_ptr(), tiny.data_ptr(), 3, *first_refused, ts, 1, tiny.data_ptr(), None)
        assert rc != 0 and "size limit" in _lib.last_error()
        assert ("with large frames on" in _lib.last_error() and "4 GiB" in _lib.last_error()) == (variant == "G"), _lib.last_error()
        assert eng.workspace_bytes() == before
        # and off again
        monkeypatch.setattr(ckpt, "load_config", _config())
        eng.set_large_frames(False)
        assert eng.max_padded_pixels() == off == amt.max_padded_pixels(variant)
        if variant == "G":
            rc = hip_lib.vfi_amt_forward(eng.handle, tiny.data_ptr(), tiny.data_ptr(), 3, H4, W4, ts, 1, tiny.data_ptr(), None)
            assert rc != 0 and "size limit" in _lib.last_error() and "2 GiB" in _lib.last_error()
        assert eng.workspace_bytes() == before
    finally:
        eng.close()
