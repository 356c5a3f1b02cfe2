"""-m gpu: AMT-G (config.yaml's ``amt_g``) on the MI355X: the new kernel vfi_amt_upsample_lrelu, vfi_conv7x7 at AMT-G's 4 -> 128,
vfi_conv7x7s2_prelu at 84 output channels, each against float64 between NaN guards; the kernels inside the forward they were written for;
the object (vfi_amt_create variant 2 / AmtEngine) and the node.  Bounds are |got - want| <= gamma * 2^-24 * M, M = sum |term| of the
element, gamma the longest chain of fp32 roundings on the way to it:

  upsample    gamma = 6 (tests/amt_g_restated.py derives it: the weights are exact for scale 2 and 4; two products, two sums, the slope)
  conv7x7     49 Cin + 3, as tests/test_gpu_amt.py (whose test body runs here at 4 -> 128)
  stem        49 * 3 products + bias: gamma = 148, + 1 for the PReLU's product, + 1 spare = 150
  model       per-pixel |d| <= 1e-3, the project's gate, against the reference's own forward (tests/golden/amt_g_net.npz, sampled) and, for
              every pixel, the float64 restatement IN THE REFERENCE'S ORDER (resize, then convc1), while the code under test runs the
              commuted order (convc1 at 1/8 resolution, then vfi_amt_upsample_lrelu)
"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import amt_g_restated
import cain_restated
import test_gpu_amt as base
from amt_g_restated import GAMMA_UPSAMPLE, NET_STRIDE, NET_TS, NODE_CASES, SEED, TOL, config_with
from amt_restated import U, frames_of
from gpu_util import describe_diff, ptr

pytestmark = pytest.mark.gpu
NAN = float("nan")
_check, _bounded, hwc = base._check, base._bounded, base.hwc


@pytest.fixture(scope="module")
def lib(hip_lib):
    from cfi_amd import _lib

    _lib.check(hip_lib.vfi_init(0), "vfi_init")
    return hip_lib


# ---- vfi_amt_upsample_lrelu -------------------------------------------------------------------------------------------------------------

def run_upsample(lib, x, s, slope, in_cs, in_off, out_cs, out_off):
    """x [N,C,h,w] host fp32 -> [N,C,s h,s w] host, through channel windows of NHWC device buffers whose every other element is NaN"""
    N, Cc, h, w = x.shape
    xin = torch.full((N * h * w + 2, in_cs), NAN, device="cuda")
    xin[1:-1, in_off:in_off + Cc] = x.permute(0, 2, 3, 1).reshape(-1, Cc).cuda()
    out = torch.full((N * h * s * w * s + 2, out_cs), NAN, device="cuda")
    _check(lib.vfi_amt_upsample_lrelu(C.c_void_p(xin[1].data_ptr() + 4 * in_off), in_cs, C.c_void_p(out[1].data_ptr() + 4 * out_off), out_cs, N, h, w,
                                      Cc, s, C.c_float(slope), None), "vfi_amt_upsample_lrelu")
    torch.cuda.synchronize()
    win = out[1:-1, out_off:out_off + Cc]
    assert torch.isnan(out[0]).all() and torch.isnan(out[-1]).all() and torch.isnan(out[:, :out_off]).all() and torch.isnan(out[:, out_off + Cc:]).all(), \
        "stray write around the output window"
    return win.reshape(N, h * s, w * s, Cc).permute(0, 3, 1, 2).cpu()


@pytest.mark.parametrize("Cc,in_cs,in_off,out_cs,out_off", [(256, 256, 0, 256, 0), (12, 20, 4, 28, 8), (12, 17, 3, 19, 5)],
                         ids=["C256", "C12_window_float4", "C12_window_scalar"])
@pytest.mark.parametrize("h,w,s", [(2, 3, 4), (9, 13, 2), (17, 16, 4)])
def test_upsample_lrelu_vs_float64(lib, h, w, s, Cc, in_cs, in_off, out_cs, out_off):
    """2x3 at x4: every output touches a clamped edge row or column.  N = 2: the second image must not read the first.  Inputs of both
    signs, so the slope is exercised; the float64 reference is torch's own F.interpolate + leaky_relu on the same values."""
    g = torch.Generator().manual_seed(1000 * h + 10 * w + s + Cc)
    x = torch.randn(2, Cc, h, w, generator=g)
    got = run_upsample(lib, x, s, 0.1, in_cs, in_off, out_cs, out_off)
    want, M = amt_g_restated.upsample_lrelu(x.double(), s, 0.1)
    assert (want < 0).any() and (want > 0).any() and got.shape == (2, Cc, h * s, w * s)
    _bounded(got, want, GAMMA_UPSAMPLE * U * M, f"upsample_lrelu {h}x{w} x{s} C{Cc} window {in_off}/{in_cs} -> {out_off}/{out_cs}")
    assert not torch.equal(got[0], got[1])


def test_upsample_lrelu_refuses_other_scales(lib):
    from cfi_amd import _lib

    x = torch.zeros(64, device="cuda")
    assert lib.vfi_amt_upsample_lrelu(ptr(x), 4, ptr(x), 4, 1, 2, 2, 4, 3, C.c_float(0.1), None) != 0 and "2 or 4" in _lib.last_error()
    assert lib.vfi_amt_upsample_lrelu(ptr(x), 2, ptr(x), 4, 1, 2, 2, 4, 2, C.c_float(0.1), None) != 0


# ---- vfi_conv7x7 at AMT-G's convf1 --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,H,W", [(1, 8, 8), (2, 9, 13), (1, 33, 47)])
def test_conv7x7_4_to_128_vs_float64(lib, N, H, W):
    """tests/test_gpu_amt.py's conv7x7 test (float64, the (49 Cin + 3) bound, NaN guards against stray writes) at 4 -> 128, LeakyReLU"""
    base.test_conv7x7_vs_float64(lib, 4, 128, N, H, W, 1)


def test_conv7x7_refuses_wider_layers(lib):
    from cfi_amd import _lib

    x = torch.zeros(4096, device="cuda")
    assert lib.vfi_conv7x7(ptr(x), 4, ptr(x), None, None, C.c_float(0.1), 1, 4, 129, ptr(x), 129, 1, 2, 2, None) != 0 and "at most 128" in _lib.last_error()


# ---- vfi_conv7x7s2_prelu ------------------------------------------------------------------------------------------------------------------

def run_stem(lib, x, w, b, slopes, out_cs=None):
    """x [N,3,H,W], w [Cout,3,7,7] host fp32 -> [N,Cout,Ho,Wo] host (Cout 64 or 84), NaN behind the channels and around the pixels"""
    N, _, H, W = x.shape
    cout = w.shape[0]
    out_cs = out_cs or cout + 4
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xin = torch.full((N, H, W, 8), NAN, device="cuda")
    xin[..., :3] = x.permute(0, 2, 3, 1).cuda()
    wd = w.permute(2, 3, 1, 0).contiguous().cuda()      # [7][7][3][Cout]
    bd, sd = b.contiguous().cuda(), slopes.contiguous().cuda()
    out = torch.full((N * Ho * Wo + 2, out_cs), NAN, device="cuda")
    _check(lib.vfi_conv7x7s2_prelu(ptr(xin), 8, ptr(wd), ptr(bd), ptr(sd), cout, ptr(out[1]), out_cs, N, H, W, None), "vfi_conv7x7s2_prelu")
    torch.cuda.synchronize()
    assert torch.isnan(out[0]).all() and torch.isnan(out[-1]).all() and torch.isnan(out[:, cout:]).all(), "stray write"
    return out[1:-1, :cout].reshape(N, Ho, Wo, cout).permute(0, 3, 1, 2).cpu()


def stem_case(cout, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(2, 3, H, W, generator=g) * 2 - 1
    w = (torch.rand(cout, 3, 7, 7, generator=g) * 2 - 1) / 147 ** 0.5
    return x, w, torch.rand(cout, generator=g) - 0.5, torch.rand(cout, generator=g) * 0.5


@pytest.mark.parametrize("H,W", [(40, 56), (37, 51)])
def test_stem_84_channels_vs_float64(lib, H, W):
    x, w, b, slopes = stem_case(84, H, W, H * W)
    got = run_stem(lib, x, w, b, slopes)
    want = F.prelu(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=3), slopes.double())
    M = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=2, padding=3)
    assert (want < 0).any() and got.shape == (2, 84, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    _bounded(got, want, 150 * U * M, f"conv7x7s2 3->84 {H}x{W}")


def test_stem_64_channels_keeps_its_bits(lib, golden_dir):
    """The 64-channel instantiation (IFRNet-L's head, AMT-S / AMT-L's stems) is untouched by the 84-channel one: the SHA-256 of its output
    for a seeded input equals the one recorded in tests/golden/amt_g_stem64.npz, which was taken on the device from the parent commit's
    library and from this one's (they agree)."""
    x, w, b, slopes = stem_case(64, 40, 56, 64)
    got = run_stem(lib, x, w, b, slopes, out_cs=64)
    digest = hashlib.sha256(got.contiguous().numpy().tobytes()).hexdigest()
    print("conv7x7s2 3->64 40x56 N=2 sha256", digest)
    assert digest == str(np.load(os.path.join(golden_dir, "amt_g_stem64.npz"))["sha256"])


# ---- the kernels inside the forward they were written for -----------------------------------------------------------------------------------

class GKernelOps(base.KernelOps):
    """amt_g_restated.amt_g_forward's ops: tests/test_gpu_amt.py's (lookup, every 7x7 layer, multi_flow_combine) plus both 7x7 stride-2
    stems and the high blocks' first layer in the object's order: convc1 as a 1x1 layer object on the 1/8 map, then vfi_amt_upsample_lrelu."""

    def __init__(self, lib):
        super().__init__(lib)
        self.calls.update(stem=0, convc1_upsample=0)

    def stem(self, x, w, b, slopes):
        self.calls["stem"] += 1
        return run_stem(self.lib, x, w, b, slopes if slopes is not None else torch.ones(w.shape[0]))

    def convc1_upsample(self, corr, w, b, s, slope):
        self.calls["convc1_upsample"] += 1
        _, cin, h, wd = corr.shape
        cout = w.shape[0]
        hnd = self.lib.vfi_conv_create_ex(0, w.contiguous().data_ptr(), b.contiguous().data_ptr(), cout, cin, 1, 1, 0, None, cin, None)
        assert hnd, "vfi_conv_create_ex failed"
        try:
            xd = self._nhwc(corr)
            lo = torch.full((h * wd, cout), NAN, device="cuda")
            out = torch.full((h * s * wd * s, cout), NAN, device="cuda")
            _check(self.lib.vfi_conv_forward_ex(hnd, ptr(xd), cin, h, wd, ptr(lo), cout, 1, 0, 0.0, 0.0, 0.0, None, 0, None), "vfi_conv_forward_ex")
            _check(self.lib.vfi_amt_upsample_lrelu(ptr(lo), cout, ptr(out), cout, 1, h, wd, cout, s, C.c_float(slope), None), "vfi_amt_upsample_lrelu")
            torch.cuda.synchronize()
        finally:
            self.lib.vfi_conv_destroy(hnd)
        return out.reshape(h * s, wd * s, cout).permute(2, 0, 1)[None].cpu()


_RESTATED = {}


def restated64(shape_name):
    """the float64 restatement (the reference's order) of a forward golden case at NET_TS, once on the device and shared: [2,3,h,w] on the host"""
    if shape_name not in _RESTATED:
        f0, f1 = frames_of(shape_name)
        sd = {k: v.cuda() for k, v in amt_g_restated.state_dict64().items()}
        with torch.no_grad():
            _RESTATED[shape_name] = amt_g_restated.amt_g_forward(sd, f0.double().cuda(), f1.double().cuda(), NET_TS).cpu()
    return _RESTATED[shape_name]


@pytest.mark.parametrize("shape_name", ["128x128", "144x208", "130x200"])
def test_forward_with_the_kernels_in_place(lib, shape_name, golden_dir, oracle_threads):
    from cfi_amd import amt_spec

    golden = np.load(os.path.join(golden_dir, "amt_g_net.npz"))
    f0, f1 = frames_of(shape_name)
    sd = amt_spec.seeded_state_dict("G", SEED)
    ops = GKernelOps(lib)
    with torch.no_grad():
        got = amt_g_restated.amt_g_forward(sd, f0, f1, NET_TS, ops=ops)
    want = restated64(shape_name)
    n = len(NET_TS)
    # per timestep: three two-direction lookups (the high blocks make none), convf1 of five update blocks + comb_block's two layers;
    # per pair: the feature encoder's stem (both frames as one batch) and the pyramid stem of each frame
    assert ops.calls == {"lookup": 6 * n, "conv7x7": 7 * n, "combine_warps": n, "combine_out": n, "stem": 3, "convc1_upsample": 2 * n}
    assert torch.isfinite(got).all()
    for i, t in enumerate(NET_TS):
        d, sums_ok = cain_restated.compare(got[i].permute(1, 2, 0), golden, f"G_{shape_name}_t{t}_", NET_STRIDE, TOL)
        dr = float((got[i].double() - want[i]).abs().max())
        print(f"AMT-G {shape_name} t={t}: sampled max |d| vs the reference {d:.3e}, max |d| vs the float64 restatement {dr:.3e}")
        assert d <= TOL and sums_ok and dr <= TOL, describe_diff(got[i].double(), want[i], f"AMT-G {shape_name} t={t}", chan_last=False)


# ---- the network object and the node ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def engine(lib):
    """AmtEngine on the seeded AMT-G weights (amt_g patched on while the state dict is checked), closed after the file's tests"""
    from cfi_amd import amt, amt_spec, ckpt

    real = ckpt.load_config
    ckpt.load_config = config_with(True)
    try:
        eng = amt.AmtEngine(amt_spec.seeded_state_dict("G", SEED))
    finally:
        ckpt.load_config = real
    assert eng.variant == "G"
    yield eng
    eng.close()
    _RESTATED.clear()


@pytest.mark.parametrize("shape_name", ["128x128", "144x208", "130x200"])
def test_object_forward_matches_the_reference_and_the_restatement(lib, engine, shape_name, golden_dir):
    golden = np.load(os.path.join(golden_dir, "amt_g_net.npz"))
    f0, f1 = frames_of(shape_name)
    got = engine.forward(hwc(f0), hwc(f1), NET_TS).cpu()
    want = restated64(shape_name)
    assert torch.isfinite(got).all() and got.shape == (len(NET_TS),) + tuple(f0.shape[2:]) + (3,)
    for i, t in enumerate(NET_TS):
        d, sums_ok = cain_restated.compare(got[i], golden, f"G_{shape_name}_t{t}_", NET_STRIDE, TOL)
        dr = float((got[i].double() - want[i].permute(1, 2, 0)).abs().max())
        print(f"AMT-G object {shape_name} t={t}: sampled max |d| vs the reference {d:.3e}, max |d| vs the float64 restatement {dr:.3e}")
        assert d <= TOL and sums_ok and dr <= TOL, describe_diff(got[i].double(), want[i].permute(1, 2, 0), f"AMT-G {shape_name} t={t}")
    assert 0 < engine.workspace_bytes() < 1 << 30


def test_per_pair_reuse_is_exact_and_does_not_leak(lib, engine):
    a0, a1 = (hwc(f) for f in frames_of("130x200"))
    b0, b1 = a1.flip(0).contiguous(), a0.flip(1).contiguous()
    ts = [0.25, 0.5, 0.75]
    together = engine.forward(a0, a1, ts).clone()
    other = engine.forward(b0, b1, [0.5]).clone()
    single = torch.cat([engine.forward(a0, a1, [t]) for t in ts])
    assert torch.equal(together, single)
    assert float((together[1] - other[0]).abs().max()) > 1e-2, "the second pair must give another frame"
    assert torch.equal(engine.forward(b0, b1, [0.5]), other) and torch.equal(engine.forward(a0, a1, ts), together)
    assert float((together[0] - together[2]).abs().max()) > 1e-3, "the timestep must matter"


def test_size_guards_of_the_object(lib, engine):
    """below 128 padded pixels a side, and above AMT-G's own pixel limit: refused by the engine and by the C object before any launch"""
    from cfi_amd import _lib, amt

    before = engine.workspace_bytes()
    small = torch.zeros(100, 300, 3, device="cuda")
    with pytest.raises(ValueError, match="at least 128"):
        engine.forward(small, small, [0.5])
    rc = engine.lib.vfi_amt_forward(engine.handle, ptr(small), ptr(small), 3, 100, 300, (C.c_float * 1)(0.5), 1, ptr(small), None)
    assert rc != 0 and "at least 128" in _lib.last_error()
    H, W = 2160, 3840                                    # fits AMT-S / AMT-L, not AMT-G
    big = torch.zeros(H, W, 3, device="cuda")
    assert amt.MAX_PADDED_PIXELS_G < H * W <= amt.MAX_PADDED_PIXELS
    with pytest.raises(ValueError, match="for AMT-G"):
        engine.forward(big, big, [0.5])
    rc = engine.lib.vfi_amt_forward(engine.handle, ptr(big), ptr(big), 3, H, W, (C.c_float * 1)(0.5), 1, ptr(big), None)
    assert rc != 0 and "size limit" in _lib.last_error() and f"Hp * Wp * {amt.G_FLOATS_PER_PADDED_PIXEL * 4} bytes" in _lib.last_error()      # the same 88 floats on both sides
    assert engine.workspace_bytes() == before


@pytest.mark.parametrize("case", sorted(NODE_CASES))
def test_node_matches_the_reference_node(lib, engine, case, golden_dir, monkeypatch):
    golden = np.load(os.path.join(golden_dir, "amt_g_node.npz"))
    amt_g_restated.check_node_case(case, amt_g_restated.run_node(case, monkeypatch, engine), golden)


def test_node_refuses_g_with_the_key_off(lib, monkeypatch):
    import cfi_amd
    from cfi_amd import amt

    def no_engine(*a, **k):
        raise AssertionError("amt-g.pth must be refused before the checkpoint and the engine")

    monkeypatch.setattr(amt, "load_file_from_direct_url", no_engine)
    monkeypatch.setattr(amt, "cached_engine", no_engine)
    with pytest.raises(NotImplementedError, match="amt-g.pth: AMT-G has a forward of its own"):
        cfi_amd.AMT_VFI().vfi("amt-g.pth", torch.zeros(3, 128, 128, 3))
