"""-m gpu: the SepConv++ path on the MI355X — 3x3 stride-2 layers on odd inputs, the fused output stage (vfi_sepconv_pair_out) against
its float64 restatement with the gamma * 2^-24 * M bound of tests/ref_ops_restated.py, the whole forward against the reference's outputs
(tests/golden/sepconv_net.npz: sampled pixels and every row / column sum) and, for every pixel, the torch restatement
(tests/sepconv_restated.py, pinned to the same goldens by tests/test_sepconv_spec_cpu.py) at the golden sizes and 1080p, and the node
against the reference node (tests/golden/sepconv_node.npz).  Tolerance of the forward: per-pixel |d| <= 1e-3."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cain_restated
import ref_ops_restated as ror
import sepconv_restated
from gpu_util import describe_diff

pytestmark = pytest.mark.gpu
TOL = 1e-3
K = 51


def _check(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


@pytest.fixture(scope="module")
def lib(hip_lib):
    from cfi_amd import _lib

    _lib.check(hip_lib.vfi_init(0), "vfi_init")
    return hip_lib


@pytest.fixture(scope="module")
def sd():
    from cfi_amd.sepconv_spec import seeded_state_dict

    return seeded_state_dict(1)


@pytest.fixture(scope="module")
def engine(lib, sd):
    from cfi_amd.sepconv import SepconvEngine

    e = SepconvEngine(sd)
    yield e
    e.close()


# ---- 3x3 stride-2 layers on odd inputs ---------------------------------------------------------------------------------------------

def _s2_layer(lib, cin, cout, seed, odd=True):
    g = torch.Generator().manual_seed(seed)
    wt = ((torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) / (cin * 9) ** 0.5).contiguous()
    b = (torch.rand(cout, generator=g) - 0.5).contiguous()
    hnd = lib.vfi_conv_create_ex(0, wt.data_ptr(), b.data_ptr(), cout, cin, 3, 2, 0, None, cin, None)
    assert hnd, "create failed"
    if odd:
        _check(lib.vfi_conv_accept_odd(hnd, 1), "vfi_conv_accept_odd")
    return hnd, wt, b


def _s2_run(lib, hnd, x, cout):
    """x [n, h, w, cin] host -> [n, ceil(h/2), ceil(w/2), cout]; input and output live inside NaN surroundings (channel windows and a
    guard region after the last image), so a read past Hin / Win or a write outside the output fails"""
    n, h, w, cin = x.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    xin = torch.full((n * h * w + 64, cin + 8), float("nan"))
    xin[:n * h * w, 4:4 + cin] = x.reshape(-1, cin)
    xd = xin.cuda()
    out = torch.full((n * ho * wo + 64, cout + 8), float("nan"), device="cuda")
    _check(lib.vfi_conv_forward_ex(hnd, xd.data_ptr() + 16, cin + 8, h, w, out.data_ptr() + 16, cout + 8, n, 0, 0.0, 0.0, 0.0, None, 0, None),
           "conv_forward_ex")
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.isnan(got[n * ho * wo:]).all() and torch.isnan(got[:, :4]).all() and torch.isnan(got[:, 4 + cout:]).all(), "stray write"
    return got[:n * ho * wo, 4:4 + cout].reshape(n, ho, wo, cout)


@pytest.mark.parametrize("h,w", [(135, 240), (45, 80), (3, 5), (1, 1)])
@pytest.mark.parametrize("cin,cout", [(256, 512), (64, 96), (16, 32)])
def test_stride2_odd_inputs_vs_torch(lib, h, w, cin, cout):
    """nn.Conv2d(k=3, s=2, p=1) on odd sizes: ceil(H/2) x ceil(W/2), zero padding; the 64-, 96- and 32-wide output tiles"""
    hnd, wt, b = _s2_layer(lib, cin, cout, h * w + cin)
    try:
        g = torch.Generator().manual_seed(h + w)
        x = torch.rand(2, cin, h, w, generator=g) * 2 - 1
        got = _s2_run(lib, hnd, x.permute(0, 2, 3, 1).contiguous(), cout)
    finally:
        lib.vfi_conv_destroy(hnd)
    want = F.conv2d(x.double(), wt.double(), b.double(), stride=2, padding=1).permute(0, 2, 3, 1)
    assert got.shape == want.shape
    assert (got.double() - want).abs().max().item() <= 2e-5, describe_diff(got.double(), want, f"{h}x{w}")


@pytest.mark.parametrize("h,w,cin,cout", [(136, 240, 256, 512), (46, 80, 64, 96), (4, 6, 16, 32), (1080, 1920, 32, 64)])
def test_stride2_even_inputs_same_bits_with_and_without_odd_sizes(lib, h, w, cin, cout):
    """opting a layer in to odd sizes changes nothing at even sizes: same output size, same kernel, same bits"""
    outs = []
    for odd in (False, True):
        hnd, wt, b = _s2_layer(lib, cin, cout, h * w + cin, odd=odd)
        try:
            g = torch.Generator().manual_seed(h + w)
            x = torch.rand(1, h, w, cin, generator=g) * 2 - 1
            outs.append(_s2_run(lib, hnd, x, cout))
        finally:
            lib.vfi_conv_destroy(hnd)
    assert torch.equal(outs[0], outs[1])
    want = F.conv2d(x.permute(0, 3, 1, 2).double(), wt.double(), b.double(), stride=2, padding=1).permute(0, 2, 3, 1)
    assert (outs[0].double() - want).abs().max().item() <= 2e-5


def test_odd_sizes_are_opt_in_and_3x3_only(lib):
    """a 3x3 stride-2 layer rejects odd sizes unless vfi_conv_accept_odd was called; 2x2 stride-2 and stride-1 layers cannot opt in"""
    hnd, _, _ = _s2_layer(lib, 16, 32, 1, odd=False)
    x = torch.zeros(1, 5, 6, 16, device="cuda")
    out = torch.zeros(1, 3, 3, 32, device="cuda")
    try:
        assert lib.vfi_conv_forward_ex(hnd, x.data_ptr(), 16, 5, 6, out.data_ptr(), 32, 1, 0, 0.0, 0.0, 0.0, None, 0, None) != 0
        _check(lib.vfi_conv_accept_odd(hnd, 1), "vfi_conv_accept_odd")
        _check(lib.vfi_conv_forward_ex(hnd, x.data_ptr(), 16, 5, 6, out.data_ptr(), 32, 1, 0, 0.0, 0.0, 0.0, None, 0, None), "odd")
    finally:
        lib.vfi_conv_destroy(hnd)
    for k, stride in ((2, 2), (3, 1)):
        w = torch.rand(32, 16, k, k)
        hnd = lib.vfi_conv_create_ex(0, w.data_ptr(), None, 32, 16, k, stride, 0, None, 16, None)
        assert hnd
        try:
            assert lib.vfi_conv_accept_odd(hnd, 1) != 0
        finally:
            lib.vfi_conv_destroy(hnd)


# ---- the fused output stage -------------------------------------------------------------------------------------------------------

def _pair_out(lib, frames0, frames1, heads, offs, H, W):
    """frames [N,H,W,C] device (each frame inside NaN guards), heads [N,Hp,Wp,cs] device, offs = channel offsets of (V1, V2, H1, H2)"""
    N, _, _, Cc = frames0.shape
    Hp, Wp, cs = heads.shape[1:]
    out = torch.full((N * H * W * 3 + 256,), float("nan"), device="cuda")
    p0 = (C.c_void_p * N)(*[frames0[n].data_ptr() for n in range(N)])
    p1 = (C.c_void_p * N)(*[frames1[n].data_ptr() for n in range(N)])
    hp = [heads.data_ptr() + 4 * o for o in offs]
    _check(lib.vfi_sepconv_pair_out(p0, p1, N, Cc, H, W, hp[0], hp[1], hp[2], hp[3], cs, Hp, Wp, out.data_ptr(), None), "sepconv_pair_out")
    torch.cuda.synchronize()
    assert torch.isnan(out[N * H * W * 3:]).all(), "wrote past the output"
    return out[:N * H * W * 3].view(N, H, W, 3)


def _guarded(x):
    """x [N,H,W,C] -> a device copy whose items sit between NaN guards of one item each (so stray reads turn into NaN)"""
    N = x.shape[0]
    buf = torch.full((2 * N + 1,) + tuple(x.shape[1:]), float("nan"), device="cuda")
    buf[1::2] = x.cuda()
    return buf[1::2]


def _want(f0, f1, heads, offs, H, W, pad="replicate"):
    f = lambda t: t.permute(0, 3, 1, 2).double().cuda()
    hd = heads.permute(0, 3, 1, 2).double().cuda()
    v1, v2, h1, h2 = [hd[:, o:o + K] for o in offs]
    Hp, Wp = heads.shape[1:3]
    # the reference pads the frames to the heads' size by replication first; both pads together are a clamp to the frame
    e0 = F.pad(f(f0)[:, :3], [0, Wp - W, 0, Hp - H], mode="replicate")
    e1 = F.pad(f(f1)[:, :3], [0, Wp - W, 0, Hp - H], mode="replicate")
    out, M = sepconv_restated.pair_out(e0, e1, v1, v2, h1, h2, H, W, pad=pad)
    return out.permute(0, 2, 3, 1), M.permute(0, 2, 3, 1)


def _heads(N, Hp, Wp, cs, offs, seed, H, W):
    """filters with sum ~1 and a spread of signs; every channel outside the four 51-channel windows and every pixel outside H x W is NaN"""
    g = torch.Generator().manual_seed(seed)
    hd = torch.full((N, Hp, Wp, cs), float("nan"))
    for o in offs:
        hd[..., o:o + K] = (torch.rand(N, Hp, Wp, K, generator=g) - 0.3) * (2.0 / K)
    hd[:, H:], hd[:, :, W:] = float("nan"), float("nan")
    return hd


@pytest.mark.parametrize("N,H,W,Cc,Hp,Wp,cs,offs", [
    (2, 67, 131, 3, 68, 132, 4 * 52, (0, 52, 104, 156)),      # odd H / W, the network's layout
    (1, 20, 30, 4, 20, 30, 256, (3, 70, 129, 200)),            # a frame smaller than the filter, C = 4, unaligned channel offsets
    (1, 9, 140, 3, 10, 140, 60, (1, 1, 5, 7)),                 # overlapping head windows, 9 rows (a partial tile of pixel pairs)
    (3, 73, 65, 3, 74, 66, 208, (156, 104, 52, 0)),            # heads in reverse order, odd sizes at both tile edges
])
def test_pair_out_vs_float64(lib, N, H, W, Cc, Hp, Wp, cs, offs):
    g = torch.Generator().manual_seed(H * W + Cc)
    f0, f1 = torch.rand(N, H, W, Cc, generator=g), torch.rand(N, H, W, Cc, generator=g)
    heads = _heads(N, Hp, Wp, cs, offs, H + W, H, W)
    got = _pair_out(lib, _guarded(f0), _guarded(f1), heads.cuda(), offs, H, W).double()
    want, M = _want(f0, f1, heads, offs, H, W)
    assert torch.isfinite(got).all(), "NaN in the output: a stray read or an unwritten pixel"
    tol = ror.tolerance(M, sepconv_restated.gamma_pair_out()) + 2 * ror.U * want.abs()
    bad = (got - want).abs() > tol
    assert not bad.any(), describe_diff(got, want, f"{H}x{W}") + f", {int(bad.sum())} over the float64 bound"


def test_pair_out_borders_follow_the_clamp(lib):
    """a frame that is constant except for its last row / column: the clamp at the 25-pixel border reads those values again and
    again, zero padding (or a pad from the even-padded size) would not"""
    H, W, offs = 40, 57, (0, 52, 104, 156)
    f0 = torch.full((1, H, W, 3), 0.25)
    f0[:, -1], f0[:, :, -1] = 1.0, 1.0
    f1 = f0.clone()
    heads = _heads(1, H, W + 1, 208, offs, 3, H, W)       # the even-padded size: one more column
    got = _pair_out(lib, _guarded(f0), _guarded(f1), heads.cuda(), offs, H, W).double()
    want, M = _want(f0, f1, heads, offs, H, W)
    tol = ror.tolerance(M, sepconv_restated.gamma_pair_out()) + 2 * ror.U * want.abs()
    assert ((got - want).abs() <= tol).all(), describe_diff(got, want, "clamp")
    zero, _ = _want(f0, f1, heads, offs, H, W, pad="constant")
    assert (got - zero)[0, -3:, -3:].abs().min() > 0.01, "zero padding at the 25-pixel border would pass this test too"


def test_pair_out_small_normaliser_is_set_to_one(lib):
    """where both frames' horizontal filters sum to exactly 0 the normaliser is 0 and the output is the un-normalised sum (the
    reference's |n| < 0.01 -> 1); elsewhere the usual division"""
    H, W, offs = 24, 80, (0, 52, 104, 156)
    g = torch.Generator().manual_seed(4)
    f0, f1 = torch.rand(1, H, W, 3, generator=g), torch.rand(1, H, W, 3, generator=g)
    heads = _heads(1, H, W, 208, offs, 8, H, W)
    alt = torch.tensor([0.02 if i % 2 == 0 else -0.02 for i in range(K - 1)] + [0.0])     # sums to 0 exactly in any order of pairs
    for o in offs[2:]:
        heads[0, 5:12, 10:40, o:o + K] = alt
    got = _pair_out(lib, _guarded(f0), _guarded(f1), heads.cuda(), offs, H, W).double()
    want, M = _want(f0, f1, heads, offs, H, W)
    assert torch.isfinite(got).all(), "0 / 0: the |n| < 0.01 rule did not apply"
    tol = ror.tolerance(M, sepconv_restated.gamma_pair_out()) + 2 * ror.U * want.abs()
    assert ((got - want).abs() <= tol).all(), describe_diff(got, want, "threshold")
    region = got[0, 5:12, 10:40]
    assert region.abs().max() > 1e-4, "the region's output should be the raw sums, not 0"


# ---- the whole forward ------------------------------------------------------------------------------------------------------------

NET_SIZES = ((64, 96, 1), (90, 160, 2), (101, 179, 2), (24, 40, 1))     # as tools/make_golden_sepconv.py


def test_forward_vs_reference_golden(engine, sd, golden_dir, oracle_threads):
    gd = np.load(os.path.join(golden_dir, "sepconv_net.npz"))
    for i, (h, w, stride) in enumerate(NET_SIZES):
        f = cain_restated.seeded_frames(2, h, w, 3, 200 + i)
        fd = f.cuda()
        keep = fd.clone()
        got = engine.forward([fd[0]], [fd[1]])[0].cpu()
        assert torch.equal(fd, keep), "forward wrote its input frames"
        assert torch.isfinite(got).all()
        d, sums_ok = cain_restated.compare(got, gd, f"{h}x{w}_", stride, TOL)
        assert d <= TOL and sums_ok, f"{h}x{w}: sampled max |d| {d}, row / column sums within tolerance: {sums_ok}"
        x = f.permute(0, 3, 1, 2).contiguous()
        want = sepconv_restated.sepconv_forward(sd, x[0:1], x[1:2])[0].permute(1, 2, 0)
        assert (got - want).abs().max().item() <= TOL, describe_diff(got, want, f"{h}x{w}")


def _frames_1080p(seed):
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand(2, 3, 137, 242, generator=g)
    return F.interpolate(lo, size=(1080, 1920), mode="bilinear", align_corners=False)


def test_forward_1080p_vs_restatement(engine, sd, oracle_threads):
    """every pixel at 1080p: the network restated on the host in fp32, its output stage in float64 on the device"""
    f = _frames_1080p(5)
    got = engine.forward([f[0].permute(1, 2, 0).contiguous().cuda()], [f[1].permute(1, 2, 0).contiguous().cuda()])[0]
    with torch.no_grad():
        one, two, heads = sepconv_restated.features(sd, f[0:1], f[1:2])
        want, _ = sepconv_restated.pair_out(one.cuda(), two.cuda(), *[h.cuda() for h in heads], 1080, 1920)
    want = want[0].permute(1, 2, 0).float()
    assert (got - want).abs().max().item() <= TOL, describe_diff(got.cpu(), want.cpu(), "1080p")


def test_head_forms_agree(lib, engine):
    """the A/B forms of the forward (test options): the output stage reading the heads NHWC instead of planar gives the same bits (same
    values, same order); the heads' first convs as four 64 -> 64 layers instead of one 64 -> 256 layer agree within the gate"""
    g = torch.Generator().manual_seed(11)
    f = torch.rand(2, 90, 160, 3, generator=g).cuda()
    ref = engine.forward([f[0]], [f[1]]).clone()
    try:
        assert lib.vfi_test_set_option(b"sepconv_planar", 0) == 0
        assert torch.equal(engine.forward([f[0]], [f[1]]), ref)
        assert lib.vfi_test_set_option(b"sepconv_planar", 1) == 0
        assert lib.vfi_test_set_option(b"sepconv_split_heads", 1) == 0
        assert (engine.forward([f[0]], [f[1]]) - ref).abs().max().item() <= TOL
    finally:
        lib.vfi_test_set_option(b"sepconv_planar", 1)
        lib.vfi_test_set_option(b"sepconv_split_heads", 0)


def test_batched_pair_is_bit_identical_to_alone_1080p(engine):
    f = _frames_1080p(7).permute(0, 2, 3, 1).contiguous().cuda()
    g = f.flip(1).contiguous()
    alone = engine.forward([f[1]], [g[0]]).clone()
    batch = engine.forward([f[0], f[1]], [g[1], g[0]])
    assert torch.equal(batch[1], alone[0])
    assert torch.equal(engine.forward([f[1]], [g[0]]), alone)
    assert engine.workspace_bytes() > 0


# ---- the node ---------------------------------------------------------------------------------------------------------------------

def _node(monkeypatch, tmp_path, sd):
    from cfi_amd import ckpt, sepconv

    path = tmp_path / "ckpts" / "sepconv" / "sepconv.pth"
    path.parent.mkdir(parents=True)
    torch.save(sd, path)      # the real file format (a plain state dict), seeded weights
    monkeypatch.setattr(sepconv, "load_file_from_github_release", lambda model_type, name: str(path))
    ckpt.clear_engine_cache()
    return sepconv.SepconvVFI()


def test_node_vs_reference_node_golden(monkeypatch, tmp_path, lib, sd, golden_dir, oracle_threads):
    from cfi_amd.schedule import InterpolationStateList, bisect_output_plan

    node = _node(monkeypatch, tmp_path, sd)
    gd = np.load(os.path.join(golden_dir, "sepconv_node.npz"))
    cases = {"m2": (3, 3, 2, None), "m3": (2, 3, 3, None), "m5": (2, 3, 5, None), "list": (3, 3, [3, 0], None),
             "skip": (3, 3, 3, [1]), "rgba": (2, 4, 2, None)}      # as tools/make_golden_sepconv.py
    for name, (n, c, m, skip) in cases.items():
        frames = cain_restated.seeded_frames(n, 48, 72, c, 9)
        keep = frames.clone()
        states = InterpolationStateList(skip, True) if skip else None
        out = node.vfi("sepconv.pth", frames, 10, m, optional_interpolation_states=states)[0]
        assert tuple(out.shape) == tuple(gd[name + "_shape"]), name
        d, sums_ok = cain_restated.compare(out, gd, name + "_", 3, TOL)
        assert d <= TOL and sums_ok, f"{name}: sampled max |d| {d}, row / column sums within tolerance: {sums_ok}"
        if name == "list":      # pair 0 at m = 3; pair 1 dropped with its first frame and the clip's last frame
            want = sepconv_restated.node_frames(sd, frames[:2], 3)[:-1]
        else:
            want = sepconv_restated.node_frames(sd, frames, m, skip)
        assert (out - want).abs().max().item() <= TOL, describe_diff(out, want, name)
        assert torch.equal(frames, keep), f"{name}: input modified"
        plan, _ = bisect_output_plan(n, m, states)
        src = [(i, idx) for i, (kind, idx) in enumerate(plan) if kind == "src"]
        assert src and all(torch.equal(out[i], frames[idx, ..., :3]) for i, idx in src), f"{name}: original frames not bit-equal"


def test_node_errors(monkeypatch, tmp_path, lib, sd):
    node = _node(monkeypatch, tmp_path, sd)
    with pytest.raises(AssertionError, match="VFI model Sepconv requires at least 2 frames to work with, only found 1"):
        node.vfi("sepconv.pth", torch.rand(1, 64, 64, 3), 10, 2)
    with pytest.raises(ValueError):
        node.vfi("sepconv.pth", torch.rand(2, 64, 64, 3), 10, 1)
    with pytest.raises(RuntimeError, match="every frame pair was dropped"):
        node.vfi("sepconv.pth", torch.rand(3, 64, 64, 3), 10, [0, 0])
