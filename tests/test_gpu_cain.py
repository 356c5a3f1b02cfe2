"""-m gpu: the CAIN path on the MI355X — reflect-padded 3x3 layers on both conv kernels, channel attention, the frame-in / frame-out
kernels, the whole forward against the reference's outputs (tests/golden/cain_net.npz: sampled pixels and every row / column sum)
and, for every pixel, the torch restatement (tests/cain_restated.py, pinned to the same goldens by tests/test_cain_spec_cpu.py) at the
golden sizes and 1080p, and the node against the reference node (tests/golden/cain_node.npz) likewise.  Tolerance: per-pixel |d| <= 1e-3."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cain_restated
from gpu_util import describe_diff

pytestmark = pytest.mark.gpu
TOL = 1e-3


def _check(lib, rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


@pytest.fixture(scope="module")
def lib(hip_lib):
    from cfi_amd import _lib

    _lib.check(hip_lib.vfi_init(0), "vfi_init")
    return hip_lib


@pytest.fixture(scope="module")
def sd():
    return cain_restated.seeded_state_dict(1)


@pytest.fixture(scope="module")
def engine(lib, sd):
    from cfi_amd.cain import CainEngine

    e = CainEngine(sd)
    yield e
    e.close()


@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 17, 30, 192, 192), (1, 27, 41, 24, 40)])
def test_reflect_conv_on_both_kernels(lib, n, h, w, cin, cout):
    """pad_mode 2 = ReflectionPad2d(1) + Conv2d on the direct kernel (vfi_test_conv_algo 1) and the Winograd kernel (2) at one size,
    read from and written to channel windows, against F.conv2d(F.pad(x, reflect))."""
    g = torch.Generator().manual_seed(h * w + cin)
    x = torch.rand(n, cin, h, w, generator=g) * 2 - 1
    wt = ((torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) / (cin * 9) ** 0.5).contiguous()
    b = (torch.rand(cout, generator=g) - 0.5).contiguous()
    want = F.conv2d(F.pad(x.double(), (1, 1, 1, 1), mode="reflect"), wt.double(), b.double()).float().permute(0, 2, 3, 1)
    xin = torch.zeros(n, h, w, cin + 8)
    xin[..., 4:4 + cin] = x.permute(0, 2, 3, 1)
    xd = xin.cuda()
    hnd = lib.vfi_conv_create_ex(0, wt.data_ptr(), b.data_ptr(), cout, cin, 3, 1, 2, None, cin, None)
    assert hnd, "create failed"
    outs = {}
    try:
        for mode in (1, 2):
            assert lib.vfi_test_conv_algo(mode) == mode
            out = torch.full((n, h, w, cout + 8), float("nan"), device="cuda")
            _check(lib, lib.vfi_conv_forward_ex(hnd, xd.data_ptr() + 16, cin + 8, h, w, out.data_ptr() + 16, cout + 8, n, 0, 0.0, 0.0, 0.0,
                                                None, 0, None), "conv_forward_ex")
            torch.cuda.synchronize()
            got = out.cpu()
            assert torch.isnan(got[..., :4]).all() and torch.isnan(got[..., 4 + cout:]).all(), "wrote outside its channel window"
            outs[mode] = got[..., 4:4 + cout]
    finally:
        lib.vfi_test_conv_algo(0)
        lib.vfi_conv_destroy(hnd)
    for mode, got in outs.items():
        assert (got - want).abs().max().item() <= 2e-5, describe_diff(got, want, f"mode {mode}")
    assert not torch.equal(outs[1], outs[2]), "both A/B forms gave the same bits: the Winograd form did not run"


def test_reflect_needs_two_pixels(lib):
    wt = torch.zeros(8, 8, 3, 3)
    hnd = lib.vfi_conv_create_ex(0, wt.data_ptr(), None, 8, 8, 3, 1, 2, None, 8, None)
    assert hnd
    try:
        x = torch.zeros(1, 1, 5, 8, device="cuda")
        assert lib.vfi_conv_forward_ex(hnd, x.data_ptr(), 8, 1, 5, x.data_ptr(), 8, 1, 0, 0.0, 0.0, 0.0, None, 0, None) != 0
    finally:
        lib.vfi_conv_destroy(hnd)
    assert not lib.vfi_conv_create_ex(1, wt.data_ptr(), None, 8, 8, 4, 2, 2, None, 8, None), "reflect is for 3x3 convolutions only"


@pytest.mark.parametrize("n,hw", [(1, 34560), (3, 17 * 23)])
def test_channel_attention_vs_torch(lib, n, hw):
    g = torch.Generator().manual_seed(hw)
    t = torch.rand(n, hw, 192, generator=g) * 2 - 1
    x = torch.rand(n, hw, 192, generator=g) - 0.5
    w1 = (torch.rand(12, 192, generator=g) - 0.5) / 4
    b1 = torch.rand(12, generator=g) - 0.5
    w2 = torch.rand(192, 12, generator=g) - 0.5
    b2 = torch.rand(192, generator=g) - 0.5
    td, xd, ws = t.cuda(), x.cuda(), torch.empty(n * 257 * 192, device="cuda")
    pw = [p.cuda() for p in (w1, b1, w2, b2)]
    out = torch.empty_like(td)
    args = (n, hw, 192, pw[0].data_ptr(), pw[1].data_ptr(), pw[2].data_ptr(), pw[3].data_ptr(), 12, ws.data_ptr(), ws.numel() * 4, None)
    _check(lib, lib.vfi_channel_attention(td.data_ptr(), xd.data_ptr(), out.data_ptr(), *args), "channel_attention")
    again = xd.clone()       # in place on x, as the RCAB chain runs
    _check(lib, lib.vfi_channel_attention(td.data_ptr(), again.data_ptr(), again.data_ptr(), *args), "channel_attention")
    torch.cuda.synchronize()
    td64 = t.double()
    s = torch.sigmoid(F.relu(td64.mean(1) @ w1.double().T + b1.double()) @ w2.double().T + b2.double())
    want = (td64 * s[:, None, :] + x.double()).float()
    got = out.cpu()
    assert (got - want).abs().max().item() <= 2e-5, describe_diff(got, want, "channel attention")
    assert torch.equal(again.cpu(), got), "in-place form differs"


@pytest.mark.parametrize("H,W,C", [(100, 180, 3), (64, 96, 4), (1080, 1920, 3)])
def test_frame_in_and_out_vs_torch(lib, H, W, C):
    g = torch.Generator().manual_seed(H + C)
    f = torch.rand(2, H, W, C, generator=g)
    fd = f.cuda()
    keep = fd.clone()
    Hp, Wp = (H + 127) // 128 * 128, (W + 127) // 128 * 128
    h, w = Hp // 8, Wp // 8
    feat = torch.full((1, h, w, 384), float("nan"), device="cuda")
    means = torch.zeros(1, 2, 3, device="cuda")
    ws = torch.empty(1024, device="cuda")
    for k in range(2):
        _check(lib, lib.vfi_cain_frame_in(fd[k].data_ptr(), C, H, W, feat.data_ptr() + k * 192 * 4, 384, means.data_ptr() + k * 12,
                                          ws.data_ptr(), ws.numel() * 4, None), "cain_frame_in")
    torch.cuda.synchronize()
    assert torch.equal(fd, keep), "frame-in wrote its input"
    x = f[..., :3].permute(0, 3, 1, 2).double()
    m = x.mean((2, 3), keepdim=True)
    pw, ph = Wp - W, Hp - H
    xp = F.pad(x - m, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2), mode="reflect")
    want = cain_restated._unshuffle8(xp).float()
    want = torch.cat([want[0], want[1]], 0).permute(1, 2, 0)
    assert (means.cpu()[0] - m.view(2, 3).float()).abs().max().item() <= 1e-6
    assert (feat.cpu()[0] - want).abs().max().item() <= 1e-6, describe_diff(feat.cpu()[0], want, "frame-in")
    # frame-out: the x8 shuffle + crop + (m0 + m1) / 2 of a 192-channel map
    t = torch.rand(1, h, w, 192, generator=g)
    out = torch.full((1, H, W, 3), float("nan"), device="cuda")
    _check(lib, lib.vfi_cain_frame_out(t.cuda().data_ptr(), means.data_ptr(), out.data_ptr(), 1, H, W, None), "cain_frame_out")
    torch.cuda.synchronize()
    sh = cain_restated._shuffle8(t.permute(0, 3, 1, 2))[:, :, ph // 2:ph // 2 + H, pw // 2:pw // 2 + W]
    want = (sh + (means.cpu()[0, 0] + means.cpu()[0, 1]).view(1, 3, 1, 1) / 2).permute(0, 2, 3, 1)
    assert (out.cpu() - want).abs().max().item() <= 1e-6, describe_diff(out.cpu(), want, "frame-out")


def test_forward_vs_reference_golden(engine, sd, golden_dir, oracle_threads):
    gd = np.load(os.path.join(golden_dir, "cain_net.npz"))
    for i, (h, w, stride) in enumerate(((64, 96, 1), (100, 180, 2), (256, 448, 4))):
        f = cain_restated.seeded_frames(2, h, w, 3, 100 + i)
        fd = f.cuda()
        keep = fd.clone()
        got = engine.forward([fd[0]], [fd[1]])[0].cpu()
        assert torch.equal(fd, keep), "forward wrote its input frames"
        d, sums_ok = cain_restated.compare(got, gd, f"{h}x{w}_", stride, TOL)
        assert d <= TOL and sums_ok, f"{h}x{w}: sampled max |d| {d}, row / column sums within tolerance: {sums_ok}"
        x = f.permute(0, 3, 1, 2).contiguous()
        with torch.no_grad():
            want = cain_restated.cain_forward(sd, x[0:1], x[1:2])[0].permute(1, 2, 0)
        assert (got - want).abs().max().item() <= TOL, describe_diff(got, want, f"{h}x{w}")
        assert got.min() < 0 or got.max() > 1, "values outside [0, 1] expected (no clamp)"


def test_forward_1080p_vs_restatement(engine, sd, oracle_threads):
    g = torch.Generator().manual_seed(5)
    lo = torch.rand(2, 3, 137, 242, generator=g)
    f = F.interpolate(lo, size=(1080, 1920), mode="bilinear", align_corners=False)
    got = engine.forward([f[0].permute(1, 2, 0).contiguous().cuda()], [f[1].permute(1, 2, 0).contiguous().cuda()])[0].cpu()
    with torch.no_grad():
        want = cain_restated.cain_forward(sd, f[0:1], f[1:2])[0].permute(1, 2, 0)
    assert (got - want).abs().max().item() <= TOL, describe_diff(got, want, "1080p")


def test_batched_pair_is_bit_identical_to_alone(engine):
    """At 540x960 (feature map 80 x 128) every layer takes the Winograd kernel, chosen per image: a pair's bits do not depend on
    its batch mates, and two runs agree."""
    g = torch.Generator().manual_seed(9)
    f = torch.rand(4, 540, 960, 3, generator=g).cuda()
    alone = engine.forward([f[1]], [f[2]]).clone()
    batch = engine.forward([f[0], f[1], f[2]], [f[1], f[2], f[3]])
    assert torch.equal(batch[1], alone[0])
    assert torch.equal(engine.forward([f[1]], [f[2]]), alone)


def _node(monkeypatch, tmp_path, sd):
    from cfi_amd import cain, ckpt

    path = tmp_path / "ckpts" / "cain" / "pretrained_cain.pth"
    path.parent.mkdir(parents=True)
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}}, path)    # the real file format, seeded weights
    monkeypatch.setattr(cain, "load_file_from_github_release", lambda model_type, name: str(path))
    ckpt.clear_engine_cache()
    return cain.CAIN_VFI()


def test_node_vs_reference_node_golden(monkeypatch, tmp_path, lib, sd, golden_dir, oracle_threads):
    from cfi_amd.schedule import InterpolationStateList, bisect_output_plan

    node = _node(monkeypatch, tmp_path, sd)
    gd = np.load(os.path.join(golden_dir, "cain_node.npz"))
    cases = {"m2": (3, 3, 2, None), "m3": (2, 3, 3, None), "m5": (2, 3, 5, None), "m7": (2, 3, 7, None), "list": (3, 3, [3, 0], None),
             "skip": (3, 3, 3, [1]), "rgba": (2, 4, 2, None)}      # as tools/make_golden_cain.py
    for name, (n, c, m, skip) in cases.items():
        frames = cain_restated.seeded_frames(n, 48, 72, c, 7)
        keep = frames.clone()
        states = InterpolationStateList(skip, True) if skip else None
        out = node.vfi("pretrained_cain.pth", frames, 10, m, optional_interpolation_states=states)[0]
        assert tuple(out.shape) == tuple(gd[name + "_shape"]), name
        d, sums_ok = cain_restated.compare(out, gd, name + "_", 3, TOL)
        assert d <= TOL and sums_ok, f"{name}: sampled max |d| {d}, row / column sums within tolerance: {sums_ok}"
        if name == "list":      # pair 0 at m = 3; pair 1 dropped with its first frame and the clip's last frame
            want = cain_restated.node_frames(sd, frames[:2], 3)[:-1]
        else:
            want = cain_restated.node_frames(sd, frames, m, skip)
        assert (out - want).abs().max().item() <= TOL, describe_diff(out, want, name)
        assert torch.equal(frames, keep), f"{name}: input modified"
        plan, _ = bisect_output_plan(n, m, states)
        src = [(i, idx) for i, (kind, idx) in enumerate(plan) if kind == "src"]
        assert src and all(torch.equal(out[i], frames[idx, ..., :3]) for i, idx in src), f"{name}: original frames not bit-equal"
        assert out.min() < 0 or out.max() > 1, f"{name}: no value outside [0, 1] (clamped?)"


def test_node_errors(monkeypatch, tmp_path, lib, sd):
    node = _node(monkeypatch, tmp_path, sd)
    with pytest.raises(RuntimeError, match="too small for its reflection padding"):
        node.vfi("pretrained_cain.pth", torch.rand(2, 32, 32, 3), 10, 2)
    with pytest.raises(AssertionError, match="VFI model CAIN  requires at least 2 frames to work with, only found 1"):
        node.vfi("pretrained_cain.pth", torch.rand(1, 64, 64, 3), 10, 2)
