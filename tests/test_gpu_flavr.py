"""-m gpu: the FLAVR path on the MI355X.

New kernels (csrc/flavr_net.hip) against float64 torch restatements at edge shapes, inputs and outputs inside NaN surroundings, with
bounds in the style of tests/ref_ops_restated.py: |got - want| <= gamma * 2^-24 * M, M = sum |term| of the element and gamma the
longest chain of fp32 roundings on the way to it (any summation order of n terms makes at most n - 1 roundings per term):

  stem        441 products + bias: gamma = 443 (ReLU is 1-Lipschitz)
  1x1 / s2    Cin products: gamma = Cin + 2
  frame-out   64 * 49 products + bias + mean: gamma = 3139
  frame-in    the mean of n = 4 Hp Wp values: a thread sums ceil(n / 65536) of them, a tree of 8 levels, the slots in double, one
              division: gamma_mean = ceil(n / 65536) + 10 on M = mean |x|; out = x - mean adds one rounding of the difference
  gate        mean m[c]: a slot (at most 1024 of them, at least 64 pixels each) sums the 4 p values of its p pixels in fp32, at most
              4 p - 1 roundings whatever the order; the slots are summed in double, + 2 for the conversion and the division:
              err_m = (4 p + 2) U mean|x|; z = b + w . m by C fmas and a 6-level butterfly: err_z = (C + 8) U (|b| + |w| . |m|)
              + |w| . err_m; y = sigmoid(z), |sigmoid'| <= 1/4, expf / add / divide within 8 ulp together: err_y = err_z / 4 + 8 U y;
              out = relu(fma(x, y, res)) or lrelu(x y): tol = |x| err_y + 2 U (|x y| + |res|)

The whole forward against the reference's outputs (tests/golden/flavr_net.npz: sampled pixels and every row / column sum) and, for every
pixel, the torch restatement (tests/flavr_restated.py, pinned to the same goldens by tests/test_flavr_spec_cpu.py) at the golden sizes,
256x448 and 1080p; the node against the reference node (tests/golden/flavr_node.npz).  Tolerance of the forward: per-pixel |d| <= 1e-3."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cain_restated
import flavr_restated
import ref_ops_restated as ror
from gpu_util import describe_diff
from test_flavr_node_cpu import CKPT_OF, NODE_CASES, check_case
from test_flavr_spec_cpu import NET_CASES, window

pytestmark = pytest.mark.gpu
TOL = 1e-3
SEED = 1
NAN = float("nan")
U = ror.U


def _check(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


@pytest.fixture(scope="module")
def lib(hip_lib):
    from cfi_amd import _lib

    _lib.check(hip_lib.vfi_init(0), "vfi_init")
    return hip_lib


@pytest.fixture(scope="module")
def engines(lib):
    from cfi_amd.flavr import FlavrEngine
    from cfi_amd.flavr_spec import seeded_state_dict

    made = {}

    def get(n_outputs):
        if n_outputs not in made:
            sd = seeded_state_dict(SEED, n_outputs)
            made[n_outputs] = (FlavrEngine(sd), sd)
        return made[n_outputs]

    yield get
    for e, _ in made.values():
        e.close()


def _ws(nbytes):
    return torch.empty(nbytes // 4 + 16, dtype=torch.float32, device="cuda")


def _bounded(got, want, tol, name):
    assert torch.isfinite(got).all(), f"{name}: NaN in the output: a stray read or an unwritten element"
    bad = (got.double() - want).abs() > tol
    assert not bad.any(), describe_diff(got.double(), want, name) + f", {int(bad.sum())} over the float64 bound"


# ---- frame-in ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,Cc", [(50, 70, 3), (101, 179, 4), (1, 1, 3), (16, 32, 3), (33, 16, 5)])
def test_frame_in_vs_float64(lib, H, W, Cc):
    g = torch.Generator().manual_seed(H * W + Cc)
    fr = torch.rand(4, H, W, Cc, generator=g)
    fr[..., 3:] = NAN                                           # alpha and beyond are not read
    buf = torch.full((9, H, W, Cc), NAN, device="cuda")         # every frame between NaN guards
    buf[1::2] = fr.cuda()
    Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    out = torch.full((Hp * Wp * 16 + 64,), NAN, device="cuda")
    mean = torch.full((8,), NAN, device="cuda")
    ws = _ws(4096)
    ptrs = (C.c_void_p * 4)(*[buf[1 + 2 * t].data_ptr() for t in range(4)])
    _check(lib.vfi_flavr_frame_in(ptrs, Cc, H, W, out.data_ptr(), mean.data_ptr(), ws.data_ptr(), 4096, None), "frame_in")
    torch.cuda.synchronize()
    assert torch.isnan(out[Hp * Wp * 16:]).all() and torch.isnan(mean[4:]).all(), "stray write"
    l, r, t, b = flavr_restated.pad16(H, W)
    x = F.pad(fr[..., :3].permute(0, 3, 1, 2).double(), (l, r, t, b), mode="replicate")      # [4,3,Hp,Wp]
    assert x.shape[2:] == (Hp, Wp)
    m = x.mean((0, 2, 3))
    n = 4 * Hp * Wp
    err_m = (-(-n // 65536) + 10) * U * x.abs().mean((0, 2, 3))
    got_m = mean[:4].cpu().double()
    assert got_m[3] == 0 and ((got_m[:3] - m).abs() <= err_m).all(), (got_m, m, err_m)
    want = (x - m[None, :, None, None]).permute(2, 3, 0, 1)                                  # [Hp,Wp,4,3]
    got = out[:Hp * Wp * 16].view(Hp, Wp, 4, 4).cpu()
    assert (got[..., 3] == 0).all()
    _bounded(got[..., :3], want, err_m[None, None, None, :] * (1 + U) + U * want.abs(), f"frame_in {H}x{W}")


# ---- stem --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Hp,Wp,bias", [(2, 2, True), (1, 1, False), (37, 53, True), (16, 48, False), (33, 35, True)])
def test_stem_vs_float64(lib, Hp, Wp, bias):
    g = torch.Generator().manual_seed(Hp * Wp)
    x = torch.rand(Hp, Wp, 4, 4, generator=g) * 2 - 1
    x[..., 3] = NAN                                             # the fourth component is padding: never used
    w = (torch.rand(64, 3, 3, 7, 7, generator=g) * 2 - 1) / 441 ** 0.5
    b = torch.rand(64, generator=g) - 0.5
    Ho, Wo, cs = (Hp + 1) // 2, (Wp + 1) // 2, 4 * 64 + 8
    xd = torch.full((Hp * Wp * 16 + 64,), NAN, device="cuda")
    xd[32:32 + Hp * Wp * 16] = x.reshape(-1).cuda()
    out = torch.full((Ho * Wo + 3, cs), NAN, device="cuda")
    ws = _ws(112896)
    wd, bd = w.cuda(), b.cuda()                                 # held until the kernels have run
    _check(lib.vfi_flavr_stem(xd.data_ptr() + 128, Hp, Wp, wd.data_ptr(), bd.data_ptr() if bias else None, out.data_ptr() + 16, cs,
                              ws.data_ptr(), 112896, None), "stem")
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.isnan(got[Ho * Wo:]).all() and torch.isnan(got[:, :4]).all() and torch.isnan(got[:, 4 + 256:]).all(), "stray write"
    x5 = x[..., :3].permute(3, 2, 0, 1)[None].double()          # [1,3,4,Hp,Wp]
    bb = b.double() if bias else None
    want = F.relu(F.conv3d(x5, w.double(), bb, stride=(1, 2, 2), padding=(1, 3, 3)))
    M = F.conv3d(x5.abs(), w.double().abs(), bb.abs() if bias else None, stride=(1, 2, 2), padding=(1, 3, 3))
    assert want.shape[2:] == (4, Ho, Wo)
    got = got[:Ho * Wo, 4:4 + 256].reshape(Ho, Wo, 4, 64)
    _bounded(got, want[0].permute(2, 3, 1, 0), ror.tolerance(M[0].permute(2, 3, 1, 0), 443), f"stem {Hp}x{Wp}")


# ---- 1x1 convolution with stride (1, s, s) -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("Hin,Win,stride", [(1, 1, 2), (5, 7, 2), (34, 22, 2), (9, 6, 1), (2, 2, 2)])
@pytest.mark.parametrize("cin,cout", [(64, 128), (16, 40)])
def test_down1x1_vs_float64(lib, Hin, Win, stride, cin, cout):
    g = torch.Generator().manual_seed(Hin * Win + cin)
    x = torch.rand(Hin, Win, 4, cin, generator=g) * 2 - 1
    w = ((torch.rand(cout, cin, generator=g) * 2 - 1) / cin ** 0.5).contiguous()
    hnd = lib.vfi_conv_create_ex(0, w.data_ptr(), None, cout, cin, 1, 1, 0, None, cin, None)
    assert hnd, "create failed"
    bordered = torch.full((Hin, Win, 6, cin), NAN)              # the network's layout: border slices are not read by this layer
    bordered[:, :, 1:5] = x
    xd = bordered.cuda()
    h, wo = (Hin + stride - 1) // stride, (Win + stride - 1) // stride
    sub = torch.full((h * wo * 4 * cin + 64,), NAN, device="cuda")
    out = torch.full((h * wo * 4 * cout + 64,), NAN, device="cuda")
    try:
        _check(lib.vfi_flavr_down1x1(hnd, cin, cout, xd.data_ptr() + 4 * cin, 6 * cin, cin, Hin, Win, stride, sub.data_ptr(), out.data_ptr(), None), "down1x1")
        torch.cuda.synchronize()
    finally:
        lib.vfi_conv_destroy(hnd)
    assert torch.isnan(out[h * wo * 4 * cout:]).all() and torch.isnan(sub[h * wo * 4 * cin:]).all(), "stray write"
    xs = x[::stride, ::stride].double()
    want = torch.einsum("hwtc,oc->hwto", xs, w.double())
    M = torch.einsum("hwtc,oc->hwto", xs.abs(), w.double().abs())
    _bounded(out[:h * wo * 4 * cout].view(h, wo, 4, cout).cpu(), want, ror.tolerance(M, cin + 2), f"down1x1 {Hin}x{Win}/{stride}")


# ---- SEGating ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,Cc", [(1, 64), (77, 512), (5000, 64), (333, 12), (70000, 128)])
@pytest.mark.parametrize("mode", [0, 1])
def test_gate_vs_float64(lib, P, Cc, mode):
    g = torch.Generator().manual_seed(P + Cc + mode)
    x = torch.rand(P, 4, Cc, generator=g) * 2 - 0.7
    res = torch.rand(P, 4, Cc, generator=g) * 2 - 1
    w = (torch.rand(Cc, Cc, generator=g) * 2 - 1) * (3.0 / Cc ** 0.5)
    b = torch.rand(Cc, generator=g) * 2 - 1
    xb = torch.full((P, 6, Cc), NAN)                            # bordered input; the border slices are not read
    xb[:, 1:5] = x
    xd = xb.cuda()
    rd = torch.full((P, 4, Cc + 4), NAN)
    rd[..., :Cc] = res
    rd = rd.cuda()
    ws_bytes = (1024 * Cc + Cc) * 4
    ws = _ws(ws_bytes)
    if mode == 0:       # in place, as a BasicBlock does it
        out, o_ps, o_ss, o_off = xd, 6 * Cc, Cc, Cc
    else:               # into the first half of a bordered concat buffer
        out, o_ps, o_ss, o_off = torch.full((P, 6, 2 * Cc), NAN, device="cuda"), 12 * Cc, 2 * Cc, 2 * Cc
    wd, bd = w.cuda(), b.cuda()                                 # held until the kernels have run
    _check(lib.vfi_flavr_gate(xd.data_ptr() + 4 * Cc, 6 * Cc, Cc, rd.data_ptr() if mode == 0 else None, 4 * (Cc + 4), Cc + 4,
                              out.data_ptr() + 4 * o_off, o_ps, o_ss, P, Cc, wd.data_ptr(), bd.data_ptr(), mode, ws.data_ptr(), ws_bytes, None), "gate")
    torch.cuda.synchronize()
    o = out.cpu()
    if mode == 0:
        assert torch.isnan(o[:, 0]).all() and torch.isnan(o[:, 5]).all(), "stray write"
        got = o[:, 1:5]
    else:
        assert torch.isnan(o[:, 0]).all() and torch.isnan(o[:, 5]).all() and torch.isnan(o[:, 1:5, Cc:]).all(), "stray write"
        got = o[:, 1:5, :Cc]
    xd64, w64, b64 = x.double(), w.double(), b.double()
    m = xd64.mean((0, 1))
    per_slot = -(-P // min(1024, max(1, -(-P // 64))))          # pixels of one of the (at most 1024) slots
    err_m = (4 * per_slot + 2) * U * xd64.abs().mean((0, 1))
    z = b64 + w64 @ m
    err_z = (Cc + 8) * U * (b64.abs() + w64.abs() @ m.abs()) + w64.abs() @ err_m
    y = torch.sigmoid(z)
    err_y = err_z / 4 + 8 * U * y
    if mode == 0:
        want = F.relu(xd64 * y + res.double())
        tol = xd64.abs() * err_y + 2 * U * ((xd64 * y).abs() + res.double().abs())
    else:
        want = F.leaky_relu(xd64 * y, 0.2)
        tol = xd64.abs() * err_y + 2 * U * (xd64 * y).abs()
    _bounded(got, want, tol, f"gate P={P} C={Cc} mode={mode}")
    assert float((y.max() - y.min())) > 0.2, "the gate values should differ between channels"


# ---- frame-out ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Hp,Wp,pt,pl,H,W,n_out", [(64, 80, 7, 5, 50, 70, 1), (16, 16, 7, 7, 1, 1, 3), (4, 5, 0, 0, 4, 5, 1), (48, 32, 0, 3, 48, 27, 3),
                                                   (35, 21, 1, 0, 33, 21, 1)])
def test_frame_out_vs_float64(lib, Hp, Wp, pt, pl, H, W, n_out):
    g = torch.Generator().manual_seed(Hp * Wp + H)
    feat = torch.rand(Hp, Wp, 64, generator=g) * 2 - 1
    w = torch.full((3 * n_out, 64, 7, 7), NAN)                  # outputs 1.. are never computed
    w[:3] = (torch.rand(3, 64, 7, 7, generator=g) * 2 - 1) / 56.0
    b = torch.full((3 * n_out,), NAN)
    b[:3] = torch.rand(3, generator=g) - 0.5
    mean = torch.tensor([0.4, 0.5, 0.6, NAN])
    fd = torch.full((Hp * Wp * 64 + 128,), NAN, device="cuda")
    fd[64:64 + Hp * Wp * 64] = feat.reshape(-1).cuda()
    out = torch.full((H * W * 3 + 64,), NAN, device="cuda")
    ws = _ws(50176)
    wd, bd, md = w.cuda(), b.cuda(), mean.cuda()                # held until the kernels have run
    _check(lib.vfi_flavr_frame_out(fd.data_ptr() + 256, Hp, Wp, wd.data_ptr(), bd.data_ptr(), md.data_ptr(), pt, pl, H, W,
                                   out.data_ptr(), ws.data_ptr(), 50176, None), "frame_out")
    torch.cuda.synchronize()
    assert torch.isnan(out[H * W * 3:]).all(), "stray write"
    f4 = F.pad(feat.permute(2, 0, 1)[None].double(), (3, 3, 3, 3), mode="reflect")
    w64, b64, m64 = w[:3].double(), b[:3].double(), mean[:3].double()
    want = F.conv2d(f4, w64, b64) + m64[None, :, None, None]
    M = F.conv2d(f4.abs(), w64.abs(), b64.abs()) + m64.abs()[None, :, None, None]
    crop = lambda t: t[0, :, pt:pt + H, pl:pl + W].permute(1, 2, 0)
    _bounded(out[:H * W * 3].view(H, W, 3).cpu(), crop(want), ror.tolerance(crop(M), 64 * 49 + 3), f"frame_out {Hp}x{Wp}")


# ---- the whole forward -------------------------------------------------------------------------------------------------------------

def _forward(engine, fr):
    """fr: four NCHW [1,3,H,W] host frames -> [H,W,3] host"""
    dev = [f[0].permute(1, 2, 0).contiguous().cuda() for f in fr]
    keep = [d.clone() for d in dev]
    got = engine.forward(dev)[0].cpu()
    assert all(torch.equal(a, b) for a, b in zip(dev, keep)), "forward wrote its input frames"
    assert torch.isfinite(got).all()
    return got


@pytest.mark.parametrize("name", sorted(NET_CASES))
def test_forward_vs_reference_golden(name, engines, golden_dir, oracle_threads):
    n_outputs, h, w, stride, fseed = NET_CASES[name]
    engine, sd = engines(n_outputs)
    gd = np.load(os.path.join(golden_dir, "flavr_net.npz"))
    fr = window(h, w, fseed)
    got = _forward(engine, fr)
    d, sums_ok = cain_restated.compare(got, gd, name + "_", stride, TOL)
    with torch.no_grad():
        want = flavr_restated.flavr_forward(sd, fr)[0].permute(1, 2, 0)
    print(name, "sampled max |d| vs golden", d, "max |d| vs restatement", (got - want).abs().max().item())
    assert d <= TOL and sums_ok, f"{name}: sampled max |d| {d}, row / column sums within tolerance: {sums_ok}"
    assert (got - want).abs().max().item() <= TOL, describe_diff(got, want, name)


def _smooth_window(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand(4, 3, h // 8 + 2, w // 8 + 2, generator=g)
    f = F.interpolate(lo, size=(h, w), mode="bilinear", align_corners=False)
    return [f[i:i + 1].contiguous() for i in range(4)]


@pytest.mark.parametrize("n_outputs", [1, 3])
def test_forward_256x448_vs_restatement(n_outputs, engines, oracle_threads):
    engine, sd = engines(n_outputs)
    fr = _smooth_window(256, 448, 20 + n_outputs)
    got = _forward(engine, fr)
    with torch.no_grad():
        want = flavr_restated.flavr_forward(sd, fr)[0].permute(1, 2, 0)
    print("256x448 n_outputs", n_outputs, "max |d|", (got - want).abs().max().item(), "std(want - mean)", (want - want.mean((0, 1))).std().item())
    assert (got - want).abs().max().item() <= TOL, describe_diff(got, want, f"256x448 o{n_outputs}")


def test_forward_1080p_vs_restatement(engines, oracle_threads):
    """every pixel at 1080x1920 (padded 1088x1920: the last up-convolution's tensor sits 0.4 % under the kernels' 2 GiB image limit)"""
    engine, sd = engines(1)
    fr = _smooth_window(1080, 1920, 5)
    got = _forward(engine, fr)
    print("1080p workspace bytes", engine.workspace_bytes())
    with torch.no_grad():
        want = flavr_restated.flavr_forward(sd, fr)[0].permute(1, 2, 0)
    print("1080p max |d|", (got - want).abs().max().item())
    assert (got - want).abs().max().item() <= TOL, describe_diff(got, want, "1080p")
    engine.release_workspace()


def test_window_in_a_batch_is_bit_identical_to_alone(engines):
    engine, _ = engines(1)
    for h, w in ((64, 96), (256, 448), (101, 179)):
        a = [f[0].permute(1, 2, 0).contiguous().cuda() for f in _smooth_window(h, w, 7)]
        b = [t.flip(0).contiguous() for t in a]
        alone = engine.forward(a).clone()
        batch = engine.forward(b + a)
        assert batch.shape == (2, h, w, 3) and torch.equal(batch[1], alone[0]), (h, w)
        assert torch.equal(engine.forward(a), alone), (h, w)
        assert not torch.equal(batch[0], alone[0])
    assert engine.workspace_bytes() > 0


def test_frames_over_the_size_limit_are_refused_before_any_launch(lib, engines):
    from cfi_amd import _lib

    engine, _ = engines(1)
    engine.forward([torch.rand(32, 32, 3, device="cuda")] * 4)
    before = engine.workspace_bytes()
    H, W = 1104, 1920                                       # 2 119 680 padded pixels: the [Hp, Wp, 256] tensor would pass 2 GiB
    f = torch.rand(H, W, 3, device="cuda")
    out = torch.full((1, H, W, 3), NAN, device="cuda")
    p = (C.c_void_p * 4)(*[f.data_ptr()] * 4)
    rc = lib.vfi_flavr_forward(engine.handle, p, 1, 3, H, W, out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc != 0 and "size limit" in _lib.last_error(), _lib.last_error()
    assert torch.isnan(out).all(), "something was written"
    assert engine.workspace_bytes() == before, "the workspace was touched"
    with pytest.raises(RuntimeError, match="size limit"):
        engine.forward([f] * 4)
    assert torch.isfinite(engine.forward([torch.rand(32, 32, 3, device="cuda")] * 4)).all()      # the engine is still usable


# ---- the node ----------------------------------------------------------------------------------------------------------------------

def test_node_vs_reference_node_golden(monkeypatch, tmp_path, lib, golden_dir, oracle_threads):
    from cfi_amd import ckpt, flavr
    from cfi_amd.flavr_spec import seeded_state_dict
    from cfi_amd.schedule import InterpolationStateList

    paths = {}
    for n_outputs, name in CKPT_OF.items():      # the real files' format: {"state_dict": ...} under "module."
        paths[name] = str(tmp_path / name)
        torch.save({"state_dict": {"module." + k: v for k, v in seeded_state_dict(SEED, n_outputs).items()}}, paths[name])
    monkeypatch.setattr(flavr, "load_file_from_github_release", lambda model_type, name: paths[name])
    ckpt.clear_engine_cache()
    gd = np.load(os.path.join(golden_dir, "flavr_node.npz"))
    node = flavr.FLAVR_VFI()
    try:
        for case, (n, h, w, c, m, dup, skip, n_outputs) in NODE_CASES.items():
            frames = cain_restated.seeded_frames(n, h, w, c, 9)
            keep = frames.clone()
            states = InterpolationStateList(skip, True) if skip else None
            if m != 2:
                with pytest.warns(UserWarning, match="only supports 2x"):
                    out = node.vfi(CKPT_OF[n_outputs], frames, 10, m, dup, states)[0]
            else:
                out = node.vfi(CKPT_OF[n_outputs], frames, 10, m, dup, states)[0]
            check_case(case, out, gd)
            want = flavr_restated.node_frames(seeded_state_dict(SEED, n_outputs), frames, dup, skip)
            assert (out - want).abs().max().item() <= TOL, describe_diff(out, want, case)
            assert torch.equal(frames, keep), f"{case}: input modified"
            src = [(i, idx) for i, (kind, idx) in enumerate(flavr.window_plan(n, dup, states)) if kind == "src"]
            assert src and all(torch.equal(out[i], frames[idx, ..., :3]) for i, idx in src), f"{case}: original frames not bit-equal"
        with pytest.raises(AssertionError, match="VFI model ST-MFNet requires at least 4 frames to work with, only found 3"):
            node.vfi("FLAVR_2x.pth", torch.rand(3, 32, 32, 3))
    finally:
        ckpt.clear_engine_cache()
