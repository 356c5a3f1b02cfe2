"""-m gpu: the live-K forms of the RIFE block-input convolutions against the forms they replace, bit for bit.

From block 1 on the block input X has 20 live channels, padded to 24 (a K chunk is 8 channels).  The padded channels meet zero
weights, so a third of the last chunk's MFMAs added fma(x, 0, acc).  Two kernels skip them:
  * trans1_conv0a_kernel<true> (csrc/rife_ops.hip): 90 instead of 108 MFMAs per sub-tile; the 108 form stays behind option fuse0a = 2;
  * conv_mfma2_kernel<..., TAIL4> (csrc/conv_mfma2.hip, variant 62 d2_m1n2_live4) for conv0a_b1 / conv0a_b2; the plain tile is variant 39.
Dropping fma(x, 0, acc) terms from an fmaf chain whose accumulator starts at +0 leaves every bit: the comparisons are torch.equal.
(The op-level entry takes NHWC input, which it pads to 24 channels itself; the planar-4 input of the network's layers is covered by
the whole-network comparison with the variants forced by trace name.)"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from cfi_amd import synth
from gpu_util import describe_diff, hptr, nhwc, ptr
from oracle import rife_oracle

pytestmark = pytest.mark.gpu

PLAIN, LIVE4 = 39, 62      # d2_m1n2 / d2_m1n2_live4 in the common variant numbering


@pytest.fixture(scope="module")
def sd():
    return synth.rife47_synth_state_dict(1234)


def _set(lib, name, value):
    assert lib.vfi_test_set_option(name, value) == 0, name


@pytest.mark.parametrize("h,w,bs", [(64, 64, 1),        # 8 tiles of the fused kernel, every one touches a border
                                    (70, 90, 2),        # padded to 128 x 128, cropped
                                    (270, 480, 3)])     # 960 tiles > 2 x 256 workgroups: the persistent loop runs twice, flow ping-pong
def test_live_k_network_matches_full_k(hip_lib, sd, h, w, bs):
    from cfi_amd.rife import RifeEngine, run_tasks

    torch.cuda.set_device(0)
    eng = RifeEngine(sd, "4.7")
    try:
        frames = synth.smooth_frames(bs + 1, h, w, seed=h + bs, shift=3.0)
        tasks = [(p, 0.5 if p % 2 == 0 else 0.3) for p in range(bs)]
        live = run_tasks(eng, frames, tasks, batch_size=bs)
        try:
            _set(hip_lib, b"fuse0a", 2)
            full0a = run_tasks(eng, frames, tasks, batch_size=bs)
        finally:
            _set(hip_lib, b"fuse0a", 1)
        try:
            assert hip_lib.vfi_test_variant_override(f"conv0a_b1={PLAIN},conv0a_b2={PLAIN}".encode()) == 0
            plain_direct = run_tasks(eng, frames, tasks, batch_size=bs)
        finally:
            hip_lib.vfi_test_variant_override(None)
        again = run_tasks(eng, frames, tasks, batch_size=bs)
    finally:
        eng.close()
    assert torch.equal(live, again), "not deterministic / state left behind by the reference forms"
    assert torch.equal(live, full0a), describe_diff(live, full0a, "trans1_conv0a: 90-MFMA form vs the kept 108-MFMA form")
    assert torch.equal(live, plain_direct), describe_diff(live, plain_direct, "conv0a_b1/b2: live-K tail vs plain tile")
    if h <= 70:
        x = frames.permute(0, 3, 1, 2)
        with torch.inference_mode():
            want = torch.cat([rife_oracle.ifnet47_forward(sd, x[p:p + 1], x[p + 1:p + 2], torch.tensor([t]).view(1, 1, 1, 1)) for p, t in tasks])
        want = want.permute(0, 2, 3, 1).clamp(0, 1)
        assert (live - want).abs().max().item() <= 1e-3, describe_diff(live, want, "live-K forms vs oracle")


def _last_launch(lib):
    rec = (C.c_int32 * 8)()
    assert lib.vfi_test_last_conv_launch(rec, 8) == 8
    return list(rec)


def _conv_s2(lib, x, wt, b, variant):
    n, cin, h, w = x.shape
    cout = wt.shape[0]
    xd = nhwc(x).cuda()
    out = torch.full((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, cout), float("nan"), device="cuda")
    rc = lib.vfi_conv3x3(ptr(xd), hptr(wt), hptr(b), None, ptr(out), n, h, w, cin, cout, 2, 1, 0.2, variant, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu(), _last_launch(lib)


@pytest.mark.parametrize("h,w", [(34, 36), (66, 130)])      # partial tiles on both axes; 2 and 5 tiles per row
@pytest.mark.parametrize("cout", [48, 64])
def test_live_k_tail_matches_plain_tile(hip_lib, cout, h, w):
    cin, n = 20, 2
    g = torch.Generator().manual_seed(cout * 1000 + h)
    x = torch.rand(n, cin, h, w, generator=g) * 2 - 1
    wt = (torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) / (cin * 9) ** 0.5
    b = torch.rand(cout, generator=g) - 0.5
    want = nhwc(F.leaky_relu(F.conv2d(x, wt, b, 2, 1), 0.2))
    tail, rec_t = _conv_s2(hip_lib, x, wt, b, LIVE4)
    plain, rec_p = _conv_s2(hip_lib, x, wt, b, PLAIN)
    auto, rec_a = _conv_s2(hip_lib, x, wt, b, -1)
    assert rec_t[:2] == [2, LIVE4] and rec_p[:2] == [2, PLAIN], (rec_t, rec_p)
    assert rec_a[:2] == [2, LIVE4], f"a 20 -> {cout} stride-2 layer must take the live-K tail by itself: {rec_a}"
    assert not torch.isnan(tail).any() and not torch.isnan(plain).any(), "unwritten outputs"
    assert torch.equal(tail, plain), describe_diff(tail, plain, f"tail vs plain, 20 -> {cout} at {h}x{w}")
    assert torch.equal(auto, tail)
    tol = 2e-5 * max(1.0, want.abs().max().item())      # tests/test_gpu_ops.py: fp32 summation order only
    assert (tail - want).abs().max().item() <= tol, describe_diff(tail, want, f"tail vs conv2d, 20 -> {cout}")


@pytest.mark.parametrize("cin", [16, 24])
def test_whole_chunks_keep_the_plain_tile(hip_lib, cin):
    """Cin % 8 == 0: no padded channel, the heuristic stays on d2_m1n2; and the tail variant refuses such a layer."""
    g = torch.Generator().manual_seed(cin)
    x = torch.rand(1, cin, 20, 36, generator=g) * 2 - 1
    wt = (torch.rand(64, cin, 3, 3, generator=g) * 2 - 1) / (cin * 9) ** 0.5
    b = torch.rand(64, generator=g) - 0.5
    _, rec = _conv_s2(hip_lib, x, wt, b, -1)
    assert rec[:2] == [2, PLAIN], rec
    xd = nhwc(x).cuda()
    out = torch.zeros(1, 10, 18, 64, device="cuda")
    assert hip_lib.vfi_conv3x3(ptr(xd), hptr(wt), hptr(b), None, ptr(out), 1, 20, 36, cin, 64, 2, 1, 0.2, LIVE4, None) != 0
