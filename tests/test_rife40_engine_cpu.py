"""CPU: the orchestration of comfyui-frame-interpolation_amd/rife40.py (Rife40Engine.forward) against oracle.rife_oracle.ifnet40_forward
through the test double of the C ABI (tests/emu_backend.py: torch restatements of the entry points the engine uses; the convolution
launcher's contract is asserted on every layer call).  Same calls and the same bound as tests/test_gpu_rife.py's arch-4.0 tests."""
import pytest
import torch

from cfi_amd import synth
from emu_backend import EmuBackend
from oracle import rife_oracle

TOL = 1e-3        # tests/test_gpu_rife.py


@pytest.fixture(scope="module")
def sd40():
    return synth.rife40_synth_state_dict(1234)


def _run40(sd, frames, ts, scale_list, training, fastmode):
    from cfi_amd.rife40 import Rife40Engine

    eng = Rife40Engine(sd, _test_backend=EmuBackend())
    try:
        h, w = frames.shape[1:3]
        eng.configure(h, w, len(ts))
        f0, f1 = frames[0].contiguous(), frames[1].contiguous()
        out = torch.empty(len(ts), h, w, 3)
        eng.forward([f0] * len(ts), [f1] * len(ts), ts, scale_list, training, fastmode, out)
        return out, eng.lib.calls
    finally:
        eng.close()


def _oracle40(sd, frames, ts, scale_list, training, fastmode):
    x = frames.permute(0, 3, 1, 2)
    n = len(ts)
    with torch.inference_mode():
        want = rife_oracle.ifnet40_forward(sd, x[0:1].repeat(n, 1, 1, 1), x[1:2].repeat(n, 1, 1, 1), torch.tensor(ts).view(-1, 1, 1, 1),
                                           scale_list, training, fastmode)
    return want.clamp(0, 1).permute(0, 2, 3, 1)


@pytest.mark.parametrize("h,w,training,fastmode,sf", [(64, 64, True, True, 1.0), (100, 150, False, False, 1.0), (120, 200, False, True, 0.5)],
                         ids=["plain", "refine", "half_scale"])
def test_forward_matches_oracle(sd40, h, w, training, fastmode, sf):
    frames = synth.smooth_frames(2, h, w, seed=4, shift=3.0)
    ts = [0.5, 0.2]
    got, calls = _run40(sd40, frames, ts, [8 / sf, 4 / sf, 2 / sf, 1 / sf], training, fastmode)
    want = _oracle40(sd40, frames, ts, [8 / sf, 4 / sf, 2 / sf, 1 / sf], training, fastmode)
    d = (got - want).abs()
    assert d.max().item() <= TOL, f"rife 4.0 {h}x{w} training={training} fastmode={fastmode} sf={sf}: max {d.max().item()} mean {d.mean().item()}"
    # 4 blocks x 11 layers; the refinement adds 2 x 8 Contextnet convs, 8 Unet down convs, 4 deconvs and the last conv
    assert calls["vfi_conv_forward_ex"] == 44 + (0 if fastmode else 29)


def test_scale_doubling(sd40):
    """block-1 flows above 32 px in both directions with training=False: the block scales are doubled in place and blocks 0/1
    re-run (rife_arch.py:598-607); with training=True the same weights must NOT double.  (tests/test_gpu_rife.py::test_rife40_scale_doubling)"""
    big = {k: (v * 6.0 if "lastconv" in k and k[:6] in ("block0", "block1") else v) for k, v in sd40.items()}
    frames = synth.smooth_frames(2, 128, 192, seed=3, shift=2.5)
    for training in (False, True):
        sl_g, sl_o = [8.0, 4.0, 2.0, 1.0], [8.0, 4.0, 2.0, 1.0]
        got, calls = _run40(big, frames, [0.5], sl_g, training, False)
        want = _oracle40(big, frames, [0.5], sl_o, training, False)
        assert sl_g == sl_o == ([16.0, 8.0, 4.0, 2.0] if not training else [8.0, 4.0, 2.0, 1.0]), (training, sl_g, sl_o)
        d = (got - want).abs()
        assert d.max().item() <= TOL, f"rife 4.0 doubling training={training}: max {d.max().item()} mean {d.mean().item()}"
        assert calls["vfi_conv_forward_ex"] == 44 + 29 + (0 if training else 22)      # blocks 0 and 1 run twice


def test_workspace_follows_the_configured_shape(sd40):
    """configure() keeps the tensors of one shape only; release_workspace() drops them and the next configure() brings them back"""
    from cfi_amd.rife40 import Rife40Engine

    eng = Rife40Engine(sd40, _test_backend=EmuBackend())
    try:
        assert eng.workspace_bytes() == 0
        frames = synth.smooth_frames(2, 64, 64, seed=4, shift=3.0)
        outs = []
        for h, w in ((64, 64), (64, 128), (64, 64)):
            eng.configure(h, w, 1)
            base = eng.workspace_bytes()
            assert base == 4 * (64 * w * (8 + 8 + 4 + 4 + 1) + 2), "tensors of the previous shape were kept"
            if (h, w) == (64, 64):
                out = torch.empty(1, 64, 64, 3)
                eng.forward([frames[0].contiguous()], [frames[1].contiguous()], [0.5], [8.0, 4.0, 2.0, 1.0], True, True, out)
                outs.append(out)
                assert eng.workspace_bytes() > base
        assert torch.equal(outs[0], outs[1])
        eng.release_workspace()
        assert eng.workspace_bytes() == 0 and eng.cfg is None
    finally:
        eng.close()
