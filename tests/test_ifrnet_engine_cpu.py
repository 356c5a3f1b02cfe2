"""CPU: the orchestration of comfyui-frame-interpolation_amd/ifrnet.py (IFRNetEngine.forward) against oracle.ifrnet_oracle.ifrnet_forward
through the test double of the C ABI (tests/emu_backend.py: torch restatements of the entry points the engine uses; the convolution
launcher's contract is asserted on every layer call, so a channel window or a ``chan_map`` layout the MI355X launcher would refuse
fails here).  Same calls and the same bound as tests/test_gpu_ifrnet.py::test_engine_against_oracle."""
import pytest
import torch

from cfi_amd import synth
from emu_backend import EmuBackend
from oracle import ifrnet_oracle

TOL = 1e-3        # tests/test_gpu_ifrnet.py


@pytest.fixture(scope="module", params=["L", "S"])
def net(request):
    from cfi_amd.ifrnet import IFRNetEngine

    kind = request.param
    sd = synth.ifrnet_synth_state_dict(kind, 1234)
    e = IFRNetEngine(sd, kind, _test_backend=EmuBackend())
    yield kind, sd, e
    e.close()


def _pairs(fr, n):
    return [fr[2 * k].contiguous() for k in range(n)], [fr[2 * k + 1].contiguous() for k in range(n)]


@pytest.mark.parametrize("h,w,n,sf,t", [(64, 64, 1, 1.0, 0.5), (100, 150, 2, 0.5, 1.0), (72, 100, 1, 0.75, 1.0)], ids=["minimal", "batched", "odd_ratio"])
def test_forward_matches_oracle(net, h, w, n, sf, t):
    kind, sd, e = net
    fr = synth.smooth_frames(2 * n, h, w, seed=h + n, shift=2.5)
    i0, i1 = fr[0::2].permute(0, 3, 1, 2).contiguous(), fr[1::2].permute(0, 3, 1, 2).contiguous()
    with torch.inference_mode():
        want = ifrnet_oracle.ifrnet_forward(sd, i0, i1, sf, t).permute(0, 2, 3, 1).contiguous()
    if (h, w) == (72, 100):
        assert e.geometry(h, w, sf)[:4] == (128, 128, 96, 96), "test premise: a working resolution that is no power-of-two fraction of the frame"
    out = torch.empty(n, h, w, 3)
    e.forward(*_pairs(fr, n), sf, t, out)
    d = (out - want).abs()
    assert d.max().item() <= TOL, f"IFRNet_{kind} {h}x{w} n={n} sf={sf} t={t}: max {d.max().item()} mean {d.mean().item()}"
    e.release_workspace()


def test_rejects_what_the_reference_rejects(net):
    kind, sd, e = net
    fr = synth.smooth_frames(2, 64, 64, seed=1)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        e.forward(*_pairs(fr, 1), 1.0 / 3.0, 1.0, torch.empty(1, 64, 64, 3))      # 21x21 working resolution: torch.cat fails in the reference


def test_repeated_call_is_bit_identical_on_the_kept_scratch(net):
    """the scratch tensors of a shape are allocated (zeroed) once and kept: a second call runs on the first one's leftovers — same output
    bit for bit, no growth — and release_workspace() gives all of it back"""
    kind, sd, e = net
    e.release_workspace()
    assert e.workspace_bytes() == 0
    fr = synth.smooth_frames(4, 64, 96, seed=5, shift=2.0)
    outs = []
    for pair in (0, 1, 0):
        o = torch.empty(1, 64, 96, 3)
        e.forward([fr[2 * pair].contiguous()], [fr[2 * pair + 1].contiguous()], 0.5, 1.0, o)
        outs.append(o)
        if len(outs) == 1:
            used = e.workspace_bytes()
            assert used > 0
    assert torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[1])
    assert e.workspace_bytes() == used, "the workspace keeps growing"
    e.prepare(fr[0].contiguous(), fr[1].contiguous())
    assert torch.equal(e.render(0.5, torch.empty(64, 96, 3)), outs[0][0])      # the (pair, timestep) interface: same call
    e.release_workspace()
    assert e.workspace_bytes() == 0 and e._pair is None
