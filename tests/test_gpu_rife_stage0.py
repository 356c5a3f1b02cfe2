"""-m gpu: RIFE 4.7 block 0's input assembled from per-frame staging images against the per-pair gather it replaces, bit for bit.

At the standard scale list block 0's X is the 1/8 down-resize of cat(img0, img1, f0, f1, t): the 2x2 centre mean of every 8x8 cell
of each frame's pack.  The frame pack kernels (encode47_fused_kernel / encode47_batch_kernel, csrc/rife_ops.hip) now leave that mean
in a staging image per slot, and stage_in0 only lays two of them side by side; option stage0 = 0 keeps stage_in_kernel's gather.
Both use the same expressions (0.5 left + 0.5 right, then 0.5 top + 0.5 bottom): torch.equal on X and on the frames."""
import pytest
import torch

from cfi_amd import synth
from gpu_util import describe_diff
from oracle import rife_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sd():
    return synth.rife47_synth_state_dict(1234)


@pytest.fixture()
def eng(hip_lib, sd):
    from cfi_amd.rife import RifeEngine

    torch.cuda.set_device(0)
    e = RifeEngine(sd, "4.7")
    yield e
    hip_lib.vfi_test_set_option(b"stage0", 1)
    hip_lib.vfi_test_set_option(b"fuse_encode", 1)
    e.close()


def _frames(n, h, w, c, u8, seed):
    fr = synth.smooth_frames(n, h, w, seed=seed, shift=3.0, c=c)
    if c == 4:
        fr = fr * 1.3 - 0.15        # RGBA, values outside [0, 1]: the clamp
    if u8:
        fr = (fr.clamp(0, 1) * 255).round().to(torch.uint8)
    return [f.cuda().contiguous() for f in fr]


def _interp(eng, s0, s1, ts):
    h, w = eng.cfg[:2]
    out = torch.empty((len(ts), h, w, 3), device="cuda")
    eng.interpolate(s0, s1, ts, out)
    torch.cuda.synchronize()
    return out.cpu()


def _x0(eng, b):
    """block 0's input X of the last interpolate call (debug tap; planar4 [B][4][Hp/8][Wp/8][4])"""
    h, w = eng.cfg[:2]
    hp, wp = -(-h // 64) * 64, -(-w // 64) * 64
    return eng.debug_read(1, 0, b * (hp // 8) * (wp // 8) * 16)


@pytest.mark.parametrize("h,w,c,u8", [(64, 64, 3, False), (70, 90, 3, True), (200, 330, 4, False)])
def test_staged_block0_matches_gather(hip_lib, eng, h, w, c, u8):
    fr = _frames(3, h, w, c, u8, seed=h)
    eng.configure(h, w, 2, 4, 1.0)
    eng.debug_keep(True)
    eng.load_frames([0, 1, 2], fr)
    staged = _interp(eng, [0, 1], [1, 2], [0.5, 0.3])
    x_staged = _x0(eng, 2)
    assert hip_lib.vfi_test_set_option(b"stage0", 0) == 0
    gathered = _interp(eng, [0, 1], [1, 2], [0.5, 0.3])
    x_gathered = _x0(eng, 2)
    assert hip_lib.vfi_test_set_option(b"stage0", 1) == 0
    eng.debug_keep(False)
    fast = _interp(eng, [0, 1], [1, 2], [0.5, 0.3])      # without the taps: the fused last transition
    assert hip_lib.vfi_test_set_option(b"stage0", 0) == 0
    fast_gathered = _interp(eng, [0, 1], [1, 2], [0.5, 0.3])
    assert torch.equal(x_staged, x_gathered), describe_diff(x_staged, x_gathered, "block 0 X: staged vs gathered")
    assert x_staged.abs().max().item() > 0.1, "the tap read nothing"
    assert torch.equal(staged, gathered), describe_diff(staged, gathered, "frames: staged vs gathered")
    assert torch.equal(fast, fast_gathered), describe_diff(fast, fast_gathered, "frames (fused path): staged vs gathered")


def test_reloaded_slot_gets_a_new_staging_image(eng):
    h, w = 70, 90
    a, b, c = _frames(3, h, w, 3, False, seed=5)
    eng.configure(h, w, 1, 2, 1.0)
    eng.load_frames([0, 1], [a, b])
    first = _interp(eng, [0], [1], [0.5])
    eng.load_frame(0, c)                       # the node's ring reuses slots
    got = _interp(eng, [1], [0], [0.5])
    eng.configure(h, w, 1, 3, 1.0)             # another pool: as a fresh engine
    eng.load_frames([2, 0], [c, b])
    want = _interp(eng, [0], [2], [0.5])
    assert torch.equal(got, want), describe_diff(got, want, "pair (b, c) after slot 0 was reloaded")
    assert not torch.equal(got, first)


def test_single_frame_loads_match_the_batch_load(hip_lib, eng):
    h, w = 70, 90
    for u8 in (False, True):
        fr = _frames(3, h, w, 3, u8, seed=6)
        eng.configure(h, w, 2, 3, 1.0)
        eng.load_frames([0, 1, 2], fr)
        want = _interp(eng, [0, 1], [1, 2], [0.5, 0.3])
        eng.configure(h, w, 2, 4, 1.0)
        for s in (2, 0, 1):
            eng.load_frame(s, fr[s])
        got = _interp(eng, [0, 1], [1, 2], [0.5, 0.3])
        assert torch.equal(got, want), describe_diff(got, want, f"one-by-one vs batch load (u8={u8})")
    # a slot loaded through the three-kernel pack has no staging image: its pairs are gathered, same frames
    assert hip_lib.vfi_test_set_option(b"fuse_encode", 0) == 0
    eng.load_frame(1, fr[1])
    assert hip_lib.vfi_test_set_option(b"fuse_encode", 1) == 0
    mixed = _interp(eng, [0, 1], [1, 2], [0.5, 0.3])
    assert torch.equal(mixed, want), describe_diff(mixed, want, "slot 1 loaded by the three-kernel path")


def test_other_scale_lists_keep_the_gather(hip_lib, eng, sd):
    """scale_factor 2 -> block scales [4, 2, 1, 0.5]: block 0 is a 1/4 down-resize, which the staging images (1/8) cannot serve.  Both
    launches carry the trace name stage_in0, so the kernel taken is told by its result: X of block 0 has (Hp/4) x (Wp/4) cells, is the
    same with the option on and off, and the frames match the oracle."""
    from cfi_amd.rife import run_tasks

    h, w = 120, 200
    frames = synth.smooth_frames(2, h, w, seed=8, shift=3.0)
    tasks = [(0, 0.5), (0, 0.3)]
    eng.debug_keep(True)
    got = run_tasks(eng, frames, tasks, batch_size=2, scale_factor=2.0)
    n = 2 * (128 // 4) * (256 // 4) * 16
    x_on = eng.debug_read(1, 0, n)
    assert hip_lib.vfi_test_set_option(b"stage0", 0) == 0
    off = run_tasks(eng, frames, tasks, batch_size=2, scale_factor=2.0)
    x_off = eng.debug_read(1, 0, n)
    assert torch.equal(x_on, x_off) and torch.equal(got, off)
    # the last plane's third component is the timestep in every cell of the 1/4 grid
    xp = x_on.view(2, 4, 32, 64, 4)
    assert torch.equal(xp[0, 3, :, :, 2], torch.full((32, 64), 0.5)) and torch.equal(xp[1, 3, :, :, 2], torch.full((32, 64), 0.3))
    x = frames.permute(0, 3, 1, 2)
    ts = torch.tensor([0.5, 0.3]).view(-1, 1, 1, 1)
    with torch.inference_mode():
        want = rife_oracle.ifnet47_forward(sd, x[0:1].repeat(2, 1, 1, 1), x[1:2].repeat(2, 1, 1, 1), ts,
                                           (4.0, 2.0, 1.0, 0.5)).clamp(0, 1).permute(0, 2, 3, 1)
    assert (got - want).abs().max().item() <= 1e-3, describe_diff(got, want, "scale_factor 2")
