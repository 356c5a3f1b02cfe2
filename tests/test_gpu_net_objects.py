"""-m gpu: what the eight whole-network objects (FILM, M2M, CAIN, Sepconv, FLAVR, AMT, ATM, XVFI) get from their shared base
(csrc/net_object.h, netengine.py), on seeded weights.

Malformed checkpoints are refused by host-side argument validation, not read: a wrong tensor count, a wrong element count in the LAST
tensor (every earlier layer exists by then and the failed create must tear it down), a null tensor pointer in the middle.

Workspace lifecycle: forward at shape A, at B, at A again, release, A once more — the three A frames are bit-equal.  The re-allocation at A
after B is where a lost zero fill would show (FILM and M2M read zero channel padding, FLAVR zero borders).  The shapes are the smallest
that reach every branch: FILM's 7-level minimum of 64; M2M padded to 128x128 / 64x128; CAIN two padded sizes with reflection on both
axes; Sepconv odd rows (the cropped residual add) / even ones; FLAVR padded 48x64 / 64x80; AMT-S 120x136 (padded 128x144, top and left
4: its 128-pixel minimum side binds) / 128x160; ATM-lite 40x100 (padded 64x128) / 64x64; XVFI (2, 1) 40x56 (padded bottom / right to
48x64) / 64x80, whose second and third run at A go through the kept-pair path."""
import ctypes as C
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

# create: the raw create entry point where it is not PREFIX_create; engine_args: what the engine takes after the state dict
Net = namedtuple("Net", "engine state_dict keys create_args frames run shape_a shape_b create engine_args", defaults=(None, ()))
NAMES = ["film", "m2m", "cain", "sepconv", "flavr", "amt", "atm", "xvfi"]


def _net(name):
    from cfi_amd import synth

    pair = lambda e, f: e.forward([f[0]], [f[1]])[0]       # noqa: E731
    if name == "film":
        from cfi_amd.film import FilmEngine
        from cfi_amd.film_spec import film_shapes

        return Net(FilmEngine, synth.film_synth_state_dict(1234), list(film_shapes()), (), 2, lambda e, f: e.forward(f[0], f[1]), (64, 96), (72, 64))
    if name == "m2m":
        from cfi_amd.m2m import M2MEngine
        from cfi_amd.m2m_spec import m2m_shapes

        return Net(M2MEngine, synth.m2m_synth_state_dict(1234), list(m2m_shapes()), (), 2, lambda e, f: e.forward(f[0], f[1], 0.5), (70, 100), (64, 128))
    if name == "cain":
        from cfi_amd.cain import CainEngine
        from cfi_amd.cain_spec import cain_shapes

        return Net(CainEngine, synth.synth_state_dict(cain_shapes()), list(cain_shapes()), (), 2, pair, (96, 136), (130, 100))
    if name == "sepconv":
        from cfi_amd.sepconv import SepconvEngine
        from cfi_amd.sepconv_spec import seeded_state_dict, sepconv_shapes

        return Net(SepconvEngine, seeded_state_dict(1), list(sepconv_shapes()), (), 2, pair, (67, 99), (64, 96))
    if name == "amt":
        from cfi_amd.amt import AmtEngine
        from cfi_amd.amt_spec import amt_shapes, seeded_state_dict

        return Net(AmtEngine, seeded_state_dict("S", 1), list(amt_shapes("S")), (0,), 2, lambda e, f: e.forward(f[0], f[1], [0.5])[0], (120, 136), (128, 160))
    if name == "atm":
        from cfi_amd.atm import AtmEngine
        from cfi_amd.atm_spec import seeded_state_dict, weight_shapes

        return Net(AtmEngine, seeded_state_dict(1), list(weight_shapes("lite")), (0,), 2, lambda e, f: e.forward(f[0], f[1]), (40, 100), (64, 64),
                   create="vfi_atm_create_variant")
    if name == "xvfi":
        from cfi_amd.xvfi import XvfiEngine
        from cfi_amd.xvfi_spec import seeded_state_dict, xvfi_shapes

        return Net(XvfiEngine, seeded_state_dict((2, 1), 1), list(xvfi_shapes(2)), (2, 1), 2, lambda e, f: e.forward(f[0], f[1], 0.5), (40, 56), (64, 80),
                   engine_args=((2, 1),))
    from cfi_amd.flavr import FlavrEngine
    from cfi_amd.flavr_spec import flavr_shapes, seeded_state_dict

    return Net(FlavrEngine, seeded_state_dict(1, 1), list(flavr_shapes(1)), (1,), 4, lambda e, f: e.forward(list(f))[0], (40, 56), (64, 80))


@pytest.fixture(scope="module")
def nets(hip_lib):
    from cfi_amd import _lib

    _lib.check(hip_lib.vfi_init(0), "vfi_init")
    made = {}

    def get(name):
        if name not in made:
            made[name] = _net(name)
        return made[name]

    return get


@pytest.mark.parametrize("name", NAMES)
def test_malformed_checkpoint_is_refused(hip_lib, nets, name):
    from cfi_amd import _lib

    net = nets(name)
    prefix = net.engine.PREFIX
    create, destroy = getattr(hip_lib, net.create or prefix + "_create"), getattr(hip_lib, prefix + "_destroy")
    tensors = [net.state_dict[k].detach().to("cpu", torch.float32).contiguous() for k in net.keys]
    n = len(tensors)

    def attempt(n_tensors=n, numel_delta=None, null_at=None):
        ptrs = (C.c_void_p * n)(*[None if i == null_at else t.data_ptr() for i, t in enumerate(tensors)])
        numels = (C.c_int64 * n)(*[t.numel() + (numel_delta if i == n - 1 and numel_delta else 0) for i, t in enumerate(tensors)])
        return create(ptrs, numels, n_tensors, *net.create_args)

    assert not attempt(n_tensors=n - 1)
    assert prefix + "_create" in _lib.last_error(), _lib.last_error()
    assert not attempt(numel_delta=1)
    err = _lib.last_error()
    assert prefix + "_create" in err and f"tensor {n - 1} " in err, err
    assert not attempt(null_at=n // 2)
    err = _lib.last_error()
    assert prefix + "_create" in err and f"tensor {n // 2} " in err and "null" in err, err
    handle = attempt()
    assert handle, _lib.last_error()
    destroy(handle)


@pytest.mark.parametrize("name", NAMES)
def test_workspace_lifecycle(nets, name):
    from cfi_amd import synth

    net = nets(name)
    fa = synth.texture_frames(net.frames, *net.shape_a, seed=3).cuda()
    fb = synth.texture_frames(net.frames, *net.shape_b, seed=4).cuda()
    eng = net.engine(net.state_dict, *net.engine_args)
    try:
        reports = hasattr(eng, "workspace_bytes")
        assert reports == (name != "film"), "FILM's object reports no workspace size (ckpt.end_call then always releases it)"
        a1 = net.run(eng, fa).clone()
        assert a1.shape == net.shape_a + (3,) and torch.isfinite(a1).all()
        assert not reports or eng.workspace_bytes() > 0
        b = net.run(eng, fb)
        assert b.shape == net.shape_b + (3,) and torch.isfinite(b).all()
        a2 = net.run(eng, fa).clone()
        torch.cuda.synchronize()
        eng.release_workspace()
        assert not reports or eng.workspace_bytes() == 0
        a3 = net.run(eng, fa)
        assert not reports or eng.workspace_bytes() > 0
        assert torch.equal(a1, a2), "shape A after shape B differs from the first run at A"
        assert torch.equal(a1, a3), "shape A after release_workspace differs from the first run at A"
    finally:
        eng.close()
