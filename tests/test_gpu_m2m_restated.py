"""-m gpu: every M2M entry point of csrc/m2m_net.hip, csrc/m2m_render.hip and the summation splat of csrc/m2m_ops.hip, launched alone
through the C ABI and compared element by element with the float64 restatements, counted bounds and case tables of tests/m2m_restated.py
(held to the oracle, with their branch conditions, by tests/test_m2m_restated_cpu.py; launch branch -> case: docs/design/m2m_coverage.md).

Buffers (small_ops_restated.Buffers): every operand and output is a window of a NaN-surrounded body; all memory outside an output's window
must be bit-identical after the call.  Every toleranced case prints max err / tol.  One synchronize per case.  The A/B options of a splat
case (splat_atomic, splat_spill_cap) are set in-process and restored in `finally`."""
import ctypes as C

import pytest
import torch

import m2m_restated as mr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_lib):
    from cfi_amd import _lib

    _lib.check(hip_lib.vfi_init(0), "vfi_init")
    return hip_lib


def _ck(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


def _run(lib, case):
    return mr.run_case(lib, case, "cuda", C.c_void_p(torch.cuda.current_stream().cuda_stream), torch.cuda.synchronize, _ck)


@pytest.mark.parametrize("case", mr.WARP_CASES, ids=lambda c: c.id)
def test_backwarp(lib, case):
    _run(lib, case)


@pytest.mark.parametrize("case", mr.PHOTO_CASES, ids=lambda c: c.id)
def test_photo_and_photo_tiles(lib, case):
    _run(lib, case)


@pytest.mark.parametrize("case", mr.SPLAT_CASES, ids=lambda c: c.id)
def test_softsplat_sum(lib, case):
    _run(lib, case)


@pytest.mark.parametrize("case", mr.SPLAT_INPUTS_CASES, ids=lambda c: c.id)
def test_splat_inputs(lib, case):
    _run(lib, case)


@pytest.mark.parametrize("case", mr.COMBINE_CASES, ids=lambda c: c.id)
def test_combine_on_a_crafted_splat(lib, case):
    _run(lib, case)


@pytest.mark.parametrize("case", mr.RENDER_CASES, ids=lambda c: c.id)
def test_render_three_step_and_fused(lib, case):
    _run(lib, case)


@pytest.mark.parametrize("case", mr.CUBE_CASES + mr.POOL_CASES + mr.NORMALIZE_CASES, ids=lambda c: c.id)
def test_cube_pool_normalize(lib, case):
    _run(lib, case)


@pytest.mark.parametrize("case,what", mr.MUTATIONS, ids=lambda v: v.id if isinstance(v, mr.Case) else v)
def test_wrong_restatement_fails_on_the_device_result(lib, case, what):
    with pytest.raises(AssertionError, match="outside the bound|differ from the exact result"):
        _run(lib, case)


def test_render_fused_refuses_what_its_ranges_cannot_cover(lib):
    """t outside [0, 1] (the tile ranges scale with it) and Hp < H are refused before anything is launched"""
    z = torch.zeros(8 * 32 * 32 * 4, device="cuda")
    out = torch.full((32 * 32 * 3,), float("nan"), device="cuda")
    p = z.data_ptr()
    for t, hp, h in ((1.5, 32, 32), (-0.25, 32, 32), (float("nan"), 32, 32), (0.5, 16, 32)):
        assert lib.vfi_m2m_render_fused(p, p, p, p, p, p, t, out.data_ptr(), hp, 32, h, 32, None) != 0, (t, hp, h)
    assert lib.vfi_m2m_combine(p, p, 8, p, 0.5, out.data_ptr(), 16, 32, 32, 32, None) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
