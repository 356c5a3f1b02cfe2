"""-m gpu: every launcher of the RIFE stage kernels (csrc/rife_ops.hip) on the device, one launcher per call through the
vfi_test_rife_* taps (include/vfi_hip_test.h), against the float64 restatements, bounds and case tables of tests/rife_stage_restated.py
(tied to the oracle by tests/test_rife_stage_restated_cpu.py):

  * stage_in (every HAS_FLOW x NP x NF x NX instantiation), stage_in0_staged (bit for bit), flow_up, feat_up;
  * the fused transitions stage_trans / stage_trans_x under stage_quad = 0 (cell kernels) and 14 (quad kernels: DPP exchanges, the LDS
    hand-over of centre pixels), has_prev on and off, and with the banded workgroup order xcd_bands = 1 at tile counts that are no
    multiple of 8; trans1_conv0a (the persistent MFMA kernel the product runs) in its live and its full form, weights packed by the
    library from plain OIHW; final_blend with and without Fdbg, cropped to H x W below the padding, plain and banded order;
  * planar4_up and t_down of the fractional block scales.

The fused kernels' second output is compared at the flow the device wrote (read back), so each comparison carries one stage's rounding.
Every buffer is a small_ops_restated.Buffers window between NaN guards: a stray write, a read outside an operand (the gap behind a
pack, the unused components of T) or a missing write fails the case.  The kernel of a case is launched ONCE: the negative test reuses
the result the case's own test left (and launches only when run alone).  Every toleranced comparison prints max err / tol."""
import ctypes as C

import pytest
import torch

import rife_stage_restated as rs

pytestmark = pytest.mark.gpu

_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def _forget_runs():
    yield
    _RUNS.clear()


def _ck(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _launch(lib, case):
    if case.id not in _RUNS:
        _RUNS[case.id] = rs.launch(lib, case, "cuda", _stream(), torch.cuda.synchronize, _ck)
    return _RUNS[case.id]


def _run(lib, case):
    assert rs.check(case, _launch(lib, case)) <= 1.0


@pytest.mark.parametrize("case", rs.STAGE_IN_CASES, ids=lambda c: c.id)
def test_stage_in(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", rs.STAGED_CASES, ids=lambda c: c.id)
def test_stage_in0_staged(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", rs.FLOW_UP_CASES, ids=lambda c: c.id)
def test_flow_up(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", rs.FEAT_UP_CASES, ids=lambda c: c.id)
def test_feat_up(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", rs.STAGE_TRANS_CASES, ids=lambda c: c.id)
def test_stage_trans(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", rs.STAGE_TRANS_X_CASES, ids=lambda c: c.id)
def test_stage_trans_x(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", rs.TRANS1_CASES, ids=lambda c: c.id)
def test_trans1_conv0a(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", rs.FINAL_BLEND_CASES, ids=lambda c: c.id)
def test_final_blend(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", rs.PLANAR4_UP_CASES, ids=lambda c: c.id)
def test_planar4_up(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", rs.T_DOWN_CASES, ids=lambda c: c.id)
def test_t_down(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("mut", list(rs.MUTATIONS), ids=lambda m: m)
def test_wrong_restatement_fails_on_the_device_result(hip_lib, mut):
    """each deliberately wrong restatement fails on the device result of EVERY case it applies to"""
    cases = [c for m, c in rs.NEGATIVE if m == mut]
    assert cases
    for case in cases:
        run = _launch(hip_lib, case)
        with pytest.raises(AssertionError, match="outside the bound|differ from the exact result"):
            rs.check(case, run, mut)


def test_wrappers_refuse_bad_arguments(hip_lib):
    """B = 0, B = 33, s_prev != 2 s_next, CX not matching NF: an error code and a message, and no launch — every buffer, guards and
    outputs alike, is bit-identical afterwards"""
    from cfi_amd import _lib

    case = next(c for c in rs.STAGE_TRANS_CASES if c.id.endswith("s4-q14-prev1-nf1-64x64"))
    B, op = rs.prepare(case, "cuda")
    name, args = op.calls[0]
    assert name == "vfi_test_rife_stage_trans"
    before = {k: b.dev.clone() for k, b in B.b.items()}
    fn = getattr(hip_lib, name)
    I = dict(B=5, s_prev=11, s_next=12, NF=13, CX=14)              # positions in the argument list
    assert args[I["B"]] == 3 and args[I["s_prev"]] == 8 and args[I["s_next"]] == 4 and args[I["NF"]] == 1 and args[I["CX"]] == 24
    bad = [("B = 0", {"B": 0}), ("B = 33", {"B": 33}), ("s_prev != 2 s_next", {"s_prev": 4}), ("s_prev != 2 s_next", {"s_prev": 16}),
           ("CX not matching NF", {"CX": 32}), ("CX not matching NF", {"NF": 2})]
    for what, change in bad:
        a = list(args)
        for k, v in change.items():
            a[I[k]] = v
        rc = fn(*a, _stream())
        assert rc == -2 and _lib.last_error(), f"{what}: returned {rc}"
    sin = next(c for c in rs.STAGE_IN_CASES if c.id.startswith("stage_in-flow1-s8-nf1-nx0"))
    B2, op2 = rs.prepare(sin, "cuda")
    before2 = {k: b.dev.clone() for k, b in B2.b.items()}
    a = list(op2.calls[0][1])
    assert a[-3] == 24 and a[-2] == 1
    for change in ({-3: 32}, {-2: 2}, {5: 0}, {5: 33}):
        b = list(a)
        for k, v in change.items():
            b[k] = v
        assert hip_lib.vfi_test_rife_stage_in(*b, _stream()) == -2
    tx = next(c for c in rs.STAGE_TRANS_X_CASES if c.id.endswith("s4-q14-prev1-nf1-192x64"))
    B3, op3 = rs.prepare(tx, "cuda")
    before3 = {k: b.dev.clone() for k, b in B3.b.items()}
    a = list(op3.calls[0][1])
    assert a[11] == 8 and a[12] == 4 and a[13] == 32
    for change in ({11: 4}, {13: 24}, {5: 0}, {5: 33}):
        b = list(a)
        for k, v in change.items():
            b[k] = v
        assert hip_lib.vfi_test_rife_stage_trans_x(*b, _stream()) == -2
    torch.cuda.synchronize()
    for bufs, was in ((B, before), (B2, before2), (B3, before3)):
        for k, b in bufs.b.items():
            assert torch.equal(b.dev.view(torch.int32), was[k].view(torch.int32)), f"{k} changed: a refused call launched"
