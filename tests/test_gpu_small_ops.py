"""-m gpu: the small ops underneath the RIFE 4.0, IFRNet, IFUNet and GMFSS nodes on the device library, against the float64
restatements, bounds and case tables of tests/small_ops_restated.py (pinned to the host build of the bodies and to the oracle's torch
expressions by tests/test_small_ops_restated_cpu.py):

  * every body-launched entry point of csrc/gmfss_ops.hip and csrc/ifunet_ops.hip at thread counts n with n % 256 != 0, n < 256 and
    n % 256 == 0 — on the device body_launch.h rounds the grid up and each body's own guard is what keeps the tail threads in bounds
    (the host build loops i < n and never runs a guard) — and with the device's ocml expf / tanhf / erff and FMA contraction;
  * vfi_bmm_nt's 4x4-tile body and its scalar body (K % 4 != 0, or an operand window offset by one float);
  * vfi_instnorm_stats' device kernels (instnorm_partial_wg_kernel for C <= 256, the body beyond; instnorm_final_wave_kernel), with
    idle lanes (C = 24, 96), empty strips, capped and non-power-of-two strip counts, and a mean-1000 / sigma-0.01 input;
  * csrc/rife40_ops.hip: each of the three warp kernels reached on purpose (C = 3; C % 4 == 0 on aligned windows; everything else,
    including C = 8 on a window offset by one float or with stride 9), |x| maximum bit for bit, input assembly, output blend.

Buffers (small_ops_restated.Buffers): every operand and output is a window of a NaN-surrounded body; all memory outside an output's
window must be bit-identical after the call.  Every toleranced case prints max err / tol.  One synchronize per case.
No kernel, body or entry point needed a fix: every case passed on its first MI355X run."""
import ctypes as C

import pytest
import torch

import small_ops_restated as so

pytestmark = pytest.mark.gpu


def _ck(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


def _run(lib, case):
    return so.run_case(lib, case, device="cuda", stream=C.c_void_p(torch.cuda.current_stream().cuda_stream), sync=torch.cuda.synchronize, check=_ck)


@pytest.mark.parametrize("case", so.BODY_CASES, ids=lambda c: c.id)
def test_body_launched_op(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", so.RIFE_CASES, ids=lambda c: c.id)
def test_rife40_op(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case,what", so.NEGATIVE_BODY + so.NEGATIVE_RIFE, ids=lambda v: v.id if isinstance(v, so.Case) else v.replace(" ", "-"))
def test_wrong_restatement_fails_on_the_device_result(hip_lib, case, what):
    with pytest.raises(AssertionError, match="outside the bound"):
        _run(hip_lib, case)
