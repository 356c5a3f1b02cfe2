"""-m gpu: every entry point of csrc/gen_ops.hip, csrc/ifrnet_ops.hip and the cooperative CBAM kernels of csrc/ifunet_fast.hip, launched
alone on the device library against the float64 restatements, per-element bounds and case tables of tests/gen_ops_restated.py (pinned
to the oracle and, for CBAM, to the host build of the bodies by tests/test_gen_ops_restated_cpu.py).

Every operand and output is a channel window of a NaN-filled, guarded body: inputs must come back bit-identical, outputs and in-place
operands untouched outside their window, no output element left NaN; one synchronize per case.  Every toleranced case prints
max err / tol.  Each (case, wrong restatement) pair of gen_ops_restated.NEGATIVE must fail on the device result with "outside the
bound".  The refusals launch nothing: each returns non-zero and the buffers it was given come back bit-identical.

Measured worst err / tol per entry point, and what changed after the first device run: docs/design/gen_ops_coverage.md."""
import ctypes as C

import pytest
import torch

import gen_ops_restated as gr

pytestmark = pytest.mark.gpu
IDS = dict(ids=lambda v: v.id if isinstance(v, gr.Case) else str(v).replace(" ", "-"))


def _ck(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


def _run(lib, case, mut=None):
    return gr.run_case(lib, case, device="cuda", stream=C.c_void_p(torch.cuda.current_stream().cuda_stream), sync=torch.cuda.synchronize, check=_ck, mut=mut)


@pytest.mark.parametrize("case", gr.AVGPOOL_CASES, **IDS)
def test_avgpool2(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.NEAREST_CASES, **IDS)
def test_upsample_nearest(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.BILINEAR_CASES, **IDS)
def test_resize_bilinear(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.FILM_CASES, **IDS)
def test_warp_film(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.AXPBY_CASES, **IDS)
def test_axpby(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.PREP_CASES, **IDS)
def test_ifrnet_prep(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.CENTER_CASES, **IDS)
def test_ifrnet_center(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.CONV7_CASES, **IDS)
def test_conv7x7s2_prelu_64(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.SIGMOID_CASES, **IDS)
def test_sigmoid(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.FILL_CASES, **IDS)
def test_fill_items(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.RATIO_CASES, **IDS)
def test_resize_bilinear_ratio(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.OUTPUT_CASES, **IDS)
def test_ifrnet_output(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.POOL_CASES, **IDS)
def test_channel_pool(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.GATE_CASES, **IDS)
def test_cbam_gate(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.SCALE_CASES, **IDS)
def test_cbam_scale_compress(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.SPATIAL_CASES, **IDS)
def test_cbam_spatial(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case,mut", gr.NEGATIVE, **IDS)
def test_wrong_restatement_fails_on_the_device_result(hip_lib, case, mut):
    with pytest.raises(AssertionError, match="outside the bound"):
        _run(hip_lib, case, mut)


def test_refusals_launch_nothing(hip_lib):
    """bad arguments return non-zero before any launch: the sizes, strides and window alignments the float4 kernels rely on, Cout = 32 of
    the 7x7 head, 65 items, a channel-pool workspace one byte short of 64 strips"""
    from cfi_amd import _lib

    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a, b = (torch.full((4096,), float("nan"), device="cuda") for _ in range(2))
    before = [t.cpu().view(torch.int32) for t in (a, b)]
    for name, why, args in gr.refusals(a.data_ptr(), b.data_ptr()):
        assert getattr(hip_lib, name)(*args, st) != 0, f"{name} accepted {why}"
        assert name in _lib.last_error(), (name, why, _lib.last_error())
    B, calls, _ = gr._build(gr.POOL_REFUSED, None, "cuda")
    assert hip_lib.vfi_channel_pool(*calls[0][1], st) != 0 and "workspace too small" in _lib.last_error()
    torch.cuda.synchronize()
    for t, was in zip((a, b), before):
        assert torch.equal(t.cpu().view(torch.int32), was)
    for buf in B.b.values():
        buf.win[:] = False          # nothing may have been written anywhere
    B.finish()
