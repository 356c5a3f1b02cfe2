"""-m gpu: the GMFlow device kernels of the GMFSS node (csrc/attention.hip: attention_kernel<4> / <1>, attention_merge_kernel, the
window addressing, the key split; csrc/gmfss_fast.hip: layernorm_wave_kernel, local_match_mfma_kernel, local_prop_coop_kernel) on the
device library against the float64 restatements, per-element bounds and case tables of tests/gmflow_restated.py (pinned to the oracle
and to the host build of the bodies by tests/test_gmflow_restated_cpu.py).

Every operand and output is a channel window of a NaN-filled, guarded body: inputs must come back bit-identical, outputs untouched
outside their window.  The key split is forced through the A/B option att_ksplit (set and restored to 0 around each call by
gmflow_restated.run_case).  Every case prints max err / tol.  Each (case, wrong restatement) pair of gmflow_restated.NEGATIVE must
fail the comparison on the device result.

No kernel, launcher or entry point needed a fix: every case passed on its first MI355X run, and no bound constant was changed after it.
Worst err / tol measured: vfi_attention 0.048 (split forced: 0.035), vfi_window_attention 0.112, vfi_local_match 0.309,
vfi_local_propagate 0.206, vfi_layernorm[_add] 0.472 (docs/design/gmflow_coverage.md)."""
import ctypes as C

import pytest
import torch

import gmflow_restated as gr

pytestmark = pytest.mark.gpu


def _ck(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


def _run(lib, case, mut=None, results=None):
    return gr.run_case(lib, case, device="cuda", stream=C.c_void_p(torch.cuda.current_stream().cuda_stream), sync=torch.cuda.synchronize, check=_ck, mut=mut,
                       results=results)


@pytest.fixture(autouse=True)
def _automatic_key_split(hip_lib):
    yield
    hip_lib.vfi_test_set_option(b"att_ksplit", 0)


@pytest.mark.parametrize("case", gr.ATT_CASES, ids=lambda c: c.id)
def test_attention(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.WIN_CASES, ids=lambda c: c.id)
def test_window_attention(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.LM_CASES, ids=lambda c: c.id)
def test_local_match(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.LP_CASES, ids=lambda c: c.id)
def test_local_propagate(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case", gr.LN_CASES, ids=lambda c: c.id)
def test_layernorm(hip_lib, case):
    _run(hip_lib, case)


@pytest.mark.parametrize("case,mut", gr.NEGATIVE, ids=lambda v: v.id if isinstance(v, gr.Case) else v.replace(" ", "-"))
def test_wrong_restatement_fails_on_the_device_result(hip_lib, case, mut):
    with pytest.raises(AssertionError, match="outside the bound"):
        _run(hip_lib, case, mut)


@pytest.mark.parametrize("dv", [128, 2])
def test_forced_split_is_read(hip_lib, dv):
    """the same noise inputs with att_ksplit 1 and 8: both inside the bound, and NOT the same bits anywhere — eight partial sums rescaled
    and merged are another fp32 association of 2 x 129 x dv sums of 256 terms; equal bits would mean the launcher ignores the option"""
    base = next(c for c in gr.ATT_CASES if c.id == f"dv{dv}-split8-runs8-2x129x256-planted".join(("attention-", "")))
    outs = {}
    for ks in (1, 8):
        case = gr.Case("attention", f"forced{ks}", **{**base.p, "kind": "noise", "ks": ks, "ks_ran": ks})
        got = {}
        _run(hip_lib, case, results=got)
        outs[ks] = got["out"]
    assert not torch.equal(outs[1], outs[8])
