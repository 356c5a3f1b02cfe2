"""CPU: the case tables of tests/small_ops_restated.py through the HOST build of the bodies (tests/hostcheck: the same entry points of
csrc/gmfss_ops.hip / csrc/ifunet_ops.hip looping their bodies on the host), with the same buffers, bounds and conditions the MI355X
run (tests/test_gpu_small_ops.py) uses.  This proves without a GPU that the float64 restatements, the derived bounds, the
min-summand conditions and the 1 % cap on left-out occlusion bits hold for the chosen inputs.  The host loop is `i < n` exact, so
the launch-tail guards of the bodies are NOT exercised here: that is the GPU file's half.

csrc/rife40_ops.hip has no host build: its four restatements are checked against oracle.rife_oracle.warp and the torch expressions
of tests/emu_backend.py (|x| maximum and the output blend with a residual among them) within the same bounds.

Negative controls: each compares a case with a deliberately wrong restatement (a tap index off by one, a channel dropped from a
window, a softmax / blend term omitted) and must fail — the bounds are tight enough to see them."""
import ctypes as C

import pytest
import torch

import emu_backend
import hostcheck
import small_ops_restated as so


@pytest.fixture(scope="module")
def lib():
    return hostcheck.load()


class _Rife40Torch(emu_backend.EmuLib):
    """the RIFE 4.0 entry points as torch expressions on host memory (fp32): emu_backend's"""

    def __init__(self):          # no host library behind it: only the four RIFE 4.0 entry points are called
        pass

    def __getattribute__(self, name):
        fn = object.__getattribute__(self, name)
        if not name.startswith("vfi_"):
            return fn
        return lambda *a: fn(*[x.value if isinstance(x, C.c_float) else x for x in a])


@pytest.mark.parametrize("case", so.BODY_CASES, ids=lambda c: c.id)
def test_body_case_on_the_host_build(lib, case):
    so.run_case(lib, case)


@pytest.mark.parametrize("case", so.RIFE_CASES, ids=lambda c: c.id)
def test_rife40_restatement_against_torch(case):
    so.run_case(_Rife40Torch(), case)


@pytest.mark.parametrize("case,what", so.NEGATIVE_BODY, ids=lambda v: v.id if isinstance(v, so.Case) else v.replace(" ", "-"))
def test_wrong_restatement_fails_body(lib, case, what):
    with pytest.raises(AssertionError, match="outside the bound"):
        so.run_case(lib, case)


@pytest.mark.parametrize("case,what", so.NEGATIVE_RIFE, ids=lambda v: v.id if isinstance(v, so.Case) else v.replace(" ", "-"))
def test_wrong_restatement_fails_rife40(case, what):
    with pytest.raises(AssertionError, match="outside the bound"):
        so.run_case(_Rife40Torch(), case)


def test_every_entry_point_has_a_case():
    """the entry points of the issue's three holes each appear in a case id"""
    names = ("pad_rgb normalize_channels prelu_scalar instnorm_stats instnorm_apply gelu window_partition bmm_nt bmm_nn softmax_rows flow_sample "
             "resize_bilinear_ac convex_upsample gmfss_metric_inputs tanh_scale splat_prep splat_normalize pixel_shuffle2 clamp_crop convex_upsample_c "
             "lerp_mask add_clamp01 ifunet_blend fill_channels rife40_prep warp_rife absmax rife40_output").split()
    ops = {c.op for c in so.ALL_CASES}
    assert set(names) == ops
    ids = [c.id for c in so.ALL_CASES]
    assert len(ids) == len(set(ids))


class _FaultyLib:
    """vfi_fill_channels / vfi_prelu_scalar with one deliberate defect each: what the buffer harness must catch"""

    def __init__(self, defect):
        self.defect = defect

    def vfi_fill_channels(self, out_ptr, cs, c, px, v, stream):
        emu_backend.view(out_ptr, 1, 1, px, cs, c)[...] = v.value
        if self.defect == "missing write":
            emu_backend.view(out_ptr, 1, 1, px, cs, c)[0, 0, px - 1, c - 1] = float("nan")
        elif self.defect == "stray write into the next channel":
            emu_backend.view(out_ptr, 1, 1, px, cs, c + 1)[0, 0, 3, c] = v.value
        elif self.defect == "stray write one pixel past the end":
            emu_backend.view(out_ptr, 1, 1, px + 1, cs, c)[0, 0, px, 0] = v.value
        elif self.defect == "stray write 255 elements past the end":
            emu_backend.view(out_ptr, 1, 1, px + 85, cs, c)[0, 0, px + 84, c - 1] = v.value
        return 0

    def vfi_prelu_scalar(self, in_ptr, in_cs, out_ptr, out_cs, c, px, slope, stream):
        shift = 1 if self.defect == "read one channel outside the window" else 0
        x = emu_backend.view(in_ptr + 4 * shift, 1, 1, px, in_cs, c)
        emu_backend.view(out_ptr, 1, 1, px, out_cs, c).copy_(torch.where(x > 0, x, x * slope.value))
        if self.defect == "write into the input":
            emu_backend.view(in_ptr, 1, 1, px, in_cs, c)[0, 0, 0, 0] = 0.0
        return 0


@pytest.mark.parametrize("op,defect,message", [
    ("fill_channels", None, None), ("prelu_scalar", None, None),
    ("fill_channels", "missing write", "got nan"), ("fill_channels", "stray write into the next channel", "outside the window changed"),
    ("fill_channels", "stray write one pixel past the end", "outside the window changed"),
    ("fill_channels", "stray write 255 elements past the end", "outside the window changed"),
    ("prelu_scalar", "read one channel outside the window", "differ from the exact result"), ("prelu_scalar", "write into the input", "outside the window changed")],
    ids=lambda v: str(v).replace(" ", "-"))
def test_buffer_harness_catches(op, defect, message):
    case = next(c for c in so.BODY_CASES if c.op == op and c.id.endswith("n513"))
    if defect is None:
        so.run_case(_FaultyLib(None), case)
        return
    with pytest.raises(AssertionError, match=message):
        so.run_case(_FaultyLib(defect), case)
