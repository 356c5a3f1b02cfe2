"""netengine.NetEngine without a GPU: a fake library object stands in for libvfi_hip.so."""
import ctypes as C
from collections import OrderedDict

import pytest
import torch

from cfi_amd import _lib, netengine


class FakeLib:
    """vfi_fake_* entry points that record their calls.  ``handle``: what vfi_fake_create returns (None = a failed create)."""

    def __init__(self, handle=0x1234, error=b"vfi_fake_create: tensor 1 has 5 elements, expected 6"):
        self.handle, self.error = handle, error
        self.created, self.destroyed, self.released, self.inits = [], [], [], []
        self.destroy_raises = False
        self.bytes = 4096

    def vfi_init(self, device):
        self.inits.append(device)
        return 0

    def vfi_last_error(self):
        return self.error

    def vfi_fake_create(self, ptrs, numels, n, *extra):
        # the engine keeps the host tensors alive only for the length of this call: read them here
        firsts = [C.cast(ptrs[i], C.POINTER(C.c_float))[0] for i in range(n)]
        self.created.append((firsts, [numels[i] for i in range(n)], n, extra))
        return self.handle

    def vfi_fake_destroy(self, handle):
        if self.destroy_raises:
            raise OSError("library already unloaded")
        self.destroyed.append(handle)

    def vfi_fake_release_workspace(self, handle):
        self.released.append(handle)
        return 0

    def vfi_fake_workspace_bytes(self, handle):
        return self.bytes


class FakeEngine(netengine.WorkspaceBytes, netengine.NetEngine):
    PREFIX, LABEL = "vfi_fake", "Fake"
    checked = None

    def shapes(self):
        return OrderedDict([("b", (2, 3)), ("a", (1,)), ("c", (4,))])

    def check_state_dict(self, state_dict):
        self.checked = sorted(state_dict)


STATE = {"a": torch.full((1,), 10.0), "c": torch.full((4,), 30.0, dtype=torch.float64), "b": torch.full((2, 3), 20.0), "unused": torch.zeros(7)}


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    return lib


def test_tensors_go_in_shapes_order_with_their_numels(fake):
    e = FakeEngine(STATE, None, 7)
    assert fake.inits == [0] and e.device == torch.device("cuda", 0)
    assert e.checked == ["a", "b", "c", "unused"]
    assert fake.created == [([20.0, 10.0, 30.0], [6, 1, 4], 3, (7,))]      # shapes() order b, a, c; float64 converted to float32
    assert e.handle == fake.handle
    e.close()


def test_null_handle_raises_with_the_library_error(fake):
    fake.handle = None
    with pytest.raises(RuntimeError, match="vfi_fake_create failed: vfi_fake_create: tensor 1 has 5 elements, expected 6"):
        FakeEngine(STATE)
    assert fake.destroyed == []


def test_no_gpu_message(fake, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match=r"^Fake VFI \(HIP\): no GPU visible; this node has no CPU fallback$"):
        FakeEngine(STATE)


def test_close_is_idempotent_and_workspace_bytes_is_zero_after_it(fake):
    e = FakeEngine(STATE)
    assert e.workspace_bytes() == 4096
    e.release_workspace()
    assert fake.released == [fake.handle]
    e.close()
    e.close()
    assert fake.destroyed == [fake.handle] and e.handle is None
    assert e.workspace_bytes() == 0


def test_del_swallows_errors(fake):
    e = FakeEngine(STATE)
    fake.destroy_raises = True
    e.__del__()
    half_built = FakeEngine.__new__(FakeEngine)      # __init__ raised before a handle existed
    half_built.__del__()
    assert half_built.workspace_bytes() == 0
    fake.destroy_raises = False
    e.close()


def test_failed_status_raises_with_the_entry_point_name(fake):
    e = FakeEngine(STATE)
    fake.vfi_fake_release_workspace = lambda handle: -1
    with pytest.raises(RuntimeError, match=r"vfi_fake_release_workspace failed \(code -1\)"):
        e.release_workspace()
    e.close()


def test_which_engines_report_their_workspace():
    from cfi_amd.amt import AmtEngine
    from cfi_amd.atm import AtmEngine
    from cfi_amd.cain import CainEngine
    from cfi_amd.film import FilmEngine
    from cfi_amd.flavr import FlavrEngine
    from cfi_amd.m2m import M2MEngine
    from cfi_amd.sepconv import SepconvEngine
    from cfi_amd.xvfi import XvfiEngine

    assert not hasattr(FilmEngine, "workspace_bytes")      # ckpt.end_call: hasattr -> FILM's 15 GB are released after every call
    for cls in (M2MEngine, CainEngine, SepconvEngine, FlavrEngine, AmtEngine, AtmEngine, XvfiEngine):
        assert hasattr(cls, "workspace_bytes") and issubclass(cls, netengine.NetEngine)
    assert FilmEngine.__del__ is netengine.NetEngine.__del__


def test_frame_pair_check(monkeypatch):
    """check_frames, behind frame_ptrs and the AMT / ATM / XVFI forwards: a mismatched shape, a non-fp32 and a non-contiguous frame raise;
    so does a host tensor (the is_cuda leg, the only one a machine without a GPU reaches with real tensors); with that leg answered, a
    good pair gives (H, W, C) and each of the other legs still fires."""
    good = torch.zeros(4, 6, 3)
    text = r"frames: \[H,W,C\] fp32 contiguous"
    with pytest.raises(AssertionError, match=text):
        netengine.check_frames(good, good)                  # host tensors: is_cuda
    with pytest.raises(AssertionError, match=text):
        netengine.frame_ptrs([good])
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    assert netengine.check_frames(good, good.clone()) == (4, 6, 3)
    assert netengine.frame_ptrs([good, good])[1] == (4, 6, 3)
    for bad in (torch.zeros(4, 5, 3), good.double(), torch.zeros(4, 6, 6)[..., ::2]):
        assert bad.shape != good.shape or bad.dtype != torch.float32 or not bad.is_contiguous()
        with pytest.raises(AssertionError, match=text):
            netengine.check_frames(good, bad)


def test_m2m_release_workspace_forgets_the_prepared_pair(fake):
    from cfi_amd.m2m import M2MEngine

    fake.vfi_m2m_release_workspace = lambda handle: 0
    e = M2MEngine.__new__(M2MEngine)
    e.lib, e.handle, e.hw = fake, 1, (64, 64)
    e.release_workspace()
    assert e.hw is None
    e.handle = None
