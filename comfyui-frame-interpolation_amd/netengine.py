"""What the Python engines of the whole-network C objects share (FILM, M2M, CAIN, Sepconv, FLAVR, AMT, ATM, XVFI; csrc/net_object.h is
the C side).

A subclass names its entry points (``PREFIX``: ``vfi_cain`` -> vfi_cain_create / _destroy / _release_workspace ...), its node (``LABEL``)
and its checkpoint layout (``shapes``), and writes its own forward.  Engines whose object reports its workspace size add
``WorkspaceBytes``: ckpt.end_call keeps such a workspace between calls when it is small and always releases the others' (FILM's 15 GB).
"""
import ctypes as C

import torch

from . import _lib


class NetEngine:
    PREFIX = None       # "vfi_film", ...
    LABEL = None        # "FILM", ...: the node's name in messages

    def shapes(self):
        """Ordered {state_dict key: shape}: the tensors the create function takes, in its order."""
        raise NotImplementedError

    def check_state_dict(self, state_dict):
        """Optional: raise on a checkpoint of another model, before anything is packed."""

    def __init__(self, state_dict, device=None, *create_args):
        if not torch.cuda.is_available():
            raise RuntimeError(f"{self.LABEL} VFI (HIP): no GPU visible; this node has no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        _lib.check(self.lib.vfi_init(self.device.index or 0), "vfi_init")
        self.check_state_dict(state_dict)
        keys = list(self.shapes().keys())
        tensors = [state_dict[k].detach().to("cpu", torch.float32).contiguous() for k in keys]
        ptrs = (C.c_void_p * len(keys))(*[t.data_ptr() for t in tensors])
        numels = (C.c_int64 * len(keys))(*[t.numel() for t in tensors])
        self.handle = self._fn("create")(ptrs, numels, len(keys), *create_args)
        if not self.handle:
            raise RuntimeError(f"{self.PREFIX}_create failed: " + _lib.last_error())

    def _fn(self, name):
        return getattr(self.lib, f"{self.PREFIX}_{name}")

    def _call(self, name, *args):
        """A status-returning entry point on this object; raises with the library's error text."""
        _lib.check(self._fn(name)(self.handle, *args), f"{self.PREFIX}_{name}")

    def close(self):
        if getattr(self, "handle", None):
            self._fn("destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def release_workspace(self):
        """Drop the activations; the packed weights stay on the device."""
        self._call("release_workspace")


class WorkspaceBytes:
    """For engines whose object has a ``*_workspace_bytes`` entry point."""

    def workspace_bytes(self):
        return int(self._fn("workspace_bytes")(self.handle)) if getattr(self, "handle", None) else 0


def check_frames(*frames):
    """The frames of one forward (a pair, a batch, a window): [H,W,C>=3] fp32 contiguous device tensors of one shape -> (H, W, C)."""
    H, W, Cc = frames[0].shape
    for f in frames:
        assert f.shape == (H, W, Cc) and f.is_cuda and f.dtype == torch.float32 and f.is_contiguous(), "frames: [H,W,C] fp32 contiguous"
    return H, W, Cc


def padded_to(n, d):
    """InputPadder(dims, d) of the reference's models: n rounded up to a multiple of d"""
    return n + (((n // d) + 1) * d - n) % d


def frame_ptrs(frames):
    """frames: a non-empty sequence of frames check_frames accepts -> (host array of their device pointers, (H, W, C))."""
    assert len(frames) > 0
    return (C.c_void_p * len(frames))(*[f.data_ptr() for f in frames]), check_frames(*frames)


class PairBatchEngine(WorkspaceBytes, NetEngine):
    """An engine whose forward takes a batch of frame pairs in one library call (CAIN, Sepconv)."""

    def forward(self, frames0, frames1, out=None):
        """frames0 / frames1: sequences of N [H,W,C>=3] fp32 contiguous device tensors (not written) -> out [N,H,W,3]."""
        n = len(frames0)
        assert n == len(frames1)
        p0, shape = frame_ptrs(frames0)
        p1, shape1 = frame_ptrs(frames1)
        assert shape1 == shape, "frames: [H,W,C] fp32 contiguous"
        H, W, Cc = shape
        if out is None:
            out = torch.empty((n, H, W, 3), dtype=torch.float32, device=self.device)
        self._call("forward", p0, p1, n, Cc, H, W, out.data_ptr(), _lib.stream_ptr())
        return out
