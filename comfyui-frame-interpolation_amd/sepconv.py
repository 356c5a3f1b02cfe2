"""Sepconv VFI node — host-side mirror of the reference's ``SepconvVFI`` (SepConv++) over the HIP library.

Node shape follows vfi_models/sepconv/__init__.py:11-56; the frame loop is vfi_utils.generic_frame_loop in its non-timestep mode, the
same loop as CAIN's: per pair, the m-1 new frames come from recursive bisection (schedule.bisect_output_plan), evaluated level by level
(nodeloop.run_plan with cain.eval_pair).  Each model call is one vfi_sepconvnet_forward (csrc/sepconv_net.hip: the whole network plus
the fused output stage).  No clamp.
"""
import ctypes as C
import typing

import torch

from . import _lib
from .cain import eval_pair
from .ckpt import cached_engine, engine_call, load_file_from_github_release
from .nodeloop import run_plan
from .schedule import InterpolationStateList, bisect_output_plan
from .sepconv_spec import load_file, sepconv_shapes

MODEL_TYPE = "sepconv"
CKPT_NAMES = ["sepconv.pth"]


class SepconvEngine:
    """Device-resident SepConv++: ``forward(frames0, frames1)`` = ``model(f0, f1)`` for a batch of pairs in one library call."""

    def __init__(self, state_dict, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("Sepconv VFI (HIP): no GPU visible; this node has no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        _lib.check(self.lib.vfi_init(self.device.index or 0), "vfi_init")
        keys = list(sepconv_shapes().keys())
        tensors = [state_dict[k].detach().to("cpu", torch.float32).contiguous() for k in keys]
        ptrs = (C.c_void_p * len(keys))(*[t.data_ptr() for t in tensors])
        numels = (C.c_int64 * len(keys))(*[t.numel() for t in tensors])
        self.handle = self.lib.vfi_sepconvnet_create(ptrs, numels, len(keys))
        if not self.handle:
            raise RuntimeError("vfi_sepconvnet_create failed: " + _lib.last_error())

    def close(self):
        if getattr(self, "handle", None):
            self.lib.vfi_sepconvnet_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def release_workspace(self):
        _lib.check(self.lib.vfi_sepconvnet_release_workspace(self.handle), "vfi_sepconvnet_release_workspace")

    def workspace_bytes(self):
        return int(self.lib.vfi_sepconvnet_workspace_bytes(self.handle)) if getattr(self, "handle", None) else 0

    def forward(self, frames0, frames1, out=None):
        """frames0 / frames1: sequences of N [H,W,C>=3] fp32 contiguous device tensors (not written) -> out [N,H,W,3]."""
        n = len(frames0)
        assert n == len(frames1) and n > 0
        H, W, Cc = frames0[0].shape
        for f in list(frames0) + list(frames1):
            assert f.shape == (H, W, Cc) and f.is_cuda and f.dtype == torch.float32 and f.is_contiguous(), "frames: [H,W,C] fp32 contiguous"
        if out is None:
            out = torch.empty((n, H, W, 3), dtype=torch.float32, device=self.device)
        p0 = (C.c_void_p * n)(*[f.data_ptr() for f in frames0])
        p1 = (C.c_void_p * n)(*[f.data_ptr() for f in frames1])
        _lib.check(self.lib.vfi_sepconvnet_forward(self.handle, p0, p1, n, Cc, H, W, out.data_ptr(), _lib.stream_ptr()), "vfi_sepconvnet_forward")
        return out


class SepconvVFI:
    @classmethod
    def INPUT_TYPES(s):
        return {
            "required": {
                "ckpt_name": (CKPT_NAMES,),
                "frames": ("IMAGE",),
                "clear_cache_after_n_frames": ("INT", {"default": 10, "min": 1, "max": 1000}),
                "multiplier": ("INT", {"default": 2, "min": 2, "max": 1000}),
            },
            "optional": {"optional_interpolation_states": ("INTERPOLATION_STATES",)},
        }

    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "vfi"
    CATEGORY = "ComfyUI-Frame-Interpolation/VFI"

    def vfi(self, ckpt_name: typing.AnyStr, frames: torch.Tensor, clear_cache_after_n_frames=10, multiplier: typing.SupportsInt = 2,
            optional_interpolation_states: InterpolationStateList = None, **kwargs):
        # (vfi_utils.assert_batch_size with vfi_name = "SepconvVFI".replace('_', ' ').replace('VFI', ''), vfi_utils.py:145-147,351)
        assert len(frames) >= 2, (f"VFI model Sepconv requires at least 2 frames to work with, only found {frames.shape[0]}. "
                                  "Please check the frame input using PreviewImage.")
        plan, tasks = bisect_output_plan(len(frames), multiplier, optional_interpolation_states)
        model_path = load_file_from_github_release(MODEL_TYPE, ckpt_name)
        entry = cached_engine(MODEL_TYPE, model_path, lambda: SepconvEngine(load_file(model_path)))
        with engine_call(entry, tuple(frames.shape[1:3])) as engine:
            return (run_plan(engine, frames, plan, tasks, eval_pair, "Sepconv VFI"),)
