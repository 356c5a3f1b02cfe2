"""Sepconv VFI node — host-side mirror of the reference's ``SepconvVFI`` (SepConv++) over the HIP library.

Node shape follows vfi_models/sepconv/__init__.py:11-56; the frame loop is vfi_utils.generic_frame_loop in its non-timestep mode, the
same loop as CAIN's: per pair, the m-1 new frames come from recursive bisection (schedule.bisect_output_plan), evaluated level by level
(nodeloop.run_plan with cain.eval_pair).  Each model call is one vfi_sepconvnet_forward (csrc/sepconv_net.hip: the whole network plus
the fused output stage).  No clamp.
"""
import typing

import torch

from .cain import eval_pair
from .ckpt import cached_engine, engine_call, load_file_from_github_release
from .netengine import PairBatchEngine
from .nodeloop import run_plan
from .schedule import InterpolationStateList, bisect_output_plan
from .sepconv_spec import load_file, sepconv_shapes

MODEL_TYPE = "sepconv"
CKPT_NAMES = ["sepconv.pth"]


class SepconvEngine(PairBatchEngine):
    """Device-resident SepConv++: ``forward(frames0, frames1)`` = ``model(f0, f1)`` for a batch of pairs in one library call."""

    PREFIX, LABEL = "vfi_sepconvnet", "Sepconv"
    shapes = staticmethod(sepconv_shapes)


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
