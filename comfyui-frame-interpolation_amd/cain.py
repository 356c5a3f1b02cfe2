"""CAIN VFI node — host-side mirror of the reference's ``CAIN_VFI`` over the HIP library.

Node shape follows vfi_models/cain/__init__.py:11-64; the frame loop is vfi_utils.generic_frame_loop in its non-timestep mode
(vfi_utils.py:161-170,202-206): per pair, the m-1 new frames come from recursive bisection, every model call interpolating between
two frames it has already (the pair's frames or earlier model outputs, kept in full precision on the device).  The output order and
the model calls are planned in schedule.bisect_output_plan; here (eval_pair, the pair kind of nodeloop.run_plan) each pair's tree is
evaluated level by level, the calls of a level batched into one vfi_cain_forward (csrc/cain_net.hip: the whole CAIN forward, ~320
launches per call).  No clamp.
"""
import typing

import torch

from .cain_spec import cain_shapes, load_file
from .ckpt import cached_engine, engine_call, load_file_from_github_release
from .netengine import PairBatchEngine
from .nodeloop import run_plan
from .schedule import InterpolationStateList, bisect_output_plan

MODEL_TYPE = "cain"
CKPT_NAMES = ["pretrained_cain.pth"]
MAX_BATCH = 8        # model calls per vfi_cain_forward (about 215 MB of workspace per call at 1080p)


class CainEngine(PairBatchEngine):
    """Device-resident CAIN: ``forward(frames0, frames1)`` = ``model(f0, f1)[0]`` for a batch of pairs in one library call."""

    PREFIX, LABEL = "vfi_cain", "CAIN"
    shapes = staticmethod(cain_shapes)


def eval_pair(engine, f0, f1, task, max_batch=MAX_BATCH):
    """The bisection pair kind of nodeloop.run_plan (CAIN, Sepconv): task = (pair, outputs, calls) of schedule.bisect_output_plan.
    Evaluates the pair's tree, positions 0 and 1 being f0 / f1, and returns the frames at ``outputs`` ([H,W,3] device tensors).  The calls
    of one tree level only read positions of earlier levels, so each level is one batch."""
    _, outputs, calls = task
    have = {0: f0, 1: f1}
    level = {0: 0, 1: 0}
    by_level = {}
    for pos, lo, hi in calls:
        level[pos] = max(level[lo], level[hi]) + 1
        by_level.setdefault(level[pos], []).append((pos, lo, hi))
    for lv in sorted(by_level):
        todo = by_level[lv]
        for s in range(0, len(todo), max_batch):
            part = todo[s:s + max_batch]
            out = engine.forward([have[lo] for _, lo, _ in part], [have[hi] for _, _, hi in part])
            for k, (pos, _, _) in enumerate(part):
                have[pos] = out[k]
    return [have[p] for p in outputs]


class CAIN_VFI:
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

    def vfi(self, ckpt_name: typing.AnyStr, frames: torch.Tensor, clear_cache_after_n_frames: typing.SupportsInt = 1,
            multiplier: typing.SupportsInt = 2, optional_interpolation_states: InterpolationStateList = None, **kwargs):
        # (vfi_utils.assert_batch_size with vfi_name = "CAIN_VFI".replace('_', ' ').replace('VFI', ''), vfi_utils.py:145-147,351)
        assert len(frames) >= 2, (f"VFI model CAIN  requires at least 2 frames to work with, only found {frames.shape[0]}. "
                                  "Please check the frame input using PreviewImage.")
        plan, tasks = bisect_output_plan(len(frames), multiplier, optional_interpolation_states)
        model_path = load_file_from_github_release(MODEL_TYPE, ckpt_name)
        entry = cached_engine(MODEL_TYPE, model_path, lambda: CainEngine(load_file(model_path)))
        with engine_call(entry, tuple(frames.shape[1:3])) as engine:
            return (run_plan(engine, frames, plan, tasks, eval_pair, "CAIN VFI"),)
