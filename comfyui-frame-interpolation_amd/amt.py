"""AMT VFI node — host-side mirror of the reference's ``AMT_VFI`` (AMT-S / AMT-L, and AMT-G on request) over the HIP library.

Node shape follows vfi_models/amt/__init__.py:11-86; the frame loop is vfi_utils.generic_frame_loop in its timestep mode
(schedule.generic_output_plan + nodeloop.run_plan).  Each pair is ONE vfi_amt_forward with all of the pair's timesteps
(csrc/amt_net.hip): the pad, mean, feature encoder, pyramid encoders and pooled feature maps run once per pair, the decoders, correlation
lookups and update blocks once per timestep.  ``amt-g.pth`` (AMT-G: AMT-L's forward with wider tables and two more update blocks) stays in the
widget list; it is served when config.yaml's ``amt_g`` key is on and raises NotImplementedError naming the checkpoint before anything is
loaded otherwise.  Frames whose padded side is below 128 pixels are refused with a
ValueError: the reference's output is all-NaN there (its coarsest correlation level is one pixel wide).  No pair lanes, no HIP graph.
"""
import ctypes as C
import typing

import torch

from . import _lib
from .amt_spec import CKPT_VARIANT, amt_shapes, check_state_dict, load_file, variant_of_ckpt
from .ckpt import cached_engine, engine_call, load_file_from_direct_url
from .netengine import NetEngine, WorkspaceBytes, check_frames, padded_to
from .nodeloop import run_plan
from .schedule import InterpolationStateList, generic_output_plan

MODEL_TYPE = "amt"
CKPT_NAMES = list(CKPT_VARIANT)
CKPT_URL = "https://huggingface.co/lalala125/AMT/resolve/main/{ckpt_name}"
MIN_PADDED_SIDE = 128
MAX_PADDED_PIXELS = (1 << 23) - 1      # the layers' 2 GiB index limit on a [Hp, Wp, 64] fp32 tensor (csrc/amt_net.hip)
# AMT-G's widest activation (decoder1's ResBlock at half resolution, 352 channels) has 88 floats per padded pixel: 2160x3840 does not fit
# (the object holds the same 88 as kCfg[2].px_floats, csrc/amt_net.hip; tests/test_gpu_amt_g.py asserts that the two limits agree)
G_FLOATS_PER_PADDED_PIXEL = 88
MAX_PADDED_PIXELS_G = ((1 << 31) - 1) // (G_FLOATS_PER_PADDED_PIXEL * 4)


def padded_size(H, W):
    """InputPadder(dims, 16) (amt_arch.py:194-200): the sides rounded up to multiples of 16"""
    return padded_to(H, 16), padded_to(W, 16)


def check_frame_size(H, W, variant=None):
    """The one documented deviation: sizes at which the reference returns NaN everywhere, or beyond the kernels' index arithmetic (AMT-G's
    limit is its own), are refused before anything is launched (or loaded)."""
    Hp, Wp = padded_size(H, W)
    if min(Hp, Wp) < MIN_PADDED_SIDE:
        raise ValueError(f"AMT VFI: {H}x{W} frames (padded {Hp}x{Wp}) are too small: AMT needs padded sides of at least {MIN_PADDED_SIDE} "
                         "pixels (below, its coarsest correlation level is one pixel wide and the reference's output is all-NaN)")
    limit = MAX_PADDED_PIXELS_G if variant == "G" else MAX_PADDED_PIXELS
    if Hp * Wp > limit:
        raise ValueError(f"AMT VFI: {H}x{W} frames (padded {Hp}x{Wp}) are beyond the kernels' index arithmetic ({limit} pixels"
                         f"{' for AMT-G' if variant == 'G' else ''})")


class AmtEngine(WorkspaceBytes, NetEngine):
    """Device-resident AMT-S / AMT-L / AMT-G (the latter only with config.yaml's ``amt_g`` on): ``forward(frame0, frame1, ts)`` = the model's clamped, un-padded frames of one pair at every t of ts."""

    PREFIX, LABEL = "vfi_amt", "AMT"

    def __init__(self, state_dict, device=None):
        self.variant = check_state_dict(state_dict)
        super().__init__(state_dict, device, ("S", "L", "G").index(self.variant))

    def shapes(self):
        return amt_shapes(self.variant)

    def forward(self, frame0, frame1, ts, out=None):
        """frame0 / frame1: [H,W,C>=3] fp32 contiguous device tensors (not written), ts: timesteps in (0, 1) -> [len(ts),H,W,3]."""
        H, W, Cc = check_frames(frame0, frame1)
        check_frame_size(H, W, self.variant)
        ts = [float(t) for t in ts]
        assert ts, "ts: at least one timestep"
        if out is None:
            out = torch.empty((len(ts), H, W, 3), dtype=torch.float32, device=self.device)
        self._call("forward", frame0.data_ptr(), frame1.data_ptr(), Cc, H, W, (C.c_float * len(ts))(*ts), len(ts), out.data_ptr(), _lib.stream_ptr())
        return out


def pair_frames(engine, f0, f1, task):
    """One pair of the plan: a single forward with all of the pair's timesteps."""
    return list(engine.forward(f0, f1, task[1]))


class AMT_VFI:
    @classmethod
    def INPUT_TYPES(s):
        return {
            "required": {
                "ckpt_name": (CKPT_NAMES,),
                "frames": ("IMAGE",),
                "clear_cache_after_n_frames": ("INT", {"default": 1, "min": 1, "max": 100}),
                "multiplier": ("INT", {"default": 2, "min": 2, "max": 1000}),
            },
            "optional": {"optional_interpolation_states": ("INTERPOLATION_STATES",)},
        }

    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "vfi"
    CATEGORY = "ComfyUI-Frame-Interpolation/VFI"

    def vfi(self, ckpt_name: typing.AnyStr, frames: torch.Tensor, clear_cache_after_n_frames: typing.SupportsInt = 1,
            multiplier: typing.SupportsInt = 2, optional_interpolation_states: InterpolationStateList = None, **kwargs):
        variant = variant_of_ckpt(ckpt_name)            # amt-g.pth without the amt_g key: NotImplementedError before anything is loaded
        check_frame_size(*frames.shape[1:3], variant)   # before an engine exists
        plan, tasks = generic_output_plan(len(frames), multiplier, optional_interpolation_states)
        model_path = load_file_from_direct_url(MODEL_TYPE, CKPT_URL.format(ckpt_name=ckpt_name))
        entry = cached_engine(MODEL_TYPE, model_path, lambda: self.make_engine(model_path, ckpt_name))
        with engine_call(entry, tuple(frames.shape[1:3])) as engine:
            return (run_plan(engine, frames, plan, tasks, pair_frames, "AMT VFI"),)

    @staticmethod
    def make_engine(model_path, ckpt_name):
        return AmtEngine(load_file(model_path, ckpt_name)[0])
