"""XVFI node — host-side mirror of the reference's ``XVFI`` class over the HIP library.

Node shape follows vfi_models/xvfi/__init__.py:50-114: the two checkpoint names, ``batch_size`` (accepted; results do not depend on it),
``multipler`` (the reference's spelling) and ``optional_interpolation_states``.  The reference zero-pads the clip at the bottom / right to a
multiple of 2^S_tst * module_scale_factor * 4 (16 for Vimeo, 512 for X4K), calls the model once per kept pair and timestep k / multipler, and
crops; here each model call is ONE vfi_xvfi_forward (csrc/xvfi_net.hip: pad, all levels, crop), and the object keeps the features and level
flows of a pair while the timestep varies.  Frames are not clamped, as in the reference.

Two deviations from the reference, both where the reference misbehaves:
  1. Output frames are in numeric order; the reference sorts the string keys '0', '0.1', ..., which is the same order for at most 10 input
     frames and ``multipler`` <= 10 and scrambles the clip beyond that.
  2. An ``InterpolationStateList`` is honoured through ``is_frame_skipped``; the reference enumerates it and raises TypeError.  A list of
     booleans (True = interpolate the pair) behaves as in the reference.
"""
import typing

import torch

from . import _lib
from .ckpt import cached_engine, engine_call, load_file_from_github_release
from .netengine import NetEngine, WorkspaceBytes, check_frames
from .nodeloop import run_plan
from .schedule import InterpolationStateList, generic_output_plan
from .xvfi_spec import CKPT_CONFIGS, check_state_dict, config_of, load_file, padded_size, xvfi_shapes

MODEL_TYPE = "xvfi"
FLOATS_PER_PADDED_PIXEL = 80      # the widest per-image buffer: the RefineUNet's input at scale 2, 64 shuffled channels + 16 (csrc/xvfi_net.hip)
MAX_PADDED_PIXELS = ((1 << 31) - 1) // (FLOATS_PER_PADDED_PIXEL * 4)      # = vfi_xvfi_max_padded_pixels(): 6 710 886
# with config.yaml's xvfi_large_frames on: one image below 4 GiB, served by the layer kernels' large-image forms
# (= vfi_xvfi_large_max_padded_pixels(): 13 421 772; 2160x3840 fits both configurations, padded 2160x3840 / 2560x4096)
LARGE_MAX_PADDED_PIXELS = ((1 << 32) - 1) // (FLOATS_PER_PADDED_PIXEL * 4)


def large_frames_enabled():
    """config.yaml's ``xvfi_large_frames`` key (absent = off), read at call time"""
    from . import ckpt

    return bool(ckpt.load_config().get("xvfi_large_frames", False))


def max_padded_pixels():
    """The limit in force: MAX_PADDED_PIXELS, or LARGE_MAX_PADDED_PIXELS with ``xvfi_large_frames`` on"""
    return LARGE_MAX_PADDED_PIXELS if large_frames_enabled() else MAX_PADDED_PIXELS


def check_frame_size(H, W, config):
    Hp, Wp = padded_size(H, W, config)
    limit = max_padded_pixels()
    if Hp * Wp > limit:
        raise ValueError(f"XVFI VFI: {H}x{W} frames (padded {Hp}x{Wp}) are beyond the kernels' index arithmetic ({limit} padded pixels)")


class XvfiEngine(WorkspaceBytes, NetEngine):
    """Device-resident XVFInet for one configuration (a checkpoint name or (module_scale_factor, S_tst)): ``forward(frame0, frame1, t)`` =
    the model's un-padded, un-clamped frame at time t of one pair."""

    PREFIX, LABEL = "vfi_xvfi", "XVFI"

    def __init__(self, state_dict, config, device=None):
        self.config = config_of(config)
        super().__init__(state_dict, device, *self.config)

    def shapes(self):
        return xvfi_shapes(self.config[0])

    def check_state_dict(self, state_dict):
        check_state_dict(state_dict, self.config[0])

    def _sync_large_frames(self):
        """The object's limit follows config.yaml's ``xvfi_large_frames`` key as it is now"""
        self._call("set_large_frames", int(large_frames_enabled()))

    def max_padded_pixels(self):
        self._sync_large_frames()
        return int(self.lib.vfi_xvfi_object_max_padded_pixels(self.handle))

    def forward(self, frame0, frame1, t, out=None):
        """frame0 / frame1: [H,W,C>=3] fp32 contiguous device tensors (not written) -> [H,W,3]."""
        H, W, Cc = check_frames(frame0, frame1)
        check_frame_size(H, W, self.config)
        self._sync_large_frames()
        if out is None:
            out = torch.empty((H, W, 3), dtype=torch.float32, device=self.device)
        self._call("forward", frame0.data_ptr(), frame1.data_ptr(), Cc, H, W, float(t), out.data_ptr(), _lib.stream_ptr())
        return out

    def level0_flow(self, H, W):
        """flow_l_tmp of level 0 for the pair of the last forward: [Hp / scale, Wp / scale, 6] device tensor"""
        Hp, Wp = padded_size(H, W, self.config)
        s = self.config[0]
        out = torch.empty((Hp // s, Wp // s, 6), dtype=torch.float32, device=self.device)
        self._call("level0_flow", out.data_ptr(), _lib.stream_ptr())
        return out


class _BoolStates:
    """The reference's plain list of booleans (True = interpolate pair i; pairs beyond the list are left alone) as a skip oracle"""

    def __init__(self, states, n_pairs):
        self.states = [bool(s) for s in states]
        over = [i for i, s in enumerate(self.states) if s and i >= n_pairs]
        if over:
            raise IndexError(f"optional_interpolation_states enables pair {over[0]} of a clip with {n_pairs} pairs")

    def is_frame_skipped(self, i):
        return i >= len(self.states) or not self.states[i]


def interpolation_states(states, n_pairs):
    if states is None or isinstance(states, InterpolationStateList) or hasattr(states, "is_frame_skipped"):
        return states
    return _BoolStates(states, n_pairs)


def xvfi_pair(eng, f0, f1, task):
    """One pair of the plan: task = (pair, [timesteps]); every timestep is one forward on the same pair, whose features the object keeps."""
    for t in task[1]:
        yield eng.forward(f0, f1, t)


class XVFI:
    @classmethod
    def INPUT_TYPES(s):
        return {
            "required": {
                "ckpt_name": (list(CKPT_CONFIGS.keys()),),
                "frames": ("IMAGE",),
                "batch_size": ("INT", {"default": 1, "min": 1, "max": 100}),
                "multipler": ("INT", {"default": 2, "min": 2, "max": 1000}),
            },
            "optional": {"optional_interpolation_states": ("INTERPOLATION_STATES",)},
        }

    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "vfi"
    CATEGORY = "ComfyUI-Frame-Interpolation/VFI"

    def vfi(self, ckpt_name: typing.AnyStr, frames: torch.Tensor, batch_size: typing.SupportsInt = 1, multipler: typing.SupportsInt = 2,
            optional_interpolation_states: InterpolationStateList = None, **kwargs):
        config = config_of(ckpt_name)
        check_frame_size(*frames.shape[1:3], config)      # before an engine exists
        states = interpolation_states(optional_interpolation_states, len(frames) - 1)
        plan, tasks = generic_output_plan(len(frames), int(multipler), states)
        model_path = load_file_from_github_release(MODEL_TYPE, ckpt_name)
        entry = cached_engine(MODEL_TYPE, model_path, lambda: XvfiEngine(load_file(model_path, ckpt_name), config))
        with engine_call(entry, tuple(frames.shape[1:3])) as engine:
            return (run_plan(engine, frames, plan, tasks, xvfi_pair, "XVFI VFI"),)
