"""AMT VFI node — host-side mirror of the reference's ``AMT_VFI`` (AMT-S / AMT-L, and AMT-G on request) over the HIP library.

Node shape follows vfi_models/amt/__init__.py:11-86; the frame loop is vfi_utils.generic_frame_loop in its timestep mode
(schedule.generic_output_plan + nodeloop.run_plan).  Each pair is ONE vfi_amt_forward with all of the pair's timesteps
(csrc/amt_net.hip): the pad, mean, feature encoder, pyramid encoders and pooled feature maps run once per pair, the decoders, correlation
lookups and update blocks once per timestep.  ``amt-g.pth`` (AMT-G: AMT-L's forward with wider tables and two more update blocks) stays in the
widget list; it is served when config.yaml's ``amt_g`` key is on and raises NotImplementedError naming the checkpoint before anything is
loaded otherwise.  Frames whose padded side is below 128 pixels are refused with a
ValueError: the reference's output is all-NaN there (its coarsest correlation level is one pixel wide).  No pair lanes, no HIP graph.

Frame size: 2^23 - 1 padded pixels for AMT-S / AMT-L; 6 100 805 for AMT-G, and with config.yaml's ``amt_large_frames`` key on 12 201 611, which
takes 2160x3840 (vfi_amt_set_large_frames; the layers' large-image kernel forms).  The key changes nothing for AMT-S / AMT-L.
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
# below 2 GiB (the object holds the same 88 as kCfg[2].px_floats, csrc/amt_net.hip; tests/test_gpu_amt_g.py asserts that the two limits agree)
G_FLOATS_PER_PADDED_PIXEL = 88
MAX_PADDED_PIXELS_G = ((1 << 31) - 1) // (G_FLOATS_PER_PADDED_PIXEL * 4)
# with config.yaml's amt_large_frames on: that buffer below 4 GiB, served by the layer kernels' large-image forms
# (= vfi_amt_large_max_padded_pixels(2): 12 201 611; 2160x3840 = 8 294 400 fits, 2832x4320 does not).  AMT-S / AMT-L keep MAX_PADDED_PIXELS.
LARGE_MAX_PADDED_PIXELS_G = ((1 << 32) - 1) // (G_FLOATS_PER_PADDED_PIXEL * 4)


def large_frames_enabled():
    """config.yaml's ``amt_large_frames`` key (absent = off), read at call time"""
    from . import ckpt

    return bool(ckpt.load_config().get("amt_large_frames", False))


def max_padded_pixels(variant=None, large=None):
    """The limit in force for a variant ("S", "L", "G" or None): AMT-G's follows ``amt_large_frames`` (``large``: the key's state where the
    caller has read it already; None: read now); AMT-S / AMT-L have one limit whatever the key says"""
    if variant != "G":
        return MAX_PADDED_PIXELS
    return LARGE_MAX_PADDED_PIXELS_G if (large_frames_enabled() if large is None else large) else MAX_PADDED_PIXELS_G


def padded_size(H, W):
    """InputPadder(dims, 16) (amt_arch.py:194-200): the sides rounded up to multiples of 16"""
    return padded_to(H, 16), padded_to(W, 16)


def check_frame_size(H, W, variant=None, large=None):
    """The one documented deviation: sizes at which the reference returns NaN everywhere, or beyond the kernels' index arithmetic (AMT-G's
    limit is its own and follows ``amt_large_frames``), are refused before anything is launched (or loaded).  Only an AMT-G frame beyond the
    old limit reads the key."""
    Hp, Wp = padded_size(H, W)
    if min(Hp, Wp) < MIN_PADDED_SIDE:
        raise ValueError(f"AMT VFI: {H}x{W} frames (padded {Hp}x{Wp}) are too small: AMT needs padded sides of at least {MIN_PADDED_SIDE} "
                         "pixels (below, its coarsest correlation level is one pixel wide and the reference's output is all-NaN)")
    if Hp * Wp <= (MAX_PADDED_PIXELS_G if variant == "G" else MAX_PADDED_PIXELS):
        return
    hint = ""
    if variant == "G":
        large = large_frames_enabled() if large is None else large
        if large and Hp * Wp <= LARGE_MAX_PADDED_PIXELS_G:
            return
        if large:
            hint = " (decoder1's 352-channel buffers at half resolution must stay below 4 GiB)"
        elif Hp * Wp <= LARGE_MAX_PADDED_PIXELS_G:      # the key would have helped: name it
            hint = f"; config.yaml's amt_large_frames: true raises it to {LARGE_MAX_PADDED_PIXELS_G}"
        else:
            hint = f" (amt_large_frames would raise it to {LARGE_MAX_PADDED_PIXELS_G} only)"
    limit = max_padded_pixels(variant, large)
    raise ValueError(f"AMT VFI: {H}x{W} frames (padded {Hp}x{Wp}) are beyond the kernels' index arithmetic ({limit} pixels"
                     f"{' for AMT-G' if variant == 'G' else ''}){hint}")


class AmtEngine(WorkspaceBytes, NetEngine):
    """Device-resident AMT-S / AMT-L / AMT-G (the latter only with config.yaml's ``amt_g`` on): ``forward(frame0, frame1, ts)`` = the model's clamped, un-padded frames of one pair at every t of ts."""

    PREFIX, LABEL = "vfi_amt", "AMT"

    def __init__(self, state_dict, device=None):
        self.variant = check_state_dict(state_dict)
        super().__init__(state_dict, device, ("S", "L", "G").index(self.variant))
        if large_frames_enabled():
            self.set_large_frames(True)

    def shapes(self):
        return amt_shapes(self.variant)

    def set_large_frames(self, on):
        """vfi_amt_set_large_frames: the object's switch (AMT-S / AMT-L: the call sets nothing)"""
        self._call("set_large_frames", int(bool(on)))

    def max_padded_pixels(self):
        """The limit the object applies as it stands now: a query, nothing is set"""
        return int(self._fn("object_max_padded_pixels")(self.handle))

    def forward(self, frame0, frame1, ts, out=None):
        """frame0 / frame1: [H,W,C>=3] fp32 contiguous device tensors (not written), ts: timesteps in (0, 1) -> [len(ts),H,W,3]."""
        H, W, Cc = check_frames(frame0, frame1)
        Hp, Wp = padded_size(H, W)
        if self.variant == "G" and Hp * Wp > MAX_PADDED_PIXELS_G:
            # only a frame beyond the 2 GiB limit needs the key: read it now (one config.yaml parse on a frame of hundreds of milliseconds);
            # every smaller frame runs what it always ran, whatever the key and the object's switch say
            large = large_frames_enabled()
            check_frame_size(H, W, self.variant, large)
            self.set_large_frames(large)
        else:
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
