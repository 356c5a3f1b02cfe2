"""Sepconv VFI node — host-side mirror of the reference's ``SepconvVFI`` (SepConv++) over the HIP library.

Node shape follows vfi_models/sepconv/__init__.py:11-56; the frame loop is vfi_utils.generic_frame_loop in its non-timestep mode, the
same loop as CAIN's: per pair, the m-1 new frames come from recursive bisection (schedule.bisect_output_plan), evaluated level by level
(nodeloop.run_plan with cain.eval_pair).  Each model call is one vfi_sepconvnet_forward (csrc/sepconv_net.hip: the whole network plus
the fused output stage).  No clamp.

Frame size, in padded pixels (the sides rounded up to even): 4 194 303, the whole-frame head stage's [Hp, Wp, 256] tensor below 4 GiB
(1080x1920 and everything up to 2 097 151 on the layers' plain forms).  With config.yaml's ``sepconv_large_frames`` key on 8 388 607,
which takes 2160x3840: frames over 2 097 151 pixels run the head stage in horizontal bands (vfi_sepconvnet_set_large_frames;
docs/design/sepconv.md "4K"), smaller ones what they always ran.
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
HEAD1_FLOATS_PER_PIXEL = 256      # the four heads' first layer, [Hp, Wp, 4 * 64]: the whole-frame head stage's widest tensor (csrc/sepconv_net.hip)
UP2_FLOATS_PER_PIXEL = 64         # up2(row1), [Hp, Wp, 64]: the widest tensor the banded head stage keeps whole
WHOLE_FRAME_PIXELS = ((1 << 31) - 2) // (HEAD1_FLOATS_PER_PIXEL * 4)      # 2 097 151: up to here the head stage runs whole-frame, key on or off
MAX_PADDED_PIXELS = ((1 << 32) - 1) // (HEAD1_FLOATS_PER_PIXEL * 4)       # = vfi_sepconvnet_max_pixels(): 4 194 303, that tensor below 4 GiB
# with config.yaml's sepconv_large_frames on: [Hp, Wp, 64] below 2^31 - 1 bytes (= vfi_sepconvnet_large_max_pixels(): 8 388 607; 2160x3840
# and 2160x3842 fit, 2898x2896 does not)
LARGE_MAX_PADDED_PIXELS = ((1 << 31) - 2) // (UP2_FLOATS_PER_PIXEL * 4)
BAND_MAX_WIDTH = WHOLE_FRAME_PIXELS // 16      # 131 071: a band of 8 rows with its halo of 8, [16, Wp, 256], below 2 GiB


def large_frames_enabled():
    """config.yaml's ``sepconv_large_frames`` key (absent = off), read at call time"""
    from . import ckpt

    return bool(ckpt.load_config().get("sepconv_large_frames", False))


def padded_size(H, W):
    """the network's replicate pad: both sides rounded up to even"""
    return H + H % 2, W + W % 2


def max_padded_pixels(large=None):
    """The limit in force: MAX_PADDED_PIXELS, or LARGE_MAX_PADDED_PIXELS with ``sepconv_large_frames`` on (``large``: the key's state where
    the caller has read it already; None: read now)"""
    return LARGE_MAX_PADDED_PIXELS if (large_frames_enabled() if large is None else large) else MAX_PADDED_PIXELS


def check_frame_size(H, W):
    """Raises for a frame the node cannot serve; only a frame beyond the old limit reads the key"""
    Hp, Wp = padded_size(H, W)
    if Hp * Wp <= MAX_PADDED_PIXELS:
        return
    large = large_frames_enabled()
    if Hp * Wp > max_padded_pixels(large):
        if large:
            hint = " (up2(row1), the [Hp, Wp, 64] fp32 tensor, must stay below 2 GiB)"
        elif Hp * Wp <= LARGE_MAX_PADDED_PIXELS:      # the key would have helped: name it
            hint = f"; config.yaml's sepconv_large_frames: true raises it to {LARGE_MAX_PADDED_PIXELS}"
        else:
            hint = f" (sepconv_large_frames would raise it to {LARGE_MAX_PADDED_PIXELS} only)"
        raise ValueError(f"Sepconv VFI: {H}x{W} frames (padded {Hp}x{Wp}) are over the size limit of {max_padded_pixels(large)} padded pixels{hint}")
    if Wp > BAND_MAX_WIDTH and Hp * Wp > WHOLE_FRAME_PIXELS:
        raise ValueError(f"Sepconv VFI: {H}x{W} frames are too wide for the banded head stage: {BAND_MAX_WIDTH} padded columns at the most "
                         "(a band of 8 rows with its halo, [16, Wp, 256] fp32, must stay below 2 GiB)")


class SepconvEngine(PairBatchEngine):
    """Device-resident SepConv++: ``forward(frames0, frames1)`` = ``model(f0, f1)`` for a batch of pairs in one library call."""

    PREFIX, LABEL = "vfi_sepconvnet", "Sepconv"
    shapes = staticmethod(sepconv_shapes)

    def _sync_large_frames(self):
        """The object's limit follows config.yaml's ``sepconv_large_frames`` key as it is now"""
        self._call("set_large_frames", int(large_frames_enabled()))

    def max_padded_pixels(self):
        self._sync_large_frames()
        return int(self._fn("object_max_pixels")(self.handle))

    def forward(self, frames0, frames1, out=None):
        H, W = frames0[0].shape[:2]
        Hp, Wp = padded_size(H, W)
        if Hp * Wp > WHOLE_FRAME_PIXELS:
            # the key chooses the head stage's form from here on (on: bands; off: the whole-frame form on the layers' large-image forms, as
            # ever) and the limit: read it now, one config.yaml parse on a frame of hundreds of milliseconds.  Every smaller frame runs what
            # it always ran, whatever the key and the object's switch say.  The refusal is the object's.
            self._sync_large_frames()
        return super().forward(frames0, frames1, out)


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
        check_frame_size(*frames.shape[1:3])      # before anything is loaded or uploaded
        plan, tasks = bisect_output_plan(len(frames), multiplier, optional_interpolation_states)
        model_path = load_file_from_github_release(MODEL_TYPE, ckpt_name)
        entry = cached_engine(MODEL_TYPE, model_path, lambda: SepconvEngine(load_file(model_path)))
        with engine_call(entry, tuple(frames.shape[1:3])) as engine:
            return (run_plan(engine, frames, plan, tasks, eval_pair, "Sepconv VFI"),)
