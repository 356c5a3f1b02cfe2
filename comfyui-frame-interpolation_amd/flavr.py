"""FLAVR VFI node — host-side mirror of the reference's ``FLAVR_VFI`` over the HIP library.

Node shape follows vfi_models/flavr/__init__.py:28-115.  Unlike every pair-at-a-time node, FLAVR reads a window of four frames
(i .. i + 3) and writes one new frame between frames i + 1 and i + 2; the reference's private loop is restated by ``window_plan``
(quirks included) and run by ``run_windows``: a sliding window of four device frames, each frame uploaded once.  Each model call is
one vfi_flavr_forward (csrc/flavr_net.hip: InputPadder(16), window mean, 3D U-Net, un-pad).  No clamp; the multiplier is always 2.
No pair lanes, no multi-rank sharding and no HIP graph for this node.

Frame size: 2 097 151 padded pixels (1080x1920 pads to 1088x1920 and fits); with config.yaml's ``flavr_large_frames`` key on 8 388 607, which
takes 2160x3840 (vfi_flavr_set_large_frames; the layers' large-image kernel forms, ~52 GB of workspace).
"""
import typing
import warnings

import torch

from . import _lib
from .ckpt import cached_engine, engine_call, load_file_from_github_release
from .flavr_spec import flavr_shapes, load_file, n_outputs_of
from .netengine import NetEngine, WorkspaceBytes, frame_ptrs
from .schedule import InterpolationStateList

MODEL_TYPE = "flavr"
CKPT_NAMES = ["FLAVR_2x.pth", "FLAVR_4x.pth", "FLAVR_8x.pth"]
NBR_FRAME = 4
FLOATS_PER_PADDED_PIXEL = 256     # the widest tensor: the last up-convolution's [Hp, Wp, 4 * 64] output (csrc/flavr_net.hip)
MAX_PADDED_PIXELS = ((1 << 31) - 2) // (FLOATS_PER_PADDED_PIXEL * 4)      # = vfi_flavr_max_padded_pixels(): 2 097 151, that tensor below 2^31 - 1 bytes
# with config.yaml's flavr_large_frames on: that tensor within the layer kernels' 2^31 - 1 floats per image
# (= vfi_flavr_large_max_padded_pixels(): 8 388 607; 2160x3840 fits, 2176x3856 does not)
LARGE_MAX_PADDED_PIXELS = ((1 << 31) - 1) // FLOATS_PER_PADDED_PIXEL


def large_frames_enabled():
    """config.yaml's ``flavr_large_frames`` key (absent = off), read at call time"""
    from . import ckpt

    return bool(ckpt.load_config().get("flavr_large_frames", False))


def padded_size(H, W):
    """InputPadder(16): the sides rounded up to multiples of 16"""
    return (H + 15) // 16 * 16, (W + 15) // 16 * 16


def max_padded_pixels(large=None):
    """The limit in force: MAX_PADDED_PIXELS, or LARGE_MAX_PADDED_PIXELS with ``flavr_large_frames`` on (``large``: the key's state where
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
            hint = " (the last up-convolution's [Hp, Wp, 256] tensor must stay within 2^31 - 1 floats)"
        elif Hp * Wp <= LARGE_MAX_PADDED_PIXELS:      # the key would have helped: name it
            hint = f"; config.yaml's flavr_large_frames: true raises it to {LARGE_MAX_PADDED_PIXELS}"
        else:
            hint = f" (flavr_large_frames would raise it to {LARGE_MAX_PADDED_PIXELS} only)"
        raise ValueError(f"FLAVR VFI: {H}x{W} frames (padded {Hp}x{Wp}) are over the size limit of {max_padded_pixels(large)} padded pixels{hint}")


class FlavrEngine(WorkspaceBytes, NetEngine):
    """Device-resident FLAVR: ``forward(frames)`` = ``unpad(model([pad(f) for f in window])[0])`` for a batch of windows in one call."""

    PREFIX, LABEL = "vfi_flavr", "FLAVR"

    def __init__(self, state_dict, device=None):
        self.n_outputs = n_outputs_of(state_dict)
        super().__init__(state_dict, device, self.n_outputs)

    def shapes(self):
        return flavr_shapes(self.n_outputs)

    def _sync_large_frames(self):
        """The object's limit follows config.yaml's ``flavr_large_frames`` key as it is now"""
        self._call("set_large_frames", int(large_frames_enabled()))

    def max_padded_pixels(self):
        self._sync_large_frames()
        return int(self._fn("object_max_padded_pixels")(self.handle))

    def forward(self, frames, out=None):
        """frames: a sequence of 4 N [H,W,C>=3] fp32 contiguous device tensors (window n = frames[4n : 4n+4]; not written) -> [N,H,W,3]."""
        assert len(frames) > 0 and len(frames) % NBR_FRAME == 0, "frames: four per window"
        n = len(frames) // NBR_FRAME
        p, (H, W, Cc) = frame_ptrs(frames)
        Hp, Wp = padded_size(H, W)
        if Hp * Wp > MAX_PADDED_PIXELS:
            # only a frame beyond the old limit needs the key: read it now (one config.yaml parse on a frame of hundreds of milliseconds);
            # every smaller frame runs what it always ran, whatever the key and the object's switch say.  The refusal is the object's.
            self._sync_large_frames()
        if out is None:
            out = torch.empty((n, H, W, 3), dtype=torch.float32, device=self.device)
        self._call("forward", p, n, Cc, H, W, out.data_ptr(), _lib.stream_ptr())
        return out


def window_plan(n_frames, duplicate_first_last_frames=False, states: InterpolationStateList = None):
    """The reference loop's output (vfi_models/flavr/__init__.py:72-97) as ``("src", frame)`` / ``("new", window)`` entries in order.
    Window i (frames i .. i + 3) is skipped only when frames i AND i + 1 are skipped.  The leading frames 0, 1 are emitted by window 0
    and the trailing frame by the last window, so skipping those windows drops them too — as the reference does."""
    plan = []
    for i in range(n_frames - 3):
        if states is not None and states.is_frame_skipped(i) and states.is_frame_skipped(i + 1):
            continue
        if i == 0:
            plan.append(("src", 0))
            if duplicate_first_last_frames:
                plan.append(("src", 0))
            plan.append(("src", 1))
        plan += [("new", i), ("src", i + 2)]
        if i == n_frames - 4:
            plan.append(("src", i + 3))
            if duplicate_first_last_frames:
                plan.append(("src", i + 3))
    return plan


def run_windows(engine, frames, plan):
    """frames [N,H,W,C] host tensor, plan of window_plan -> [len(plan),H,W,3] fp32 host tensor.  A frame goes to the device when the first
    window that reads it runs and is dropped after the last one."""
    if not plan:      # (the reference fails in torch.cat of an empty list)
        raise RuntimeError("FLAVR VFI: every window was skipped - nothing to output")
    frames = frames[..., :3]
    H, W = frames.shape[1:3]
    out = torch.empty((len(plan), H, W, 3), dtype=torch.float32)
    dev = engine.device
    held = {}
    for row, (kind, idx) in enumerate(plan):
        if kind == "src":
            out[row] = frames[idx]
            continue
        for f in [f for f in held if f < idx]:
            del held[f]
        for f in range(idx, idx + NBR_FRAME):
            if f not in held:
                held[f] = frames[f].to(dev, torch.float32).contiguous()
        out[row] = engine.forward([held[f] for f in range(idx, idx + NBR_FRAME)])[0].cpu()
    return out


class FLAVR_VFI:
    @classmethod
    def INPUT_TYPES(s):
        return {
            "required": {
                "ckpt_name": (CKPT_NAMES,),
                "frames": ("IMAGE",),
                "clear_cache_after_n_frames": ("INT", {"default": 10, "min": 1, "max": 1000}),
                "multiplier": ("INT", {"default": 2, "min": 2, "max": 2}),
                "duplicate_first_last_frames": ("BOOLEAN", {"default": False}),
            },
            "optional": {"optional_interpolation_states": ("INTERPOLATION_STATES",)},
        }

    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "vfi"
    CATEGORY = "ComfyUI-Frame-Interpolation/VFI"

    def vfi(self, ckpt_name: typing.AnyStr, frames: torch.Tensor, clear_cache_after_n_frames=10, multiplier: typing.SupportsInt = 2,
            duplicate_first_last_frames: bool = False, optional_interpolation_states: InterpolationStateList = None, **kwargs):
        if multiplier != 2:
            warnings.warn("Currently, FLAVR only supports 2x interpolation. The process will continue but please set multiplier=2 afterward")
        # (vfi_utils.assert_batch_size(frames, batch_size=4, vfi_name="ST-MFNet"): the reference names the wrong model here, kept)
        assert len(frames) >= NBR_FRAME, (f"VFI model ST-MFNet requires at least 4 frames to work with, only found {frames.shape[0]}. "
                                          "Please check the frame input using PreviewImage.")
        check_frame_size(*frames.shape[1:3])      # before anything is loaded or uploaded
        plan = window_plan(len(frames), duplicate_first_last_frames, optional_interpolation_states)
        model_path = load_file_from_github_release(MODEL_TYPE, ckpt_name)
        entry = cached_engine(MODEL_TYPE, model_path, lambda: FlavrEngine(load_file(model_path)))
        with engine_call(entry, tuple(frames.shape[1:3])) as engine:
            return (run_windows(engine, frames, plan),)
