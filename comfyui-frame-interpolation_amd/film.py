"""FILM VFI node — host-side mirror of the reference's ``FILM_VFI`` over the HIP library.

Same node shape and scheduling as vfi_models/film/__init__.py:12-113 (greedy bisection per pair, skipped pairs are
dropped, outputs re-used as inputs after ``clamp(0,1)``); the interpolator itself (vfi_models/film/film_arch.py
``Interpolator.debug_forward``, the source mirror of the TorchScript artifact the reference loads) is executed
by the C-side object vfi_film_* (csrc/film_net.hip) as a sequence of the library's generic ops: every torch.nn.functional call
of the reference maps to one entry point

    F.conv2d(padding='same') (+LeakyReLU)  -> vfi_conv_forward     (fp32 MFMA implicit GEMM)
    F.avg_pool2d(2,2)                       -> vfi_avgpool2
    F.grid_sample via film_arch.warp        -> vfi_warp_film
    F.interpolate(bilinear / nearest)       -> vfi_resize_bilinear / vfi_upsample_nearest
    +, *scalar                              -> vfi_axpby

and every ``torch.cat`` along channels disappears: producers write into channel windows of pre-allocated NHWC
tensors (physical channel positions are translated once, at weight-pack time, through ``chan_map``).
torch only allocates device buffers and moves frames (plumbing).
"""
import bisect
import typing

import numpy as np
import torch

from . import _lib
from .ckpt import cached_engine, engine_call, load_file_from_github_release
from .film_spec import check_state_dict, film_shapes
from .lanes import LaneSet, lane_set, lanes_for
from .netengine import NetEngine
from .nodeloop import run_plan
from .schedule import InterpolationStateList, film_output_plan

MODEL_TYPE = "film"
# Frames of up to this many pixels run the launches they ran before the layers' large forms existed: (2^32 - 1) // (208 * 4), the
# widest tensor at one image below 4 GiB.  Above it the node opens ONE pair lane whatever lanes.DEFAULT_LANES says: a 4K workspace is
# 69 GB, and two of them beside the staging rings have not been measured.
LANE_PIXELS = 5162220


def max_pixels():
    """The largest frame the C object takes, H * W (vfi_film_max_pixels: read from the library, not repeated here)"""
    return int(_lib.load().vfi_film_max_pixels())


def check_frame_size(H, W):
    """Before a clip is uploaded or an engine built: the wording of vfi_film_forward's own guard"""
    limit = max_pixels()
    if H * W > limit:
        raise ValueError(f"FILM VFI: a {H}x{W} frame is over the size limit of FILM, {limit} pixels: the aligned pyramid's level 0 "
                         f"(208 floats per pixel) must stay within the layers' 2147483647 floats per image")


def lanes_for_frame(H, W):
    """Pair lanes of a call on H x W frames"""
    return lanes_for(MODEL_TYPE) if H * W <= LANE_PIXELS else 1


def film_lane_set(build):
    """The node's LaneSet, built with the lanes of the model type as before"""
    ls = lane_set(MODEL_TYPE, build)
    ls.k_built = ls.k
    return ls


def limit_lanes(engine, H, W):
    """The lanes one call on H x W frames may open: never more than the set was built with (its streams), one above LANE_PIXELS.  Lanes beyond
    the first are built at first use, so a 4K call never pays for a second engine."""
    if isinstance(engine, LaneSet):
        engine.k = min(getattr(engine, "k_built", engine.k), lanes_for_frame(H, W))


class FilmEngine(NetEngine):
    """Device-resident FILM interpolator (one frame pair per call, like the reference node): the C-side object
    vfi_film_create / vfi_film_forward / vfi_film_destroy (csrc/film_net.hip) — weights packed once, workspace owned by the
    library, the whole launch sequence of a pair issued by one call."""

    PREFIX, LABEL = "vfi_film", "FILM"
    shapes = staticmethod(film_shapes)
    check_state_dict = staticmethod(check_state_dict)
    # no workspace_bytes: the object does not report it, so ckpt.end_call releases the workspace (15 GB at 1080p) after every call

    def two_streams(self, on):
        """vfi_film_forward forks half of the network onto the object's side stream (default) / stays on the caller's stream (what the
        node wants once several pairs are in flight on lanes of their own).  Bit-identical frames either way."""
        return bool(self.lib.vfi_film_two_streams(self.handle, int(bool(on))))

    lone_pair = two_streams      # lanes.tell_lone_pair

    def debug_flow(self, d, level, h, w):
        """test tap: flow pyramid level of the last forward, direction d (0 forward, 1 backward) -> [h,w,2] host tensor"""
        buf = torch.empty(h * w * 2, dtype=torch.float32)
        n = _lib.test_tap("vfi_film_debug_read_flow")(self.handle, d, level, buf.data_ptr(), buf.numel())
        if n != buf.numel():
            raise RuntimeError("vfi_film_debug_read_flow: " + _lib.last_error())
        return buf.view(h, w, 2)

    def workspace_now(self):
        """Device bytes of the workspace as it stands (tools, documentation).  Deliberately not called workspace_bytes: ckpt.end_call would
        take that name as leave to keep 15-69 GB resident between calls."""
        return int(self.lib.vfi_film_workspace_bytes(self.handle)) if getattr(self, "handle", None) else 0

    def forward(self, x0, x1, clamp=False):
        """x0, x1: [H,W,C>=3] fp32 device tensors -> [H,W,3] device tensor (Interpolator.forward, time = 0.5)."""
        H, W = x0.shape[:2]
        for x in (x0, x1):
            assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape[:2]) == (H, W) and x.shape[2] == x0.shape[2]
        out = torch.empty((H, W, 3), dtype=torch.float32, device=self.device)
        self._call("forward", x0.data_ptr(), x1.data_ptr(), x0.shape[2], H, W, out.data_ptr(), int(bool(clamp)), _lib.stream_ptr())
        return out


def film_schedule(inter_frames):
    """Greedy bisection order of one pair (vfi_models/film/__init__.py:17-40): list of (left, right, new) grid
    positions; the model is always asked for the midpoint (it ignores dt, film_arch.py:427-429)."""
    idxes = [0, inter_frames + 1]
    remains = list(range(1, inter_frames + 1))
    splits = torch.linspace(0, 1, inter_frames + 2)
    calls = []
    for _ in range(len(remains)):
        starts = splits[idxes[:-1]]
        ends = splits[idxes[1:]]
        distances = ((splits[None, remains] - starts[:, None]) / (ends[:, None] - starts[:, None]) - .5).abs()
        start_i, step = np.unravel_index(torch.argmin(distances).item(), distances.shape)
        new = remains[step]
        calls.append((idxes[start_i], idxes[start_i + 1], new))
        idxes.insert(bisect.bisect_left(idxes, new), new)
        del remains[step]
    return calls


def film_pair(eng, f0, f1, task):
    """FILM's pair kind of nodeloop.run_plan: task = (pair, positions) of schedule.film_output_plan.  The greedy bisection runs
    sequentially on the current stream, every output clamped to [0, 1] and re-used as an input."""
    new = task[1]
    res = {0: f0, len(new) + 1: f1}
    for l, r, k in film_schedule(len(new)):
        res[k] = eng.forward(res[l], res[r], clamp=True)
    return [res[k] for k in new]


def _load_state_dict(path):
    try:
        return torch.jit.load(path, map_location="cpu").state_dict()   # the reference's artifact (film/__init__.py:74)
    except Exception:
        sd = torch.load(path, map_location="cpu", weights_only=False)
        return sd.state_dict() if hasattr(sd, "state_dict") else sd


class FILM_VFI:
    @classmethod
    def INPUT_TYPES(s):
        return {
            "required": {
                "ckpt_name": (["film_net_fp32.pt"],),
                "frames": ("IMAGE",),
                "clear_cache_after_n_frames": ("INT", {"default": 10, "min": 1, "max": 1000}),
                "multiplier": ("INT", {"default": 2, "min": 2, "max": 1000}),
            },
            "optional": {"optional_interpolation_states": ("INTERPOLATION_STATES",)},
        }

    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "vfi"
    CATEGORY = "ComfyUI-Frame-Interpolation/VFI"

    def vfi(self, ckpt_name: typing.AnyStr, frames: torch.Tensor, clear_cache_after_n_frames=10,
            multiplier: typing.SupportsInt = 2, optional_interpolation_states: InterpolationStateList = None, **kwargs):
        H, W = (int(v) for v in frames.shape[1:3])
        check_frame_size(H, W)      # before the checkpoint is read, an engine built or a frame uploaded
        model_path = load_file_from_github_release(MODEL_TYPE, ckpt_name)
        # (the reference re-loads the TorchScript file on every call, film/__init__.py:74; see ckpt.cached_engine)
        def build():
            sd = _load_state_dict(model_path)
            return film_lane_set(lambda: FilmEngine(sd))
        with engine_call(cached_engine(MODEL_TYPE, model_path, build), (H, W)) as engine:
            limit_lanes(engine, H, W)      # (the cached set may come from a call on frames of another size)
            plan, tasks = film_output_plan(len(frames), multiplier, optional_interpolation_states)
            return (run_plan(engine, frames, plan, tasks, film_pair, "FILM VFI"),)
