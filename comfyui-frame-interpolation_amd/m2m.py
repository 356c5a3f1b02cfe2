"""M2M VFI node — host-side mirror of the reference's ``M2M_VFI`` over the HIP library.

Node shape and frame loop follow vfi_models/m2m/__init__.py:14-60 + vfi_utils.generic_frame_loop
(vfi_utils.py:149-389, timestep mode): frame_i, its multiplier-1 middle frames, ..., last frame; skipped pairs keep
their first frame; no clamp.  The model (vfi_models/m2m/M2M_arch.py ``M2M_PWC.forward`` :894-1037) is executed as
a sequence of the library's generic ops, issued by the C-side object vfi_m2m_* (csrc/m2m_object.hip):

    Basic("...sconv(2)-prelu-conv(3,replpad)-prelu...") / conv() / Conv2 / deconv()   -> vfi_conv_forward_ex (MFMA)
    costvol_func / softsplat_func (the reference's cupy kernels)                        -> vfi_costvol9x9 / vfi_softsplat_sum
    backwarp (grid_sample zeros, align_corners=True)                                    -> vfi_warp_m2m
    F.interpolate(bilinear) * scale                                                     -> vfi_resize_bilinear
    padding + joint normalisation, cube attention, photometric metric, splat
    inputs, normalise / hole fill / de-normalise                                        -> vfi_m2m_*

Both directions of a pair share every weight, so they run as a batch of 2 (image 0 = frame0->frame1 quantities,
image 1 = the reverse); "partner" reads use the swap flag of the kernels.  torch.cat along channels never
materialises: producers write into channel windows of pre-allocated NHWC tensors.

Unlike the reference (which re-runs the whole network for every timestep, vfi_utils.py:201-211), the flow / refine
part is timestep independent (M2M_arch.py:936-958) and runs ONCE per pair (``prepare``); only the splat runs per
timestep (``render``).  Results are identical; multiplier m costs 1 network pass + (m-1) splats.
"""
import typing

import torch

from . import _lib
from .ckpt import cached_engine, engine_call, load_file_from_github_release
from .lanes import lane_set
from .m2m_spec import check_state_dict, m2m_shapes
from . import nodeloop
from .netengine import NetEngine, WorkspaceBytes
from .schedule import InterpolationStateList, generic_output_plan

MODEL_TYPE = "m2m"
RATIO = 4        # M2M_PWC.forward default ratio (the node never overrides it, vfi_models/m2m/__init__.py:51-55)


class M2MEngine(WorkspaceBytes, NetEngine):
    """Device-resident M2M interpolator: ``prepare(frame0, frame1)`` once per pair, ``render(t)`` per timestep — the C-side
    object vfi_m2m_create / vfi_m2m_prepare / vfi_m2m_render / vfi_m2m_destroy (csrc/m2m_object.hip): weights packed once,
    workspace owned by the library, the ~110 launches of a pair issued by one call."""

    PREFIX, LABEL = "vfi_m2m", "M2M"
    shapes = staticmethod(m2m_shapes)
    check_state_dict = staticmethod(check_state_dict)
    hw = None           # (H, W) of the prepared pair

    def release_workspace(self):
        super().release_workspace()
        self.hw = None

    def prepare(self, frame0, frame1):
        """frame0/frame1: [H,W,C>=3] fp32 device tensors.  Runs everything that does not depend on the timestep (the frames are
        consumed by the first kernel of the call; later kernels read the library's own copies)."""
        H, W, Cc = frame0.shape
        assert frame1.shape == frame0.shape and Cc >= 3 and frame0.is_contiguous() and frame1.is_contiguous()
        assert frame0.is_cuda and frame0.dtype == torch.float32
        self._call("prepare", frame0.data_ptr(), frame1.data_ptr(), Cc, H, W, _lib.stream_ptr())
        self.hw = (H, W)

    def render(self, t, out=None):
        """One middle frame at time t for the prepared pair -> [H,W,3] device tensor (not clamped, like the reference)."""
        assert self.hw is not None, "prepare() first"
        H, W = self.hw
        if out is None:
            out = torch.empty((H, W, 3), dtype=torch.float32, device=self.device)
        self._call("render", float(t), out.data_ptr(), _lib.stream_ptr())
        return out

    def forward(self, frame0, frame1, t):
        self.prepare(frame0, frame1)
        return self.render(t)

    # -- test taps (include/vfi_hip_test.h) ------------------------------------------------------------------------------
    def _debug(self, what, shape):
        buf = torch.empty(shape, dtype=torch.float32)
        n = _lib.test_tap("vfi_m2m_debug_read")(self.handle, what, buf.data_ptr(), buf.numel())
        if n != buf.numel():
            raise RuntimeError("vfi_m2m_debug_read: " + _lib.last_error())
        return buf

    def _padded(self):
        m = RATIO * 16
        return (self.hw[0] + m - 1) // m * m, (self.hw[1] + m - 1) // m * m

    @property
    def flow(self):
        Hp, Wp = self._padded()
        return [self._debug(0, (2, Hp // 4, Wp // 4, 2))]

    @property
    def d0(self):
        return self._debug(1, (2,) + self._padded() + (8,))

    @property
    def r(self):
        return self._debug(2, (2,) + self._padded() + (12,))


def _load_state_dict(path):
    sd = torch.load(path, map_location="cpu", weights_only=False)
    return sd.state_dict() if hasattr(sd, "state_dict") else sd


def timestep_pair(eng, f0, f1, task):
    """The timestep pair kind of nodeloop.run_plan (M2M, IFRNet, GMFSS, IFUNet): task = (pair, [timesteps]); ``prepare`` once, then
    ``render(t, out)`` per timestep, each frame into a tensor of its own (allocated on the current stream: the pair's lane).  Yields
    every frame as soon as its render is queued, so that its copy-back is queued before the next render."""
    eng.prepare(f0, f1)
    for t in task[1]:
        out = torch.empty(f0.shape[:2] + (3,), dtype=torch.float32, device=f0.device)
        eng.render(t, out)
        yield out


def run_plan(engine, frames, plan, tasks, name="M2M VFI"):
    """nodeloop.run_plan with the timestep pair kind: the frame loop of the M2M, IFRNet, GMFSS and IFUNet nodes.  frames: [N,H,W,C] host
    tensor; plan / tasks from schedule.generic_output_plan."""
    return nodeloop.run_plan(engine, frames, plan, tasks, timestep_pair, name)


class M2M_VFI:
    @classmethod
    def INPUT_TYPES(s):
        return {
            "required": {
                "ckpt_name": (["M2M.pth"],),
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
        assert len(frames) >= 2, f"VFI model M2M requires at least 2 frames to work with, only found {frames.shape[0]}."
        model_path = load_file_from_github_release(MODEL_TYPE, ckpt_name)
        # (the reference rebuilds M2M_PWC on every call, m2m/__init__.py:43-46; see ckpt.cached_engine)
        def build():
            sd = _load_state_dict(model_path)
            return lane_set("m2m", lambda: M2MEngine(sd))
        # (the workspace, 0.3 GB per lane at 1080p, stays for the next clip of this frame shape: ckpt.KEEP_WORKSPACE_BYTES)
        with engine_call(cached_engine(MODEL_TYPE, model_path, build), tuple(frames.shape[1:3])) as engine:
            plan, tasks = generic_output_plan(len(frames), multiplier, optional_interpolation_states)
            return (run_plan(engine, frames, plan, tasks),)
