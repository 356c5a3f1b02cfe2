"""ATM VFI node — host-side mirror of the reference's ``ATM_VFI`` over the HIP library.

Node shape follows vfi_models/atm/__init__.py:76-182: the three checkpoint names, the three ``global_motion`` choices and the ``vfi``
keywords.  ``atm-vfi-lite.pt`` is served; ``atm-vfi-base.pt`` / ``atm-vfi-base-pct.pt`` (ATM-base) are served when config.yaml's ``atm_base``
key is on and raise NotImplementedError naming themselves otherwise; ``"On with Ensemble (slowest)"`` (the multi-scale global-motion
ensemble, network_lite.py:540-704) is served for both models when config.yaml's ``atm_ensemble`` key is on and raises NotImplementedError by
name otherwise.  All of this before anything is loaded.  The frame loop is the
reference's own (:152-177): per kept pair the first frame and the new frames of ``inference()`` (:39-74) — FILM's greedy midpoint schedule,
every model call the midpoint of two known frames, clamped to [0, 1] and re-used —, a skipped pair contributes nothing at all, the clip's
last frame is appended: schedule.film_output_plan + nodeloop.run_plan with film.film_schedule.  Each model call is ONE vfi_atm_forward
(csrc/atm_net.hip), or ONE vfi_atm_forward_ensemble in the ensemble mode (the global branch at scales 1, 1/2 and 1/4, scored and chosen on
the device): centred replicate pad to multiples of 64, the network, un-pad, clamp.  No pair lanes, no HIP graph.

Frame size: 6 710 886 (lite) / 4 194 303 (base) padded pixels; with config.yaml's ``atm_large_frames`` key on 13 421 772 / 8 388 607, which
lets both models take 2160x3840 in every ``global_motion`` mode (vfi_atm_set_large_frames; the layers' large-image kernel forms).
"""
import typing

import torch

from . import _lib
from .atm_spec import CKPT_NAMES, VARIANTS, atm_ensemble_enabled, atm_large_frames_enabled, check_ckpt_name, check_state_dict, load_file, weight_shapes
from .ckpt import cached_engine, engine_call, load_file_from_github_release
from .film import film_schedule
from .netengine import NetEngine, WorkspaceBytes, check_frames, padded_to
from .nodeloop import run_plan
from .schedule import InterpolationStateList, film_output_plan

MODEL_TYPE = "atm"
GLOBAL_MOTION = {"On": (True, False), "On with Ensemble (slowest)": (True, True), "Off (fastest)": (False, False)}      # (global motion, ensemble)
ENSEMBLE = 2      # global_motion_flag's value for the ensemble choice (True / False: on / off), what AtmEngine.forward routes to vfi_atm_forward_ensemble
FLOATS_PER_PADDED_PIXEL = 80      # the widest per-image buffer: the refinement net's input, 76 channels padded to 80 (csrc/atm_net.hip)
MAX_PADDED_PIXELS = ((1 << 31) - 1) // (FLOATS_PER_PADDED_PIXEL * 4)      # = vfi_atm_max_padded_pixels(): 6 710 886
# ATM-base: the refinement net's full-resolution concat buffer, 2 * 64 = 128 channels (kCfg[1].px_floats, csrc/atm_net.hip): 1472x2560 fits,
# 2176x3840 does not; tests/test_gpu_atm_base.py asserts that this limit is vfi_atm_object_max_padded_pixels' of a base object
BASE_FLOATS_PER_PADDED_PIXEL = 128
MAX_PADDED_PIXELS_BASE = ((1 << 31) - 1) // (BASE_FLOATS_PER_PADDED_PIXEL * 4)      # 4 194 303
# with config.yaml's atm_large_frames on: one image below 4 GiB, served by the layer kernels' large-image forms
# (= vfi_atm_large_max_padded_pixels(0 / 1): 13 421 772 / 8 388 607; 2160x3840, padded 2176x3840 = 8 355 840, fits both)
LARGE_MAX_PADDED_PIXELS = ((1 << 32) - 1) // (FLOATS_PER_PADDED_PIXEL * 4)
LARGE_MAX_PADDED_PIXELS_BASE = ((1 << 32) - 1) // (BASE_FLOATS_PER_PADDED_PIXEL * 4)


def padded_size(H, W):
    """InputPadder(dims, 64) (atm/__init__.py:13-17): the sides rounded up to multiples of 64"""
    return padded_to(H, 64), padded_to(W, 64)


def max_padded_pixels(variant="lite", large=None):
    """The limit in force for a variant: today's, or the large one with config.yaml's ``atm_large_frames`` on (``large``: the key's state
    where the caller has read it already; None: read now)"""
    if atm_large_frames_enabled() if large is None else large:
        return LARGE_MAX_PADDED_PIXELS_BASE if variant == "base" else LARGE_MAX_PADDED_PIXELS
    return MAX_PADDED_PIXELS_BASE if variant == "base" else MAX_PADDED_PIXELS


def check_frame_size(H, W, variant="lite", large=None):
    Hp, Wp = padded_size(H, W)
    limit = max_padded_pixels(variant, large)
    if Hp * Wp > limit:
        raise ValueError(f"ATM VFI: {H}x{W} frames (padded {Hp}x{Wp}) are beyond the kernels' index arithmetic ({limit} padded pixels"
                         f"{' for ATM-base' if variant == 'base' else ''})")


def global_motion_flag(global_motion):
    """The widget's choice -> True / False, or ENSEMBLE for the ensemble choice when config.yaml's ``atm_ensemble`` key is on; without the key
    the ensemble choice raises by name, as unknown ones do."""
    if global_motion not in GLOBAL_MOTION:
        raise KeyError(f"unknown global_motion {global_motion!r} (known: {list(GLOBAL_MOTION)})")
    on, ensemble = GLOBAL_MOTION[global_motion]
    if ensemble and atm_ensemble_enabled():
        return ENSEMBLE
    if ensemble:
        raise NotImplementedError(f"global_motion {global_motion!r}: the multi-scale global-motion ensemble is not built yet; use 'On' or 'Off (fastest)'")
    return on


class AtmEngine(WorkspaceBytes, NetEngine):
    """Device-resident ATM-lite or ATM-base (``variant``; base only with config.yaml's ``atm_base`` on): ``forward(frame0, frame1,
    global_motion)`` = the model's clamped, un-padded midpoint frame of one pair; global_motion: False / True, or ENSEMBLE for the multi-scale
    ensemble."""

    PREFIX, LABEL = "vfi_atm", "ATM"

    def __init__(self, state_dict, variant="lite", device=None):
        assert variant in VARIANTS, f"variant: one of {VARIANTS}"
        self.variant = variant
        super().__init__(state_dict, device, VARIANTS.index(variant))

    def _fn(self, name):
        return super()._fn("create_variant" if name == "create" else name)

    def shapes(self):
        return weight_shapes(self.variant)

    def check_state_dict(self, state_dict):
        check_state_dict(state_dict, self.variant)

    def _sync_large_frames(self):
        """The object's limit follows config.yaml's ``atm_large_frames`` key as it is now"""
        self._call("set_large_frames", int(atm_large_frames_enabled()))

    def max_padded_pixels(self):
        self._sync_large_frames()
        return int(self._fn("object_max_padded_pixels")(self.handle))

    def forward(self, frame0, frame1, global_motion=True, out=None):
        """frame0 / frame1: [H,W,C>=3] fp32 contiguous device tensors (not written) -> [H,W,3]."""
        H, W, Cc = check_frames(frame0, frame1)
        Hp, Wp = padded_size(H, W)
        if Hp * Wp > (MAX_PADDED_PIXELS_BASE if self.variant == "base" else MAX_PADDED_PIXELS):
            # only a frame beyond the 2 GiB limit needs the key: read it now (one config.yaml parse, 0.7 ms, on a frame of 65 ms and more);
            # every smaller frame runs what it always ran, whatever the key and the object's switch say
            large = atm_large_frames_enabled()
            check_frame_size(H, W, self.variant, large)
            self._call("set_large_frames", int(large))
        if out is None:
            out = torch.empty((H, W, 3), dtype=torch.float32, device=self.device)
        if global_motion == ENSEMBLE:
            self._call("forward_ensemble", frame0.data_ptr(), frame1.data_ptr(), Cc, H, W, out.data_ptr(), _lib.stream_ptr())
        else:
            self._call("forward", frame0.data_ptr(), frame1.data_ptr(), Cc, H, W, int(bool(global_motion)), out.data_ptr(), _lib.stream_ptr())
        return out

    def ensemble_record(self):
        """(three losses, chosen level) of the last ensemble forward (a test tap: libvfi_hip_test.so only); synchronises its stream"""
        import ctypes

        losses, level = (ctypes.c_float * 3)(), ctypes.c_int()
        _lib.check(_lib.test_tap("vfi_atm_ensemble_record")(self.handle, losses, ctypes.byref(level)), "vfi_atm_ensemble_record")
        return [float(x) for x in losses], level.value


def atm_pair(eng, f0, f1, task, global_motion):
    """One pair of the plan: task = (pair, positions) of schedule.film_output_plan.  The greedy midpoint schedule runs sequentially on the
    current stream; every output is clamped (by the forward) and re-used as an input."""
    new = task[1]
    res = {0: f0, len(new) + 1: f1}
    for l, r, k in film_schedule(len(new)):
        res[k] = eng.forward(res[l], res[r], global_motion)
    return [res[k] for k in new]


class ATM_VFI:
    @classmethod
    def INPUT_TYPES(s):
        return {
            "required": {
                "ckpt_name": (list(CKPT_NAMES),),
                "frames": ("IMAGE",),
                "clear_cache_after_n_frames": ("INT", {"default": 10, "min": 1, "max": 1000}),
                "multiplier": ("INT", {"default": 2, "min": 2, "max": 2}),
                "global_motion": (["On", "On with Ensemble (slowest)", "Off (fastest)"],),
            },
            "optional": {"optional_interpolation_states": ("INTERPOLATION_STATES",)},
        }

    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "vfi"
    CATEGORY = "ComfyUI-Frame-Interpolation/VFI"

    def vfi(self, ckpt_name: typing.AnyStr, frames: torch.Tensor, clear_cache_after_n_frames=10, multiplier: typing.SupportsInt = 2,
            global_motion="On", optional_interpolation_states: InterpolationStateList = None, **kwargs):
        variant = check_ckpt_name(ckpt_name)            # ATM-base without the atm_base key: NotImplementedError naming the file, before anything is loaded
        gm = global_motion_flag(global_motion)          # the ensemble without the atm_ensemble key likewise, for both models
        check_frame_size(*frames.shape[1:3], variant)   # before an engine exists
        plan, tasks = film_output_plan(len(frames), multiplier, optional_interpolation_states)
        model_path = load_file_from_github_release(MODEL_TYPE, ckpt_name)
        entry = cached_engine(MODEL_TYPE, model_path, lambda: AtmEngine(load_file(model_path, ckpt_name), variant))
        with engine_call(entry, tuple(frames.shape[1:3])) as engine:
            return (run_plan(engine, frames, plan, tasks, lambda e, f0, f1, t: atm_pair(e, f0, f1, t, gm), "ATM VFI"),)
