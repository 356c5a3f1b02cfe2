"""CPU: the FLAVR VFI node's surface — the reference's widgets (vfi_models/flavr/__init__.py:28-47), its opt-in registration under
``flavr_vfi`` — and its private window loop (flavr.window_plan / run_windows) on a stand-in engine over the torch restatement, against
the reference node's own outputs in tests/golden/flavr_node.npz (tools/make_golden_flavr.py)."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import cain_restated
import cfi_amd
import flavr_restated
from cfi_amd import _lib, flavr, flavr_spec
from cfi_amd.schedule import InterpolationStateList

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, NODE_STRIDE = 1, 3
# name -> (frames, h, w, channels, multiplier, duplicate_first_last_frames, skip list, n_outputs): tools/make_golden_flavr.py NODE_CASES
NODE_CASES = {"n4": (4, 48, 72, 3, 2, False, None, 1), "n6": (6, 48, 72, 3, 2, False, None, 1), "dup": (5, 48, 72, 3, 2, True, None, 1),
              "skip01": (6, 48, 72, 3, 2, False, [0, 1], 1), "skip2": (6, 48, 72, 3, 2, False, [2], 1),
              "skiplast": (6, 48, 72, 3, 2, False, [2, 3], 1), "rgba": (4, 48, 72, 4, 2, False, None, 1),
              "m3": (4, 48, 72, 3, 3, False, None, 1), "odd": (5, 50, 70, 3, 2, False, None, 1), "x4": (4, 48, 72, 3, 2, False, None, 3)}
CKPT_OF = {1: "FLAVR_2x.pth", 3: "FLAVR_4x.pth"}


class RestatedFlavr:
    """FlavrEngine.forward on the CPU: one restated model call per window (test infrastructure only)."""

    def __init__(self, sd):
        self.sd, self.device = sd, torch.device("cpu")

    def forward(self, frames):
        def nchw(f):
            return f[..., :3].permute(2, 0, 1)[None].contiguous()

        with torch.no_grad():
            out = [flavr_restated.flavr_forward(self.sd, [nchw(f) for f in frames[i:i + 4]]) for i in range(0, len(frames), 4)]
        return torch.cat(out).permute(0, 2, 3, 1)

    def release_workspace(self):
        pass

    def workspace_bytes(self):
        return 0


def run_node(case, monkeypatch, engine_of):
    """The node's vfi() with the checkpoint lookup and the engine replaced: engine_of(n_outputs) -> engine"""
    n, h, w, c, m, dup, skip, n_outputs = NODE_CASES[case]
    monkeypatch.setattr(flavr, "load_file_from_github_release", lambda model_type, ckpt: ckpt)
    monkeypatch.setattr(flavr, "cached_engine", lambda model_type, path, build: (engine_of({v: k for k, v in CKPT_OF.items()}[path]), True))
    if engine_of(n_outputs).device.type == "cpu":
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    frames = cain_restated.seeded_frames(n, h, w, c, 9)
    states = InterpolationStateList(skip, True) if skip else None
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = cfi_amd.FLAVR_VFI().vfi(CKPT_OF[n_outputs], frames, 10, m, dup, states)[0]
    assert any("only supports 2x" in str(x.message) for x in caught) == (m != 2)
    return out


def check_case(case, out, golden):
    assert tuple(out.shape) == tuple(golden[case + "_shape"]) and out.dtype == torch.float32 and out.device.type == "cpu"
    d, sums_ok = cain_restated.compare(out, golden, case + "_", NODE_STRIDE, 1e-3)
    assert d <= 1e-3 and sums_ok, (case, d, sums_ok)


def test_widgets_match_the_reference():
    cls = cfi_amd.FLAVR_VFI
    it = cls.INPUT_TYPES()
    assert list(it["required"]) == ["ckpt_name", "frames", "clear_cache_after_n_frames", "multiplier", "duplicate_first_last_frames"]
    assert it["required"]["ckpt_name"] == (["FLAVR_2x.pth", "FLAVR_4x.pth", "FLAVR_8x.pth"],)
    assert it["required"]["frames"] == ("IMAGE",)
    assert it["required"]["clear_cache_after_n_frames"] == ("INT", {"default": 10, "min": 1, "max": 1000})
    assert it["required"]["multiplier"] == ("INT", {"default": 2, "min": 2, "max": 2})
    assert it["required"]["duplicate_first_last_frames"] == ("BOOLEAN", {"default": False})
    assert it["optional"] == {"optional_interpolation_states": ("INTERPOLATION_STATES",)}
    assert cls.RETURN_TYPES == ("IMAGE",) and cls.FUNCTION == "vfi" and cls.CATEGORY == "ComfyUI-Frame-Interpolation/VFI"
    assert flavr.CKPT_NAMES == ["FLAVR_2x.pth", "FLAVR_4x.pth", "FLAVR_8x.pth"] and flavr.MODEL_TYPE == "flavr"


def _mappings(extra_nodes):
    patch = "" if extra_nodes is None else (
        "import cfi_amd.ckpt as k; real = k.load_config; k.load_config = lambda: dict(real(), extra_nodes=%r); " % extra_nodes)
    code = ("import sys; sys.path.insert(0, %r); from pkgload import load_package; load_package(); import cfi_amd; " % ROOT + patch +
            "print(sorted(cfi_amd.NODE_CLASS_MAPPINGS)); print(sorted(cfi_amd.NODE_DISPLAY_NAME_MAPPINGS))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    classes, names = [eval(line) for line in r.stdout.strip().splitlines()[-2:]]
    return set(classes), set(names)


def test_default_registry_has_no_flavr():
    classes, names = _mappings(None)
    assert classes == {"RIFE VFI", "FILM VFI", "M2M VFI", "IFRNet VFI", "GMFSS Fortuna VFI", "IFUnet VFI", "Make Interpolation State List"}
    assert "FLAVR VFI" not in names


def test_opt_in_registers_flavr_under_flavr_vfi():
    classes, names = _mappings("flavr_vfi")
    assert "FLAVR VFI" in classes and "FLAVR VFI" in names and "CAIN VFI" not in classes and names <= classes
    assert {"CAIN VFI", "Sepconv VFI", "FLAVR VFI"} <= _mappings("cain, sepconv, FLAVR_VFI")[0]


def test_bare_flavr_stays_an_unknown_node():
    with pytest.raises(AssertionError, match="unknown node"):
        _mappings("flavr")
    assert "flavr" not in cfi_amd.EXTRA_NODES and "flavr_vfi" in cfi_amd.EXTRA_NODES


def test_no_new_environment_variable():
    assert not any("FLAVR" in v for v in _lib.SUPPORTED_ENV)


def test_window_plan_quirks():
    S = lambda idx: InterpolationStateList(idx, True)
    src, new = (lambda i: ("src", i)), (lambda i: ("new", i))
    assert flavr.window_plan(4) == [src(0), src(1), new(0), src(2), src(3)]
    assert flavr.window_plan(4, True) == [src(0), src(0), src(1), new(0), src(2), src(3), src(3)]
    assert flavr.window_plan(6, False, S([2])) == flavr.window_plan(6)                                  # one frame alone skips nothing
    assert flavr.window_plan(6, False, S([0, 1])) == [new(1), src(3), new(2), src(4), src(5)]            # frames 0..2 are lost
    assert flavr.window_plan(6, False, S([2, 3])) == [src(0), src(1), new(0), src(2), new(1), src(3)]    # frames 4, 5 are lost
    assert flavr.window_plan(4, False, S([0, 1])) == []
    keep = InterpolationStateList([0], False)                                                            # keep-list: every other frame skipped
    assert flavr.window_plan(6, False, keep) == [src(0), src(1), new(0), src(2)]
    for n, dup, skip in ((7, False, None), (6, True, [1, 2]), (5, False, [0, 1])):
        assert flavr.window_plan(n, dup, S(skip) if skip else None) == flavr_restated.window_plan(n, dup, skip)


@pytest.mark.parametrize("case", sorted(NODE_CASES))
def test_node_loop_matches_the_reference_node(case, golden_dir, monkeypatch):
    golden = np.load(os.path.join(golden_dir, "flavr_node.npz"))
    engines = {}

    def engine_of(n_outputs):
        if n_outputs not in engines:
            engines[n_outputs] = RestatedFlavr(flavr_spec.seeded_state_dict(SEED, n_outputs))
        return engines[n_outputs]

    check_case(case, run_node(case, monkeypatch, engine_of), golden)


def test_every_window_skipped_is_an_error(monkeypatch):
    monkeypatch.setattr(flavr, "load_file_from_github_release", lambda model_type, ckpt: ckpt)
    with pytest.raises(RuntimeError, match="every window was skipped"):
        flavr.run_windows(RestatedFlavr(None), cain_restated.seeded_frames(4, 16, 16, 3, 1), flavr.window_plan(4, False, InterpolationStateList([0, 1], True)))


def test_under_four_frames_assertion_text():
    with pytest.raises(AssertionError) as e:
        cfi_amd.FLAVR_VFI().vfi("FLAVR_2x.pth", torch.zeros(3, 16, 16, 3))
    assert str(e.value) == ("VFI model ST-MFNet requires at least 4 frames to work with, only found 3. "
                            "Please check the frame input using PreviewImage.")
