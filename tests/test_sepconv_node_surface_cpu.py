"""CPU: the Sepconv VFI node's surface — the reference's widgets (vfi_models/sepconv/__init__.py:11-29) — its opt-in registration
(config.yaml extra_nodes: "sepconv"), and its frame loop, which is CAIN's (schedule.bisect_output_plan against the reference's
generic_frame_loop(use_timestep=False), tests/golden/cain_schedule_kat.json)."""
import json
import os
import subprocess
import sys

import pytest

import cfi_amd
from cfi_amd import _lib
from cfi_amd.schedule import InterpolationStateList, bisect_output_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_widgets_match_the_reference():
    cls = cfi_amd.SepconvVFI
    it = cls.INPUT_TYPES()
    assert list(it["required"]) == ["ckpt_name", "frames", "clear_cache_after_n_frames", "multiplier"]
    assert it["required"]["ckpt_name"] == (["sepconv.pth"],)
    assert it["required"]["frames"] == ("IMAGE",)
    assert it["required"]["clear_cache_after_n_frames"] == ("INT", {"default": 10, "min": 1, "max": 1000})
    assert it["required"]["multiplier"] == ("INT", {"default": 2, "min": 2, "max": 1000})
    assert it["optional"] == {"optional_interpolation_states": ("INTERPOLATION_STATES",)}
    assert cls.RETURN_TYPES == ("IMAGE",) and cls.FUNCTION == "vfi" and cls.CATEGORY == "ComfyUI-Frame-Interpolation/VFI"


def _mappings(extra_nodes):
    patch = "" if extra_nodes is None else (
        "import cfi_amd.ckpt as k; real = k.load_config; k.load_config = lambda: dict(real(), extra_nodes=%r); " % extra_nodes)
    code = ("import sys; sys.path.insert(0, %r); from pkgload import load_package; load_package(); import cfi_amd; " % ROOT + patch +
            "print(sorted(cfi_amd.NODE_CLASS_MAPPINGS)); print(sorted(cfi_amd.NODE_DISPLAY_NAME_MAPPINGS))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    classes, names = [eval(line) for line in r.stdout.strip().splitlines()[-2:]]
    return set(classes), set(names)


def test_default_registry_has_no_sepconv():
    classes, names = _mappings(None)
    assert "Sepconv VFI" not in classes and "Sepconv VFI" not in names


def test_opt_in_registers_sepconv():
    classes, names = _mappings("sepconv")
    assert "Sepconv VFI" in classes and "Sepconv VFI" in names and "CAIN VFI" not in classes and names <= classes
    both = _mappings("cain, sepconv")[0]
    assert {"CAIN VFI", "Sepconv VFI"} <= both


def test_no_new_environment_variable():
    assert not any("SEPCONV" in v for v in _lib.SUPPORTED_ENV)


def _positions(n_frames, multiplier, skip):
    states = InterpolationStateList(skip, True) if skip else None
    plan, tasks = bisect_output_plan(n_frames, multiplier, states)
    new = [pair + p for pair, outs, _ in tasks for p in outs]
    return [float(idx) if kind == "src" else float(new[idx]) for kind, idx in plan], sum(len(c) for _, _, c in tasks)


def test_plans_of_the_node_cases_match_the_reference_loop(golden_dir):
    """Sepconv's node uses generic_frame_loop(use_timestep=False) exactly as CAIN's: the same known answers hold for every multiplier
    case of the goldens (2, 3, 5, lists, skip lists)"""
    with open(os.path.join(golden_dir, "cain_schedule_kat.json")) as f:
        kat = json.load(f)
    ms = {json.dumps(e["multiplier"]) for e in kat}
    assert {"2", "3", "5"} <= ms and any(m.startswith("[") for m in ms)
    for e in kat:
        got, calls = _positions(e["n_frames"], e["multiplier"], e["skip"])
        assert got == e["positions"], e
        assert calls == e["model_calls"], e


def test_multiplier_one_and_all_zero_lists_fail_up_front():
    with pytest.raises(ValueError):
        bisect_output_plan(3, 1, None)
    plan, _ = bisect_output_plan(3, [0, 0], None)
    assert plan == []
