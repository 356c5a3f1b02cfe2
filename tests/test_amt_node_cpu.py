"""CPU: the AMT VFI node's surface — the reference's widgets (vfi_models/amt/__init__.py:11-50), its opt-in registration under ``amt_vfi``,
the size guard — and its frame loop (schedule.generic_output_plan + nodeloop.run_plan with amt.pair_frames: one forward per pair with all
of the pair's timesteps) on a stand-in engine over the torch restatement, against the reference node's own outputs in
tests/golden/amt_node.npz (tools/make_golden_amt.py).  tests/test_gpu_amt.py runs the same cases on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cfi_amd
from amt_restated import NODE_CASES, RestatedAmt, check_node_case, run_node
from cfi_amd import _lib, amt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
def test_widgets_match_the_reference():
    cls = cfi_amd.AMT_VFI
    it = cls.INPUT_TYPES()
    assert list(it["required"]) == ["ckpt_name", "frames", "clear_cache_after_n_frames", "multiplier"]
    assert it["required"]["ckpt_name"] == (["amt-s.pth", "amt-l.pth", "amt-g.pth", "gopro_amt-s.pth"],)
    assert it["required"]["frames"] == ("IMAGE",)
    assert it["required"]["clear_cache_after_n_frames"] == ("INT", {"default": 1, "min": 1, "max": 100})
    assert it["required"]["multiplier"] == ("INT", {"default": 2, "min": 2, "max": 1000})
    assert it["optional"] == {"optional_interpolation_states": ("INTERPOLATION_STATES",)}
    assert cls.RETURN_TYPES == ("IMAGE",) and cls.FUNCTION == "vfi" and cls.CATEGORY == "ComfyUI-Frame-Interpolation/VFI"
    assert amt.MODEL_TYPE == "amt" and amt.CKPT_URL.format(ckpt_name="amt-s.pth") == "https://huggingface.co/lalala125/AMT/resolve/main/amt-s.pth"


def _mappings(extra_nodes):
    patch = "" if extra_nodes is None else (
        "import cfi_amd.ckpt as k; real = k.load_config; k.load_config = lambda: dict(real(), extra_nodes=%r); " % extra_nodes)
    code = ("import sys; sys.path.insert(0, %r); from pkgload import load_package; load_package(); import cfi_amd; " % ROOT + patch +
            "print(sorted(cfi_amd.NODE_CLASS_MAPPINGS)); print(sorted(cfi_amd.NODE_DISPLAY_NAME_MAPPINGS))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    classes, names = [eval(line) for line in r.stdout.strip().splitlines()[-2:]]
    return set(classes), set(names)


def test_opt_in_registry_in_a_fresh_process():
    classes, names = _mappings(None)
    assert classes == {"RIFE VFI", "FILM VFI", "M2M VFI", "IFRNet VFI", "GMFSS Fortuna VFI", "IFUnet VFI", "Make Interpolation State List"}
    assert "AMT VFI" not in names
    classes, names = _mappings("amt_vfi")
    assert "AMT VFI" in classes and "AMT VFI" in names and "FLAVR VFI" not in classes and names <= classes
    assert cfi_amd.EXTRA_NODES["amt_vfi"] == ("AMT VFI", "AMT VFI (MI355X HIP)")
    with pytest.raises(AssertionError, match="unknown node"):
        _mappings("amt")
    assert "amt" not in cfi_amd.EXTRA_NODES
    assert not any("AMT" in v for v in _lib.SUPPORTED_ENV)


def test_size_guard_raises_before_an_engine_exists(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("the size guard must come before the checkpoint and the engine")

    monkeypatch.setattr(amt, "load_file_from_direct_url", no_engine)
    monkeypatch.setattr(amt, "cached_engine", no_engine)
    with pytest.raises(ValueError, match="at least 128"):
        cfi_amd.AMT_VFI().vfi("amt-s.pth", torch.zeros(3, 100, 300, 3))
    with pytest.raises(ValueError, match="index arithmetic"):
        amt.check_frame_size(4096, 4096)
    amt.check_frame_size(113, 128), amt.check_frame_size(1080, 1920), amt.check_frame_size(2160, 3840)
    assert amt.padded_size(130, 200) == (144, 208) and amt.padded_size(128, 1920) == (128, 1920)
    with pytest.raises(NotImplementedError, match="amt-g.pth"):
        cfi_amd.AMT_VFI().vfi("amt-g.pth", torch.zeros(3, 128, 128, 3))


@pytest.mark.parametrize("case", sorted(NODE_CASES))
def test_node_loop_matches_the_reference_node(case, golden_dir, monkeypatch):
    golden = np.load(os.path.join(golden_dir, "amt_node.npz"))
    engines = {}

    def engine_of(variant):
        if variant not in engines:
            engines[variant] = RestatedAmt(variant)
        return engines[variant]

    check_node_case(case, run_node(case, monkeypatch, engine_of), golden)
    # one forward per pair that has new frames, with all of that pair's timesteps
    _, n, _, _, _, m, skip = NODE_CASES[case]
    calls = [c for e in engines.values() for c in e.calls]
    ms = [m] * (n - 1) if isinstance(m, int) else list(m) + [2] * (n - 1 - len(m))
    want = [[k / mm for k in range(1, mm)] for i, mm in enumerate(ms) if mm > 1 and not (skip and isinstance(m, int) and i in skip)]
    assert calls == want
