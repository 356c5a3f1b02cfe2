"""CPU: the ATM VFI node's surface — the reference's widgets (vfi_models/atm/__init__.py:76-112), its opt-in registration under ``atm_vfi``,
the refusals by name — and its frame loop (schedule.film_output_plan + nodeloop.run_plan with atm.atm_pair: the reference's greedy midpoint
recursion, a skipped pair leaving no frame at all) on a stand-in engine over the torch restatement, against the reference node's own outputs
in tests/golden/atm_node.npz (tools/make_golden_atm.py).  tests/test_gpu_atm.py runs node cases on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cfi_amd
from atm_restated import NODE_CASES, RestatedAtm, check_node_case, run_node
from cfi_amd import _lib, atm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_widgets_match_the_reference():
    cls = cfi_amd.ATM_VFI
    it = cls.INPUT_TYPES()
    assert list(it["required"]) == ["ckpt_name", "frames", "clear_cache_after_n_frames", "multiplier", "global_motion"]
    assert it["required"]["ckpt_name"] == (["atm-vfi-base.pt", "atm-vfi-lite.pt", "atm-vfi-base-pct.pt"],)
    assert it["required"]["frames"] == ("IMAGE",)
    assert it["required"]["clear_cache_after_n_frames"] == ("INT", {"default": 10, "min": 1, "max": 1000})
    assert it["required"]["multiplier"] == ("INT", {"default": 2, "min": 2, "max": 2})
    assert it["required"]["global_motion"] == (["On", "On with Ensemble (slowest)", "Off (fastest)"],)
    assert it["optional"] == {"optional_interpolation_states": ("INTERPOLATION_STATES",)}
    assert cls.RETURN_TYPES == ("IMAGE",) and cls.FUNCTION == "vfi" and cls.CATEGORY == "ComfyUI-Frame-Interpolation/VFI"
    assert atm.MODEL_TYPE == "atm"
    import inspect

    assert list(inspect.signature(cls.vfi).parameters)[1:] == ["ckpt_name", "frames", "clear_cache_after_n_frames", "multiplier", "global_motion",
                                                               "optional_interpolation_states", "kwargs"]


def _mappings(extra_nodes):
    patch = "" if extra_nodes is None else (
        "import cfi_amd.ckpt as k; real = k.load_config; k.load_config = lambda: dict(real(), extra_nodes=%r); " % extra_nodes)
    code = ("import sys; sys.path.insert(0, %r); from pkgload import load_package; load_package(); import cfi_amd; " % ROOT + patch +
            "print(sorted(cfi_amd.NODE_CLASS_MAPPINGS)); print(sorted(cfi_amd.NODE_DISPLAY_NAME_MAPPINGS)); "
            "print(sorted(m for m in sys.modules if m.split('.')[0] in ('timm', 'einops')))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    classes, names, heavy = [eval(line) for line in r.stdout.strip().splitlines()[-3:]]
    return set(classes), set(names), heavy


def test_opt_in_registry_in_a_fresh_process():
    classes, names, _ = _mappings(None)
    assert classes == {"RIFE VFI", "FILM VFI", "M2M VFI", "IFRNet VFI", "GMFSS Fortuna VFI", "IFUnet VFI", "Make Interpolation State List"}
    assert "ATM VFI" not in names
    classes, names, heavy = _mappings("atm_vfi")
    assert "ATM VFI" in classes and "ATM VFI" in names and "AMT VFI" not in classes and names <= classes
    assert heavy == [], "the product path imports neither timm nor einops"
    assert cfi_amd.EXTRA_NODES["atm_vfi"] == ("ATM VFI", "ATM VFI (MI355X HIP)")
    with pytest.raises(AssertionError, match="unknown node"):
        _mappings("atm")
    assert "atm" not in cfi_amd.EXTRA_NODES
    assert not any("ATM" in v for v in _lib.SUPPORTED_ENV)


def test_refusals_come_before_an_engine_exists(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("the refusals must come before the checkpoint and the engine")

    monkeypatch.setattr(atm, "load_file_from_github_release", no_engine)
    monkeypatch.setattr(atm, "cached_engine", no_engine)
    frames = torch.zeros(3, 64, 64, 3)
    with pytest.raises(NotImplementedError, match="On with Ensemble.*ensemble is not built yet"):
        cfi_amd.ATM_VFI().vfi("atm-vfi-lite.pt", frames, 10, 2, "On with Ensemble (slowest)")
    for ckpt in ("atm-vfi-base.pt", "atm-vfi-base-pct.pt"):
        with pytest.raises(NotImplementedError, match=ckpt + ".*ATM-base is not built yet"):
            cfi_amd.ATM_VFI().vfi(ckpt, frames, 10, 2, "On")
    with pytest.raises(KeyError):
        cfi_amd.ATM_VFI().vfi("atm-vfi-lite.pt", frames, 10, 2, "Sometimes")
    with pytest.raises(ValueError, match="index arithmetic"):
        cfi_amd.ATM_VFI().vfi("atm-vfi-lite.pt", torch.zeros(1, 1, 1, 3).expand(2, 2160, 3840, 3), 10, 2, "On")


@pytest.fixture(scope="module")
def engine():
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    return RestatedAtm()


@pytest.mark.parametrize("case", sorted(NODE_CASES))
def test_node_loop_matches_the_reference_node(case, golden_dir, monkeypatch, engine):
    golden = np.load(os.path.join(golden_dir, "atm_node.npz"))
    before = engine.calls
    out = run_node(case, monkeypatch, engine)
    check_node_case(case, out, golden)
    n, h, w, c, m, skip, gm = NODE_CASES[case]
    ms = [m] * (n - 1) if isinstance(m, int) else list(m) + [2] * (n - 1 - len(m))
    kept = [i for i in range(n - 1) if not (skip and i in skip)]
    assert engine.calls - before == sum(ms[i] - 1 for i in kept)          # one model call per new frame
    assert out.shape[0] == sum(ms[i] for i in kept) + 1                   # a skipped pair leaves nothing, not even its first frame
    if case == "odd_on":
        assert atm.padded_size(h, w) == (128, 192) and ((128 - h) // 2, (192 - w) // 2) == (14, 6)
