"""CPU: ATM's multi-scale global-motion ensemble ("On with Ensemble (slowest)") behind config.yaml's ``atm_ensemble`` key — the unchanged
refusal with the key off, the routing with it on, the restatement of the ensemble (tests/atm_ensemble_restated.py) against the reference's
own outputs (tests/golden/atm_ens_net.npz, atm_base_ens_net.npz: frame <= 1e-3 per pixel, the same chosen level, losses within 1e-3
relative), the node loop on a stand-in engine against the reference node (atm_ens_node.npz, atm_base_ens_node.npz), and the conditions on
the golden inputs that make a pass mean something.  ``ckpt.load_config`` is patched to turn the key on: the package's config.yaml leaves it off.

Conditions (on the inputs, by the reference's own record and again through the float64 restatement): the smallest loss of every case is at
least 1e-2 (relative) below the second smallest; per model every level wins at least once; finite output with <= 10 % of its values
clamped; at least one case per model differs from "On" by more than 1e-2 somewhere; float32 within 1e-4 of float64."""
import os

import numpy as np
import pytest
import torch

import atm_ensemble_restated as E
import cain_restated
import cfi_amd
from cfi_amd import atm, atm_spec, ckpt

CASES = [(v, c) for v in ("lite", "base") for c in E.NET_CASES[v]]


@pytest.fixture(scope="module", autouse=True)
def threads():
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))      # as the golden writer


def _golden(golden_dir, variant, kind):
    return np.load(os.path.join(golden_dir, f"{E.GOLDEN_PREFIX[variant]}_{kind}.npz"))


def _no_engine(*a, **k):
    raise AssertionError("the refusals must come before the checkpoint and the engine")


def test_with_the_key_off_the_refusal_is_todays(monkeypatch):
    assert "atm_ensemble" not in ckpt.load_config() and not atm_spec.atm_ensemble_enabled()      # the package's own config.yaml
    monkeypatch.setattr(atm, "load_file_from_github_release", _no_engine)
    monkeypatch.setattr(atm, "cached_engine", _no_engine)
    for cfg in (None, E.config_with(False), E.config_with(False, True)):
        if cfg:
            monkeypatch.setattr(ckpt, "load_config", cfg)
        assert not atm_spec.atm_ensemble_enabled()
        assert atm.global_motion_flag("On") is True and atm.global_motion_flag("Off (fastest)") is False
        with pytest.raises(NotImplementedError, match=r"global_motion 'On with Ensemble \(slowest\)': the multi-scale global-motion ensemble is not built yet; "
                                                      r"use 'On' or 'Off \(fastest\)'"):
            atm.global_motion_flag(E.ENSEMBLE)
        with pytest.raises(NotImplementedError, match="On with Ensemble.*ensemble is not built yet"):
            cfi_amd.ATM_VFI().vfi("atm-vfi-lite.pt", torch.zeros(3, 64, 64, 3), 10, 2, E.ENSEMBLE)


def test_with_the_key_on_the_choice_is_routed_and_the_other_refusals_stay(monkeypatch):
    monkeypatch.setattr(ckpt, "load_config", E.config_with(True))
    assert atm_spec.atm_ensemble_enabled() and not atm_spec.atm_base_enabled()
    assert atm.global_motion_flag(E.ENSEMBLE) == atm.ENSEMBLE == 2
    assert atm.global_motion_flag("On") is True and atm.global_motion_flag("Off (fastest)") is False
    assert atm.ENSEMBLE != True and atm.ENSEMBLE != False      # noqa: E712  (the engine tells the three modes apart by value)
    with pytest.raises(KeyError, match="unknown global_motion"):
        atm.global_motion_flag("On with ensemble")
    monkeypatch.setattr(atm, "load_file_from_github_release", _no_engine)
    monkeypatch.setattr(atm, "cached_engine", _no_engine)
    for name in ("atm-vfi-base.pt", "atm-vfi-base-pct.pt"):      # ATM-base without its own key: refused first
        with pytest.raises(NotImplementedError, match=name + ".*ATM-base is not built yet"):
            cfi_amd.ATM_VFI().vfi(name, torch.zeros(3, 64, 64, 3), 10, 2, E.ENSEMBLE)
    big = torch.zeros(1, 1, 1, 3).expand(2, 2160, 4096, 3)
    with pytest.raises(ValueError, match="index arithmetic"):
        cfi_amd.ATM_VFI().vfi("atm-vfi-lite.pt", big, 10, 2, E.ENSEMBLE)
    monkeypatch.setattr(ckpt, "load_config", E.config_with(True, True))
    with pytest.raises(ValueError, match="for ATM-base"):
        cfi_amd.ATM_VFI().vfi("atm-vfi-base.pt", torch.zeros(1, 1, 1, 3).expand(2, 2160, 3840, 3), 10, 2, E.ENSEMBLE)


def test_the_mask_rule_of_the_shifted_block():
    """mask_level: a level whose map pads to the previous level's layout is masked with that level's pad regions"""
    assert E.mask_level([(4, 4), (2, 2), (1, 1)]) == [0, 0, 0]              # 64x64: all pad to 12x12
    assert E.mask_level([(12, 12), (6, 6), (3, 3)]) == [0, 0, 0]            # 192x192: level 0 has no padding at all
    assert E.mask_level([(12, 20), (6, 10), (3, 5)]) == [0, 1, 1]           # 192x320: 12x24, then 12x12 twice
    assert E.mask_level([(16, 28), (8, 14), (4, 7)]) == [0, 1, 2]           # 256x448: 24x36, 12x24, 12x12: every level its own
    assert E.mask_level([(68, 120), (34, 60), (17, 30)]) == [0, 1, 2]       # 1088x1920
    assert [E.select(l) for l in ([1, 1, 2], [2, 1, 1], [3, 2, 1], [1, 1, 1], [2, 1, 3])] == [0, 1, 2, 0, 1]


@pytest.mark.parametrize("variant,case", CASES)
def test_restatement_matches_the_reference(variant, case, golden_dir):
    golden = _golden(golden_dir, variant, "net")
    out, taps = E.restated(variant, case)
    d, sums_ok = cain_restated.compare(out, golden, case + "_", E.NET_STRIDE, E.TOL)
    want = [float(x) for x in golden[case + "_losses"]]
    rel = max(abs(a - b) / b for a, b in zip(taps["losses"], want))
    print(f"ATM-{variant} ensemble {case}: max |d| vs the reference {d:.3e}, losses {taps['losses']} (relative error {rel:.3e}), level {taps['level']}")
    assert d <= E.TOL and sums_ok
    assert taps["level"] == int(golden[case + "_level"])
    assert rel <= E.LOSS_TOL


def _margin(losses):
    ls = sorted(losses)
    return (ls[1] - ls[0]) / ls[1]


@pytest.mark.parametrize("variant,case", CASES)
def test_golden_case_meets_the_conditions(variant, case, golden_dir):
    golden = _golden(golden_dir, variant, "net")
    # the reference's own record
    assert _margin([float(x) for x in golden[case + "_losses"]]) >= E.MARGIN
    assert float(golden[case + "_clamped_frac"]) <= 0.10 and np.isfinite(golden[case + "_sample"]).all()
    # again through the float64 restatement
    out64, taps64 = E.restated(variant, case, torch.float64)
    out32, taps32 = E.restated(variant, case)
    clamped = float(((out64 <= 0) | (out64 >= 1)).double().mean())
    d32 = float((out32.double() - out64).abs().max())
    print(f"ATM-{variant} ensemble {case}: margin {_margin(taps64['losses']):.3e}, clamped {clamped:.4f}, float32 vs float64 {d32:.3e}")
    assert torch.isfinite(out64).all() and _margin(taps64["losses"]) >= E.MARGIN and clamped <= 0.10
    assert taps64["level"] == taps32["level"] == int(golden[case + "_level"])
    assert d32 <= 1e-4


@pytest.mark.parametrize("variant", ["lite", "base"])
def test_every_level_wins_and_the_ensemble_differs_from_on(variant, golden_dir):
    golden = _golden(golden_dir, variant, "net")
    cases = list(E.NET_CASES[variant])
    assert {int(golden[c + "_level"]) for c in cases} == {0, 1, 2}
    assert max(float(golden[c + "_on_diff_max"]) for c in cases) > 1e-2
    assert {E.restated(variant, c)[1]["level"] for c in cases} == {0, 1, 2}
    assert max(E.restated(variant, c)[1]["on_diff"] for c in cases) > 1e-2
    for c in cases:      # where level 0 wins the ensemble IS "On"
        if int(golden[c + "_level"]) == 0:
            assert float(golden[c + "_on_diff_max"]) == 0.0 and E.restated(variant, c)[1]["on_diff"] == 0.0


@pytest.fixture(scope="module", params=["lite", "base"])
def engine(request):
    return E.RestatedEnsemble(request.param)


@pytest.mark.parametrize("case", sorted(E.NODE_CASES))
def test_node_loop_matches_the_reference_node(case, engine, golden_dir, monkeypatch):
    golden = _golden(golden_dir, engine.variant, "node")
    before = engine.calls
    out = E.run_node(engine.variant, case, monkeypatch, engine)
    E.R.check_node_case(case, out, golden)
    n, h, w, c, m, skip = E.NODE_CASES[case]
    kept = [i for i in range(n - 1) if not (skip and i in skip)]
    assert engine.calls - before == len(kept) * (m - 1)          # one model call per new frame
    assert out.shape[0] == len(kept) * m + 1


def test_the_record_tap_is_in_the_test_library_only(hip_lib):
    """include/vfi_hip_test_atm.h: bound in the test build, absent from the product library (dlopen only, no call); the new entry points
    are the product library's"""
    import ctypes

    from cfi_amd import _lib

    assert list(_lib.ATM_TEST_PROTOTYPES) == ["vfi_atm_ensemble_record"] and hasattr(hip_lib, "vfi_atm_ensemble_record")
    product = ctypes.CDLL(_lib.LIB_PATH)
    assert not hasattr(product, "vfi_atm_ensemble_record")
    for name in ("vfi_atm_forward_ensemble", "vfi_atm_alignment_loss", "vfi_atm_alignment_scratch_floats", "vfi_atm_select_flow",
                 "vfi_atm_window_attention_labels"):
        assert hasattr(product, name) and name in _lib.PROTOTYPES
