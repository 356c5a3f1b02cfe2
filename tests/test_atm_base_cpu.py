"""CPU: ATM-base behind config.yaml's ``atm_base`` key — the checkpoint layout (cfi_amd.atm_spec: CONFIG["base"], atm_shapes("base"), the
strict check) against the reference's own network_base.Network state dict as tools/make_golden_atm_base.py recorded it, the unchanged
refusals with the key off, the restatement of base's forward (tests/atm_base_restated.py) against the reference's own outputs
(tests/golden/atm_base_attn.npz, atm_base_attn_self.npz, atm_base_net.npz, atm_base_node.npz) within 1e-3 per pixel, the node loop on a
stand-in engine, base's own size guard, and the conditions on the seeded base weights that make those outputs worth comparing against.  ``ckpt.load_config`` is
patched to turn the key on: the package's config.yaml leaves it off.

Liveliness (conditions on the inputs, not measurements of the code under test; at every golden shape, in both modes, by the reference's own
record and again through the float64 restatement): read-out effect >= 1e-3, largest final flow >= 0.5 px, <= 10 % of the output clamped,
float32 within 1e-4 of float64.  Measured here (On / Off): effect 2.5e-2 .. 5.7e-2 / 2.8e-3 .. 5.2e-3, flows 1.80 .. 2.10 / 1.60 .. 2.03 px,
clamped <= 1.7 % / <= 1.5 %, float32 vs float64 <= 3.1e-5."""
import os

import numpy as np
import pytest
import torch

import atm_base_restated as B
import cain_restated
import cfi_amd
from cfi_amd import atm, atm_spec, ckpt


@pytest.fixture()
def base_on(monkeypatch):
    monkeypatch.setattr(ckpt, "load_config", B.config_with(True))


@pytest.fixture(scope="module", autouse=True)
def threads():
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))      # as the golden writer


def test_base_shapes_match_the_reference_state_dict(golden_dir):
    golden = np.load(os.path.join(golden_dir, "atm_base_net.npz"))
    want = atm_spec.atm_shapes(variant="base")
    assert list(want) == [str(k) for k in golden["sd_names"]]
    assert [",".join(map(str, v)) for v in want.values()] == [str(s) for s in golden["sd_shapes"]]
    assert len(want) == atm_spec.N_TENSORS == 236 and list(want) == list(atm_spec.atm_shapes()), "the same names in the same order as lite's"
    params = sum(int(np.prod(v)) for k, v in want.items() if not k.endswith(".relative_coord"))
    assert params == int(golden["n_parameters"]) == atm_spec.CONFIG["base"]["n_parameters"] == 51564259
    assert len(atm_spec.weight_shapes("base")) == 232 and not any("relative_coord" in k for k in atm_spec.weight_shapes("base"))
    assert want["feat_extracts.0.0.0.weight"] == (24, 3, 3, 3) and want["cross_scale_feature_fusion.proj.weight"] == (384, 384, 1, 1)
    assert want["global_feature_fusion.proj.weight"] == (672, 672, 1, 1) and want["last_feat_extract.0.0.weight"] == (288, 192, 3, 3)
    assert want["local_motion_atmformer.0.mlp.fc1.weight"] == (1536, 384) and want["global_motion_atmformer.1.mlp.dwconv.dwconv.weight"] == (2688, 1, 3, 3)
    assert want["local_motion_mlp.0.0.weight"] == (576, 776, 3, 3) and want["global_motion_mlp.0.0.weight"] == (768, 1352, 3, 3)
    assert want["upsample_pyramid.2.1.0.weight"] == (197, 101, 2, 2) and want["proj.0.weight"] == (64, 116, 3, 3)
    # lite's table is the parent's
    assert atm_spec.atm_shapes() == atm_spec.atm_shapes("lite") and atm_spec.weight_shapes() == atm_spec.weight_shapes("lite")
    assert atm_spec.VARIANTS == ("lite", "base")


def test_with_the_key_off_the_refusals_are_todays(tmp_path, monkeypatch):
    assert "atm_base" not in ckpt.load_config() and not atm_spec.atm_base_enabled()      # the package's own config.yaml
    sd_base = B.state_dict_as(torch.float32)
    for cfg in (None, B.config_with(False)):
        if cfg:
            monkeypatch.setattr(ckpt, "load_config", cfg)
        assert atm_spec.check_ckpt_name("atm-vfi-lite.pt") == "lite"
        for name in ("atm-vfi-base.pt", "atm-vfi-base-pct.pt"):
            with pytest.raises(NotImplementedError, match=name.replace(".", r"\.") + ": ATM-base is not built yet; only atm-vfi-lite.pt"):
                atm_spec.check_ckpt_name(name)
            with pytest.raises(NotImplementedError, match="ATM-base is not built yet"):
                atm_spec.load_file(str(tmp_path / name))       # the file does not exist: nothing was opened
        with pytest.raises(NotImplementedError, match="an ATM state dict with 24 first feature channels: ATM-base is not built yet"):
            atm_spec.check_state_dict(sd_base)
        with pytest.raises(NotImplementedError, match="ATM-base is not built yet"):
            atm_spec.check_state_dict(sd_base, "base")
        with pytest.raises(KeyError):
            atm_spec.check_ckpt_name("atm.pt")

        def no_engine(*a, **k):
            raise AssertionError("the refusals must come before the checkpoint and the engine")

        monkeypatch.setattr(atm, "load_file_from_github_release", no_engine)
        monkeypatch.setattr(atm, "cached_engine", no_engine)
        for name in ("atm-vfi-base.pt", "atm-vfi-base-pct.pt"):
            with pytest.raises(NotImplementedError, match=name + ".*ATM-base is not built yet"):
                cfi_amd.ATM_VFI().vfi(name, torch.zeros(3, 64, 64, 3), 10, 2, "On")


def test_with_the_key_on_base_is_served_and_checked_strictly(tmp_path, base_on):
    assert atm_spec.atm_base_enabled()
    assert [atm_spec.check_ckpt_name(n) for n in atm_spec.CKPT_NAMES] == ["base", "lite", "base"]
    with pytest.raises(KeyError):
        atm_spec.check_ckpt_name("atm.pt")
    sd, sd_lite = B.state_dict_as(torch.float32), atm_spec.seeded_state_dict(B.SEED)
    assert list(sd) == list(atm_spec.atm_shapes("base")) and all(v.dtype == torch.float32 for v in sd.values())
    assert atm_spec.check_state_dict(sd) == "base" and atm_spec.check_state_dict(sd, "base") == "base" and atm_spec.check_state_dict(sd_lite) == "lite"
    short = dict(sd)
    del short["proj.1.weight"]
    with pytest.raises(RuntimeError, match="Missing key"):
        atm_spec.check_state_dict(short)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        atm_spec.check_state_dict(dict(sd, extra=torch.zeros(1)))
    with pytest.raises(RuntimeError, match="size mismatch for global_motion_mlp.0.0.weight"):
        atm_spec.check_state_dict(dict(sd, **{"global_motion_mlp.0.0.weight": torch.zeros(672, 1352, 3, 3)}))
    bad = dict(sd)
    bad["global_motion_atmformer.1.attn.relative_coord"] = -sd["global_motion_atmformer.1.attn.relative_coord"]
    with pytest.raises(RuntimeError, match="relative_coord.*computes"):
        atm_spec.check_state_dict(bad)
    # a dict of the other model than the name stands for: a size mismatch, as for load_state_dict
    with pytest.raises(RuntimeError, match="size mismatch for feat_extracts.0.0.0.weight"):
        atm_spec.check_state_dict(sd_lite, "base")
    with pytest.raises(RuntimeError, match="size mismatch for feat_extracts.0.0.0.weight"):
        atm_spec.check_state_dict(sd, "lite")
    for name in ("atm-vfi-base.pt", "atm-vfi-base-pct.pt"):
        path = str(tmp_path / name)
        torch.save({"model_state_dict": dict(sd, **{"local_motion_atmformer.1.attn_mask": torch.zeros(4, 64, 64)})}, path)
        got = atm_spec.load_file(path)
        assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
        torch.save({"model_state_dict": sd_lite}, path)              # a lite dict under a base name
        with pytest.raises(RuntimeError, match="size mismatch"):
            atm_spec.load_file(path)
    path = str(tmp_path / "atm-vfi-lite.pt")
    torch.save({"model_state_dict": sd}, path)                       # a base dict under the lite name
    with pytest.raises(RuntimeError, match="size mismatch"):
        atm_spec.load_file(path)


def test_ensemble_and_oversized_frames_are_refused_before_an_engine_exists(monkeypatch, base_on):
    def no_engine(*a, **k):
        raise AssertionError("the refusals must come before the checkpoint and the engine")

    monkeypatch.setattr(atm, "load_file_from_github_release", no_engine)
    monkeypatch.setattr(atm, "cached_engine", no_engine)
    for name in ("atm-vfi-base.pt", "atm-vfi-base-pct.pt", "atm-vfi-lite.pt"):
        with pytest.raises(NotImplementedError, match="On with Ensemble.*ensemble is not built yet"):
            cfi_amd.ATM_VFI().vfi(name, torch.zeros(3, 64, 64, 3), 10, 2, "On with Ensemble (slowest)")
    # base's widest per-image buffer has 128 floats per padded pixel; its byte offsets must stay below 2 GiB
    assert atm.MAX_PADDED_PIXELS_BASE == 4194303 and (atm.MAX_PADDED_PIXELS_BASE + 1) * 128 * 4 > 2 ** 31 - 1 >= atm.MAX_PADDED_PIXELS_BASE * 128 * 4
    assert atm.MAX_PADDED_PIXELS == 6710886
    atm.check_frame_size(1080, 1920, "base"), atm.check_frame_size(1440, 2560, "base"), atm.check_frame_size(1472, 2560, "base")
    atm.check_frame_size(1600, 3000), atm.check_frame_size(1600, 3000, "lite")
    with pytest.raises(ValueError, match="index arithmetic .4194303 padded pixels for ATM-base"):
        atm.check_frame_size(1600, 3000, "base")
    with pytest.raises(ValueError, match="for ATM-base"):
        atm.check_frame_size(2176, 3840, "base")
    with pytest.raises(ValueError, match="for ATM-base"):
        cfi_amd.ATM_VFI().vfi("atm-vfi-base.pt", torch.zeros(1, 1, 1, 3).expand(2, 2160, 3840, 3), 10, 2, "On")


@pytest.mark.parametrize("cross", [True, False], ids=["cross", "self"])
@pytest.mark.parametrize("name", sorted(B.ATTN_CASES))
def test_block_restatement_matches_the_reference(name, cross, golden_dir):
    golden = np.load(os.path.join(golden_dir, B.attn_golden_file(cross)))
    h, w, win, shift = B.ATTN_CASES[name]
    p, x = B.attn_case(name, cross)
    with torch.no_grad():
        y, mot = B.window_block(p, x, win, shift, cross)
    kind = "cross" if cross else "self"
    d = float((y[..., ::B.ATTN_CH_STRIDE] - torch.from_numpy(golden[f"{name}_{kind}_x"])).abs().max())
    dm = float((mot - torch.from_numpy(golden[f"{name}_{kind}_motion"])).abs().max()) if cross else 0.0
    print(f"ATM-base {name} {kind}: max |d| {d:.3e}, motion {dm:.3e}")
    assert d <= B.TOL and dm <= B.TOL
    if cross:      # the case does what it is for: a read-out of pixels, not of rounding noise
        assert float(mot.abs().max()) > 1.0


@pytest.mark.parametrize("mode", sorted(B.MODES))
@pytest.mark.parametrize("shape_name", sorted(B.NET_SHAPES))
def test_forward_restatement_matches_the_reference(shape_name, mode, golden_dir):
    golden = np.load(os.path.join(golden_dir, "atm_base_net.npz"))
    out = B.restated32(shape_name, mode)
    key = f"{shape_name}_{'on' if B.MODES[mode] else 'off'}_"
    d, sums_ok = cain_restated.compare(out, golden, key, B.NET_STRIDE, B.TOL)
    print(f"ATM-base {shape_name} {mode}: max |d| vs the reference {d:.3e}")
    assert d <= B.TOL and sums_ok


@pytest.mark.parametrize("mode", sorted(B.MODES))
@pytest.mark.parametrize("shape_name", sorted(B.NET_SHAPES))
def test_seeded_base_weights_exercise_the_motion_path(shape_name, mode, golden_dir):
    golden = np.load(os.path.join(golden_dir, "atm_base_net.npz"))
    gm = B.MODES[mode]
    key = f"{shape_name}_{'on' if gm else 'off'}_"
    # the reference's own record
    assert float(golden[key + "motion_effect_mean"]) >= 1e-3 and float(golden[key + "max_flow"]) >= 0.5 and float(golden[key + "clamped_frac"]) <= 0.10
    f0, f1 = B.frames_of(shape_name)
    sd64, taps = B.state_dict_as(torch.float64), {}
    with torch.no_grad():
        out = B.atm_forward(sd64, f0.double(), f1.double(), gm, taps=taps)
        dark = B.atm_forward(sd64, f0.double(), f1.double(), gm, zero_motion=True)
    out32 = B.restated32(shape_name, mode).permute(2, 0, 1)[None]
    effect = float((out - dark).abs().mean())
    flow = float(max(taps["flow0"].abs().max(), taps["flow1"].abs().max()))
    clamped = float(((out <= 0) | (out >= 1)).double().mean())
    d32 = float((out32.double() - out).abs().max())
    print(f"ATM-base {shape_name} {mode}: motion effect {effect:.3e}, largest flow {flow:.3f} px, clamped {clamped:.4f}, float32 vs float64 {d32:.3e}")
    assert effect >= 1e-3
    assert flow >= 0.5
    assert clamped <= 0.10
    assert d32 <= 1e-4


@pytest.fixture(scope="module")
def engine():
    return B.RestatedAtmBase()


@pytest.mark.parametrize("ckpt_name", ["atm-vfi-base.pt", "atm-vfi-base-pct.pt"])
def test_both_base_names_reach_the_engine(ckpt_name, golden_dir, monkeypatch, engine):
    golden = np.load(os.path.join(golden_dir, "atm_base_node.npz"))
    B.check_node_case("m2", B.run_node("m2", monkeypatch, engine, ckpt_name), golden)


@pytest.mark.parametrize("case", sorted(set(B.NODE_CASES) - {"m2"}))
def test_node_loop_matches_the_reference_node(case, golden_dir, monkeypatch, engine):
    golden = np.load(os.path.join(golden_dir, "atm_base_node.npz"))
    before = engine.calls
    out = B.run_node(case, monkeypatch, engine)
    B.check_node_case(case, out, golden)
    n, h, w, c, m, skip, gm = B.NODE_CASES[case]
    ms = [m] * (n - 1) if isinstance(m, int) else list(m) + [2] * (n - 1 - len(m))
    kept = [i for i in range(n - 1) if not (skip and i in skip)]
    assert engine.calls - before == sum(ms[i] - 1 for i in kept)          # one model call per new frame
    assert out.shape[0] == sum(ms[i] for i in kept) + 1


def test_the_node_builds_a_base_engine_for_a_base_name(monkeypatch, base_on, tmp_path):
    """the variant is resolved from the name before anything is loaded, and is what the engine is created with"""
    seen = {}

    class Stop(Exception):
        pass

    def fake_engine(sd, variant):
        seen["variant"], seen["keys"] = variant, len(sd)
        raise Stop

    path = str(tmp_path / "atm-vfi-base-pct.pt")
    torch.save({"model_state_dict": B.state_dict_as(torch.float32)}, path)
    monkeypatch.setattr(atm, "load_file_from_github_release", lambda model_type, name: path)
    monkeypatch.setattr(atm, "cached_engine", lambda model_type, p, build: build())
    monkeypatch.setattr(atm, "AtmEngine", fake_engine)
    with pytest.raises(Stop):
        cfi_amd.ATM_VFI().vfi("atm-vfi-base-pct.pt", torch.zeros(2, 64, 64, 3), 10, 2, "On")
    assert seen == {"variant": "base", "keys": 236}
