"""CPU: AMT-G behind config.yaml's ``amt_g`` key — the checkpoint layout (cfi_amd.amt_spec: CONFIG["G"], amt_shapes("G"), the strict
check), the unchanged refusals with the key off, the restatement of AMT_G's forward (tests/amt_g_restated.py, the reference's order of
resize and convc1) against the reference's own outputs (tests/golden/amt_g_net.npz, amt_g_node.npz; tools/make_golden_amt_g.py), the
conditions on the seeded checkpoint, the node loop on a stand-in engine, and AMT-G's own size guard.  ``ckpt.load_config`` is patched to
turn the key on: the package's config.yaml leaves it off."""
import os

import numpy as np
import pytest
import torch

import amt_g_restated
import cain_restated
import cfi_amd
from amt_g_restated import NET_SHAPES, NET_STRIDE, NET_TS, NODE_CASES, SEED, TOL, UPDATE_BLOCKS, config_with
from amt_restated import frames_of
from cfi_amd import amt, amt_spec, ckpt


@pytest.fixture()
def g_on(monkeypatch):
    monkeypatch.setattr(ckpt, "load_config", config_with(True))


@pytest.fixture(scope="module")
def sd_g():
    return amt_spec.seeded_state_dict("G", SEED)


def test_shapes_counts_and_reference_key_order(golden_dir):
    shapes = amt_spec.amt_shapes("G")
    assert len(shapes) == 259 and sum(int(np.prod(s)) for s in shapes.values()) == 30638919
    golden = np.load(os.path.join(golden_dir, "amt_g_net.npz"))
    assert list(shapes) == [str(k) for k in golden["state_dict_keys"]]      # the reference's own AMT_G().state_dict() order
    assert shapes["encoder.pyramid1.0.0.weight"] == (84, 3, 7, 7) and shapes["feat_encoder.layer3_2.1.conv2.weight"] == (160, 160, 3, 3)
    assert shapes["feat_encoder.conv2.weight"] == (128, 160, 1, 1) and "feat_encoder.layer3_2.0.downsample.0.weight" not in shapes
    for blk, cdim in zip(UPDATE_BLOCKS, (112, 96, 84, 96, 84)):
        assert shapes[blk + ".convf1.weight"] == (128, 4, 7, 7) and shapes[blk + ".convc2.weight"] == (192, 256, 3, 3)
        assert shapes[blk + ".gru.0.weight"] == (192, 188 + 4 + cdim, 3, 3) and shapes[blk + ".feat_head.2.weight"] == (cdim, 192, 3, 3)
    keys = list(shapes)
    firsts = [keys.index(b + ".convc1.weight") for b in UPDATE_BLOCKS]
    assert firsts == sorted(firsts), "the update blocks are in registration order"
    # the tables beside G's are the parent's
    assert amt_spec.VARIANTS == ("S", "L") and amt_spec.CKPT_VARIANT["amt-g.pth"] is None
    assert len(amt_spec.amt_shapes("S")) == 213 and len(amt_spec.amt_shapes("L")) == 207


def test_with_the_key_off_the_refusals_are_unchanged(tmp_path, sd_g, monkeypatch):
    assert "amt_g" not in ckpt.load_config() and not amt_spec.amt_g_enabled()      # the package's own config.yaml
    for cfg in (None, config_with(False)):
        if cfg:
            monkeypatch.setattr(ckpt, "load_config", cfg)
        with pytest.raises(NotImplementedError, match="amt-g.pth: AMT-G has a forward of its own"):
            amt_spec.variant_of_ckpt("amt-g.pth")
        with pytest.raises(NotImplementedError, match="amt-g.pth"):
            amt_spec.load_file(os.path.join(tmp_path, "amt-g.pth"))      # the file does not exist: nothing was opened
        with pytest.raises(NotImplementedError, match="this state dict is AMT-G's"):
            amt_spec.check_state_dict(sd_g)
        with pytest.raises(KeyError):
            amt_spec.variant_of_ckpt("amt-x.pth")

        def no_engine(*a, **k):
            raise AssertionError("amt-g.pth must be refused before the checkpoint and the engine")

        monkeypatch.setattr(amt, "load_file_from_direct_url", no_engine)
        monkeypatch.setattr(amt, "cached_engine", no_engine)
        with pytest.raises(NotImplementedError, match="amt-g.pth"):
            cfi_amd.AMT_VFI().vfi("amt-g.pth", torch.zeros(3, 128, 128, 3))
        with pytest.raises(NotImplementedError, match="amt-g.pth"):      # the name comes before the size, as before
            cfi_amd.AMT_VFI().vfi("amt-g.pth", torch.zeros(3, 100, 300, 3))


def test_with_the_key_on_g_is_served_and_checked_strictly(tmp_path, sd_g, g_on):
    assert amt_spec.amt_g_enabled() and amt_spec.variant_of_ckpt("amt-g.pth") == "G" and amt_spec.variant_of_ckpt("amt-l.pth") == "L"
    assert list(sd_g) == list(amt_spec.amt_shapes("G")) and all(v.dtype == torch.float32 for v in sd_g.values())
    assert amt_spec.check_state_dict(sd_g) == "G" and amt_spec.check_state_dict(sd_g, "G") == "G"
    missing = dict(sd_g)
    del missing["update3_high.gru.2.bias"]
    with pytest.raises(RuntimeError, match="Missing key"):
        amt_spec.check_state_dict(missing)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        amt_spec.check_state_dict(dict(sd_g, extra=torch.zeros(1)))
    with pytest.raises(RuntimeError, match="size mismatch for update2_high.convf1.weight"):
        amt_spec.check_state_dict(dict(sd_g, **{"update2_high.convf1.weight": torch.zeros(96, 4, 7, 7)}))
    # S, L and foreign dicts are told apart as before
    sd_l = amt_spec.seeded_state_dict("L", SEED)
    assert amt_spec.check_state_dict(sd_l) == "L"
    with pytest.raises(RuntimeError, match="not an AMT state dict"):
        amt_spec.check_state_dict({"x": torch.zeros(1)})
    # the {"state_dict": ...} file, and dicts under the wrong name
    path = os.path.join(tmp_path, "amt-g.pth")
    torch.save({"state_dict": sd_g}, path)
    got, variant = amt_spec.load_file(path)
    assert variant == "G" and list(got) == list(sd_g) and all(torch.equal(got[k], sd_g[k]) for k in sd_g)
    torch.save({"state_dict": sd_l}, path)              # an L dict under amt-g.pth
    with pytest.raises(RuntimeError, match="AMT-L state dict where AMT-G"):
        amt_spec.load_file(path)
    path_l = os.path.join(tmp_path, "amt-l.pth")
    torch.save({"state_dict": sd_g}, path_l)            # a G dict under amt-l.pth
    with pytest.raises(RuntimeError, match="AMT-G state dict where AMT-L"):
        amt_spec.load_file(path_l)


_F64 = {}


def restated64(shape_name):
    if shape_name not in _F64:
        f0, f1 = frames_of(shape_name)
        with torch.no_grad():
            _F64[shape_name] = amt_g_restated.amt_g_forward(amt_g_restated.state_dict64(), f0.double(), f1.double(), NET_TS)
    return _F64[shape_name]


@pytest.mark.parametrize("shape_name", sorted(NET_SHAPES))
def test_forward_restatement_matches_the_reference(shape_name, golden_dir, sd_g, oracle_threads):
    """float64 and fp32, the reference's order of resize and convc1, <= 1e-3 per sampled pixel and line sum at both timesteps"""
    golden = np.load(os.path.join(golden_dir, "amt_g_net.npz"))
    f0, f1 = frames_of(shape_name)
    with torch.no_grad():
        out32 = amt_g_restated.amt_g_forward(sd_g, f0, f1, NET_TS)
    for out, kind in ((restated64(shape_name), "float64"), (out32, "fp32")):
        assert out.shape == (len(NET_TS), 3) + tuple(f0.shape[2:]) and torch.isfinite(out).all()
        for i, t in enumerate(NET_TS):
            d, sums_ok = cain_restated.compare(out[i].permute(1, 2, 0), golden, f"G_{shape_name}_t{t}_", NET_STRIDE, TOL)
            print(f"AMT-G {kind} restatement {shape_name} t={t}: max |d| vs the reference {d:.3e}")
            assert d <= TOL and sums_ok


@pytest.mark.parametrize("shape_name", sorted(NET_SHAPES))
def test_seeded_weights_make_every_block_visible(shape_name, golden_dir, oracle_threads):
    """The conditions on the stand-in weights at t = 0.5, by the goldens' record of the reference: the lookup moves the frame by >= 1e-2 on
    average, <= 5 % of the output values are clamped, and zeroing the two outputs of ANY of the five update blocks moves the frame by
    >= 5e-3 on average (a broken block cannot hide below the 1e-3 gate).  The two high blocks are checked again through the restatement."""
    golden = np.load(os.path.join(golden_dir, "amt_g_net.npz"))
    ce, sat = float(golden[f"G_{shape_name}_corr_effect_mean"]), float(golden[f"G_{shape_name}_saturated_frac"])
    effects = {b: float(golden[f"G_{shape_name}_block_effect_{b}"]) for b in UPDATE_BLOCKS}
    print(f"AMT-G {shape_name}: corr_effect_mean {ce:.4f}, saturated_frac {sat:.4%}, block effects {effects}")
    assert ce >= 1e-2 and sat <= 0.05 and all(e >= 5e-3 for e in effects.values())
    if shape_name != "128x128":
        return
    f0, f1 = frames_of(shape_name)
    full = restated64(shape_name)[0]
    sd = amt_g_restated.state_dict64()
    for blk in ("update3_high", "update2_high"):
        with torch.no_grad():
            blind = amt_g_restated.amt_g_forward(sd, f0.double(), f1.double(), [0.5], zero_block=blk)[0]
        eff = float((full - blind).abs().mean())
        print(f"AMT-G {shape_name}: {blk} zeroed through the restatement: {eff:.4f} (the reference: {effects[blk]:.4f})")
        assert abs(eff - effects[blk]) <= 1e-3 and eff >= 5e-3


@pytest.mark.parametrize("case", sorted(NODE_CASES))
def test_node_loop_matches_the_reference_node(case, golden_dir, monkeypatch, oracle_threads):
    golden = np.load(os.path.join(golden_dir, "amt_g_node.npz"))
    engine = amt_g_restated.RestatedAmtG()
    amt_g_restated.check_node_case(case, amt_g_restated.run_node(case, monkeypatch, engine), golden)
    _, n, _, _, _, m, skip = NODE_CASES[case]      # one forward per pair that has new frames, with all of that pair's timesteps
    assert engine.calls == [[k / m for k in range(1, m)] for i in range(n - 1) if not (skip and i in skip)]


def test_size_guard_of_g_comes_before_the_checkpoint_and_the_engine(monkeypatch, g_on):
    def no_engine(*a, **k):
        raise AssertionError("the size guard must come before the checkpoint and the engine")

    monkeypatch.setattr(amt, "load_file_from_direct_url", no_engine)
    monkeypatch.setattr(amt, "cached_engine", no_engine)
    # the widest activation of AMT-G has 88 floats per padded pixel; its byte offsets must stay below 2 GiB
    assert amt.MAX_PADDED_PIXELS_G == 6100805 and (amt.MAX_PADDED_PIXELS_G + 1) * 88 * 4 > 2 ** 31 - 1 >= amt.MAX_PADDED_PIXELS_G * 88 * 4
    amt.check_frame_size(1080, 1920, "G"), amt.check_frame_size(1440, 2560, "G"), amt.check_frame_size(2160, 3840, "L"), amt.check_frame_size(2160, 3840)
    with pytest.raises(ValueError, match="index arithmetic .6100805 pixels for AMT-G"):
        amt.check_frame_size(2160, 3840, "G")
    with pytest.raises(ValueError, match="for AMT-G"):
        cfi_amd.AMT_VFI().vfi("amt-g.pth", torch.zeros(1).expand(2, 2160, 3840, 3))
    with pytest.raises(ValueError, match="at least 128"):
        cfi_amd.AMT_VFI().vfi("amt-g.pth", torch.zeros(3, 100, 300, 3))
