"""CPU: the AMT checkpoint layout (cfi_amd.amt_spec): counts, strictness, telling S, L, G and foreign checkpoints apart, the
``{"state_dict": ...}`` wrapper of the real files, and the refusal of amt-g.pth before anything is loaded."""
import os

import numpy as np
import pytest
import torch

from cfi_amd import amt_spec, ifrnet_spec

SEED = 1


def test_tensor_and_parameter_counts():
    for variant, tensors, params in (("S", 213, 2990543), ("L", 207, 12935367)):
        shapes = amt_spec.amt_shapes(variant)
        assert len(shapes) == tensors
        assert sum(int(np.prod(s)) for s in shapes.values()) == params
    s, l = amt_spec.amt_shapes("S"), amt_spec.amt_shapes("L")
    assert s["comb_block.0.weight"] == (18, 9, 3, 3) and l["comb_block.0.weight"] == (30, 15, 7, 7)
    assert s["feat_encoder.conv2.weight"] == (84, 96, 1, 1) and l["feat_encoder.conv2.weight"] == (128, 128, 1, 1)
    assert s["update4.convc1.weight"] == (64, 392, 1, 1) and "update4.convc2.weight" not in s and l["update4.convc2.weight"] == (160, 256, 3, 3)
    assert s["encoder.pyramid1.0.0.weight"] == (20, 3, 3, 3) and l["encoder.pyramid1.0.0.weight"] == (48, 3, 7, 7)
    assert s["decoder1.convblock.2.weight"] == (60, 24, 4, 4) and l["decoder1.convblock.2.weight"] == (144, 40, 4, 4)
    assert not any("norm" in k for k in list(s) + list(l))      # InstanceNorm2d(affine=False) has no entries


def test_check_is_strict_and_tells_the_variants_apart():
    for variant in amt_spec.VARIANTS:
        sd = amt_spec.seeded_state_dict(variant, SEED)
        assert list(sd) == list(amt_spec.amt_shapes(variant)) and all(v.dtype == torch.float32 for v in sd.values())
        assert amt_spec.check_state_dict(sd) == variant
        other = "L" if variant == "S" else "S"
        with pytest.raises(RuntimeError, match=f"AMT-{variant} state dict where AMT-{other}"):
            amt_spec.check_state_dict(sd, other)
        truncated = dict(list(sd.items())[:-3])
        with pytest.raises(RuntimeError, match="not an AMT state dict|Missing key"):
            amt_spec.check_state_dict(truncated)
        missing = dict(sd)
        del missing["update3.gru.2.bias"]
        with pytest.raises(RuntimeError, match="Missing key"):
            amt_spec.check_state_dict(missing)
        with pytest.raises(RuntimeError, match="Unexpected key"):
            amt_spec.check_state_dict(dict(sd, extra=torch.zeros(1)))
        with pytest.raises(RuntimeError, match="size mismatch"):
            amt_spec.check_state_dict(dict(sd, **{"update2.convf1.weight": torch.zeros(8, 4, 7, 7)}))
    # AMT-G: its own update blocks, told apart by name
    g = dict(amt_spec.seeded_state_dict("L", SEED), **{"update3_high.convc1.weight": torch.zeros(256, 392, 1, 1)})
    with pytest.raises(NotImplementedError, match="AMT-G"):
        amt_spec.check_state_dict(g)
    # a foreign checkpoint (IFRNet shares the decoders' key names, not the encoders')
    foreign = {k: torch.zeros(s) for k, s in ifrnet_spec.ifrnet_shapes("L").items()}
    with pytest.raises(RuntimeError, match="not an AMT state dict"):
        amt_spec.check_state_dict(foreign)


def test_state_dict_wrapper_and_checkpoint_names(tmp_path):
    assert list(amt_spec.CKPT_VARIANT) == ["amt-s.pth", "amt-l.pth", "amt-g.pth", "gopro_amt-s.pth"]      # the reference's CKPT_CONFIGS order
    sd = amt_spec.seeded_state_dict("S", SEED)
    for name in ("amt-s.pth", "gopro_amt-s.pth"):
        path = os.path.join(tmp_path, name)
        torch.save({"state_dict": sd}, path)
        got, variant = amt_spec.load_file(path)
        assert variant == "S" and list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    path = os.path.join(tmp_path, "amt-l.pth")
    torch.save({"state_dict": sd}, path)          # an S file under L's name
    with pytest.raises(RuntimeError, match="AMT-S state dict where AMT-L"):
        amt_spec.load_file(path)
    torch.save(sd, path)                          # no wrapper
    with pytest.raises(RuntimeError, match="'state_dict' entry"):
        amt_spec.load_file(path)


def test_amt_g_is_refused_before_anything_is_loaded(tmp_path):
    with pytest.raises(NotImplementedError, match="amt-g.pth"):
        amt_spec.variant_of_ckpt("amt-g.pth")
    with pytest.raises(NotImplementedError, match="amt-g.pth"):
        amt_spec.load_file(os.path.join(tmp_path, "amt-g.pth"))      # the file does not exist: nothing was opened
    with pytest.raises(KeyError):
        amt_spec.variant_of_ckpt("amt-x.pth")
