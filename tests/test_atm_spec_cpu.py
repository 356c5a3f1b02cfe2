"""CPU: the checkpoint layout of ATM-lite (cfi_amd.atm_spec) against the reference's own state dict as tools/make_golden_atm.py recorded it
in tests/golden/atm_net.npz, the refusals (a relative_coord table the kernel does not compute, ATM-base by name and by shape), the real
file's form, and the frame-size limit on the host side of the call."""
import os

import numpy as np
import pytest
import torch

from cfi_amd import atm, atm_spec


def test_shapes_match_the_reference_state_dict(golden_dir):
    golden = np.load(os.path.join(golden_dir, "atm_net.npz"))
    want = atm_spec.atm_shapes()
    assert list(want) == [str(k) for k in golden["sd_names"]]
    assert [",".join(map(str, v)) for v in want.values()] == [str(s) for s in golden["sd_shapes"]]
    assert len(want) == atm_spec.N_TENSORS == 236
    params = sum(int(np.prod(v)) for k, v in want.items() if not k.endswith(".relative_coord"))
    assert params == int(golden["n_parameters"]) == atm_spec.N_PARAMETERS == 11975523
    assert len(atm_spec.weight_shapes()) == 232 and not any("relative_coord" in k for k in atm_spec.weight_shapes())
    coords = [v for k, v in want.items() if k.endswith(".relative_coord")]
    assert coords == [(1, 1, 2, 64, 64)] * 2 + [(1, 1, 2, 144, 144)] * 2


def test_relative_coord_is_key_minus_query():
    rc = atm_spec.relative_coord(12)
    assert rc.shape == (1, 1, 2, 144, 144)
    q, k = 3 * 12 + 5, 7 * 12 + 1          # query (x 5, y 3), key (x 1, y 7)
    assert rc[0, 0, 0, q, k] == -4 and rc[0, 0, 1, q, k] == 4 and float(rc[0, 0, :, q, q].abs().max()) == 0


def test_seeded_state_dict_loads_and_a_wrong_relative_coord_is_refused():
    sd = atm_spec.seeded_state_dict(3)
    atm_spec.check_state_dict(sd)
    assert list(sd) == list(atm_spec.atm_shapes())
    bad = dict(sd)
    bad["global_motion_atmformer.1.attn.relative_coord"] = -sd["global_motion_atmformer.1.attn.relative_coord"]
    with pytest.raises(RuntimeError, match="relative_coord.*computes"):
        atm_spec.check_state_dict(bad)
    short = dict(sd)
    del short["proj.1.weight"]
    with pytest.raises(RuntimeError, match="Missing key"):
        atm_spec.check_state_dict(short)
    wide = dict(sd)
    wide["feat_extracts.0.0.0.weight"] = torch.zeros(32, 3, 3, 3)
    with pytest.raises(NotImplementedError, match="ATM-base is not"):
        atm_spec.check_state_dict(wide)


def test_load_file_takes_the_real_form_and_drops_cached_masks(tmp_path):
    sd = atm_spec.seeded_state_dict(4)
    blob = dict(sd)
    blob["local_motion_atmformer.1.attn_mask"] = torch.zeros(4, 64, 64)
    blob["local_motion_atmformer.1.HW"] = torch.tensor([1024.0])
    path = str(tmp_path / "atm-vfi-lite.pt")
    torch.save({"model_state_dict": blob}, path)
    got = atm_spec.load_file(path)
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    torch.save(blob, path)
    with pytest.raises(RuntimeError, match="model_state_dict"):
        atm_spec.load_file(path)
    bad = dict(blob)
    bad["local_motion_atmformer.0.attn.relative_coord"] = sd["local_motion_atmformer.0.attn.relative_coord"].transpose(-1, -2).contiguous()
    torch.save({"model_state_dict": bad}, path)
    with pytest.raises(RuntimeError, match="relative_coord"):
        atm_spec.load_file(path)


@pytest.mark.parametrize("ckpt", ["atm-vfi-base.pt", "atm-vfi-base-pct.pt"])
def test_base_checkpoints_are_refused_by_name(ckpt, tmp_path):
    with pytest.raises(NotImplementedError, match=ckpt.replace(".", r"\.") + ".*ATM-base is not built yet"):
        atm_spec.check_ckpt_name(ckpt)
    with pytest.raises(NotImplementedError, match="ATM-base is not built yet"):
        atm_spec.load_file(str(tmp_path / ckpt))       # before the file is opened
    with pytest.raises(KeyError):
        atm_spec.check_ckpt_name("atm.pt")


def test_frame_size_limit_is_the_librarys(hip_lib):
    """The limit comes from the widest per-image buffer (80 floats per padded pixel, 32-bit byte offsets): the Python guard and the
    library's own figure agree, and the guard is on the host side of the call."""
    assert atm.MAX_PADDED_PIXELS == hip_lib.vfi_atm_max_padded_pixels() == (2 ** 31 - 1) // 320
    assert atm.padded_size(100, 180) == (128, 192) and atm.padded_size(1080, 1920) == (1088, 1920) and atm.padded_size(64, 64) == (64, 64)
    atm.check_frame_size(1080, 1920), atm.check_frame_size(1440, 2560)
    with pytest.raises(ValueError, match="index arithmetic"):
        atm.check_frame_size(2160, 3840)
    assert 2176 * 3840 > atm.MAX_PADDED_PIXELS >= 1472 * 2560
