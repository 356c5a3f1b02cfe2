"""CPU: FLAVR's checkpoint layout (cfi_amd.flavr_spec) and the torch restatement of its forward (tests/flavr_restated.py), pinned to the
reference's own outputs in tests/golden/flavr_net.npz (tools/make_golden_flavr.py) at every golden size."""
import os

import numpy as np
import pytest
import torch

import cain_restated
import flavr_restated
from cfi_amd import flavr_spec

SEED = 1
# name -> (n_outputs, h, w, sample stride, frame seed): tools/make_golden_flavr.py NET_CASES
NET_CASES = {"o1_64x96": (1, 64, 96, 1, 300), "o1_50x70": (1, 50, 70, 1, 301), "o1_101x179": (1, 101, 179, 2, 302),
             "o3_64x96": (3, 64, 96, 1, 303)}


def window(h, w, seed):
    f = cain_restated.seeded_frames(4, h, w, 3, seed).permute(0, 3, 1, 2).contiguous()
    return [f[i:i + 1] for i in range(4)]


def test_tensor_and_parameter_counts():
    for n_outputs, tensors, params in ((1, 59, 42061571), (3, 76, 42084297)):
        shapes = flavr_spec.flavr_shapes(n_outputs)
        assert len(shapes) == tensors
        assert sum(int(np.prod(s)) for s in shapes.values()) == params
    # 4x and 8x differ in outconv only
    a, b = flavr_spec.flavr_shapes(3), flavr_spec.flavr_shapes(7)
    assert list(a) == list(b) and [k for k in a if a[k] != b[k]] == ["outconv.1.weight", "outconv.1.bias"]
    assert "encoder.stem.0.bias" not in flavr_spec.flavr_shapes(1) and "encoder.stem.0.bias" in a
    assert not any("downsample.0.bias" in k for k in a)


def test_check_is_strict():
    for n_outputs in (1, 3):
        sd = flavr_spec.seeded_state_dict(SEED, n_outputs)
        flavr_spec.check_state_dict(sd)
        assert flavr_spec.n_outputs_of(sd) == n_outputs
        missing = dict(sd)
        del missing["decoder.1.upconv.1.attn_layer.0.bias"]
        with pytest.raises(RuntimeError, match="Missing key"):
            flavr_spec.check_state_dict(missing)
        with pytest.raises(RuntimeError, match="Unexpected key"):
            flavr_spec.check_state_dict(dict(sd, extra=torch.zeros(1)))
        with pytest.raises(RuntimeError, match="size mismatch"):
            flavr_spec.check_state_dict(dict(sd, **{"feature_fuse.conv.0.weight": torch.zeros(64, 256, 3, 3)}))
    # a 2x file with encoder biases is not a 2x model
    with pytest.raises(RuntimeError, match="Unexpected key"):
        flavr_spec.check_state_dict(dict(flavr_spec.seeded_state_dict(SEED, 1), **{"encoder.stem.0.bias": torch.zeros(64)}))


def test_module_prefix_handling(tmp_path):
    sd = flavr_spec.seeded_state_dict(SEED, 1)
    path = os.path.join(tmp_path, "FLAVR_2x.pth")
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}}, path)
    got = flavr_spec.load_file(path)
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    torch.save({"state_dict": sd}, path)      # no prefix: the reference's partition() turns every key into "" and the load fails
    with pytest.raises(RuntimeError, match="module."):
        flavr_spec.load_file(path)
    torch.save(sd, path)                      # no wrapper
    with pytest.raises(KeyError):
        flavr_spec.load_file(path)


@pytest.mark.parametrize("name", sorted(NET_CASES))
def test_restatement_matches_the_reference(name, golden_dir):
    n_outputs, h, w, stride, fseed = NET_CASES[name]
    golden = np.load(os.path.join(golden_dir, "flavr_net.npz"))
    assert int(golden["seed"]) == SEED
    with torch.no_grad():
        out = flavr_restated.flavr_forward(flavr_spec.seeded_state_dict(SEED, n_outputs), window(h, w, fseed))[0].permute(1, 2, 0)
    assert tuple(out.shape) == (h, w, 3)
    d, sums_ok = cain_restated.compare(out, golden, name + "_", stride, 1e-3)
    assert d <= 1e-3 and sums_ok, (name, d, sums_ok)


def test_seeded_weights_make_the_network_visible():
    """out - window mean must be large against the 1e-3 gate: std >= 0.05 at 64x96 (PyTorch's default initialisation gives 0.010)"""
    for n_outputs in (1, 3):
        fr = window(64, 96, 300)
        with torch.no_grad():
            out = flavr_restated.flavr_forward(flavr_spec.seeded_state_dict(SEED, n_outputs), fr)
        mean = torch.stack(fr, 2).mean((2, 3, 4))[:, :, None, None]
        std = float((out - mean).std())
        print("n_outputs", n_outputs, "std(out - mean)", std)
        assert std >= 0.05, std


def test_frame_order_is_visible():
    """swapping frames 0 and 3 of the window changes the output by more than 1e-2 somewhere: a mis-wired time slice cannot pass the gate"""
    sd = flavr_spec.seeded_state_dict(SEED, 1)
    fr = window(64, 96, 300)
    with torch.no_grad():
        a = flavr_restated.flavr_forward(sd, fr)
        b = flavr_restated.flavr_forward(sd, [fr[3], fr[1], fr[2], fr[0]])
    d = float((a - b).abs().max())
    print("max |swap difference|", d)
    assert d > 1e-2, d


def test_padding_rule():
    assert flavr_restated.pad16(64, 96) == (0, 0, 0, 0)
    assert flavr_restated.pad16(50, 70) == (5, 5, 7, 7)
    assert flavr_restated.pad16(101, 179) == (6, 7, 5, 6)
    assert flavr_restated.pad16(1080, 1920) == (0, 0, 4, 4)
