"""CPU: the CAIN checkpoint layout (cfi_amd.cain_spec) and the torch restatement of its forward (tests/cain_restated.py) against the
reference's own outputs (tests/golden/cain_net.npz, tools/make_golden_cain.py)."""
import math
import os

import numpy as np
import pytest
import torch

import cain_restated
from cfi_amd import cain_spec


def test_key_table_counts():
    shapes = cain_spec.cain_shapes()
    assert len(shapes) == 494
    assert sum(math.prod(s) for s in shapes.values()) == 42780432
    assert shapes["encoder.interpolate.headConv.weight"] == (192, 384, 3, 3)
    assert shapes["encoder.interpolate.body.4.body.11.body.3.conv_du.0.weight"] == (12, 192, 1, 1)
    assert shapes["encoder.interpolate.body.4.body.12.conv.weight"] == (192, 192, 3, 3)


@pytest.fixture(scope="module")
def sd():
    return cain_restated.seeded_state_dict(1)


def test_loader_handles_wrapper_and_prefix(sd, tmp_path):
    p = tmp_path / "pretrained_cain.pth"
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}}, p)
    got = cain_spec.load_file(str(p))
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)


def test_missing_extra_or_misshapen_keys_raise(sd):
    bad = dict(sd)
    bad.pop("encoder.interpolate.tailConv.bias")
    with pytest.raises(RuntimeError, match="Missing key"):
        cain_spec.check_state_dict(bad)
    bad = dict(sd, extra=torch.zeros(1))
    with pytest.raises(RuntimeError, match="Unexpected key"):
        cain_spec.check_state_dict(bad)
    bad = dict(sd)
    bad["encoder.interpolate.headConv.bias"] = torch.zeros(191)
    with pytest.raises(RuntimeError, match="size mismatch"):
        cain_spec.check_state_dict(bad)
    cain_spec.check_state_dict(sd)


NET_SIZES = ((64, 96, 1), (100, 180, 2), (256, 448, 4))     # as tools/make_golden_cain.py
NODE_CASES = {"m2": (3, 3, 2, None), "m3": (2, 3, 3, None), "m5": (2, 3, 5, None), "m7": (2, 3, 7, None), "skip": (3, 3, 3, [1]),
              "rgba": (2, 4, 2, None)}


def test_restatement_matches_reference_golden(sd, golden_dir):
    g = np.load(os.path.join(golden_dir, "cain_net.npz"))
    assert int(g["seed"]) == 1
    for i, (h, w, stride) in enumerate(NET_SIZES):
        f = cain_restated.seeded_frames(2, h, w, 3, 100 + i).permute(0, 3, 1, 2).contiguous()
        keep = f.clone()
        with torch.no_grad():
            out = cain_restated.cain_forward(sd, f[0:1], f[1:2])[0].permute(1, 2, 0)
        assert torch.equal(f, keep)
        d, sums_ok = cain_restated.compare(out, g, f"{h}x{w}_", stride, 1e-6)
        assert d <= 1e-6 and sums_ok, (h, w, d)


def test_node_restatement_matches_reference_node_golden(sd, golden_dir):
    """the restated frame loop (cain_restated.node_frames) that the GPU node test compares every pixel against"""
    g = np.load(os.path.join(golden_dir, "cain_node.npz"))
    for name, (n, c, m, skip) in NODE_CASES.items():
        out = cain_restated.node_frames(sd, cain_restated.seeded_frames(n, 48, 72, c, 7), m, skip)
        assert tuple(out.shape) == tuple(g[name + "_shape"]), name
        d, sums_ok = cain_restated.compare(out, g, name + "_", 3, 1e-6)
        assert d <= 1e-6 and sums_ok, (name, d)
