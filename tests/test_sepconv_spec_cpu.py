"""CPU: the SepConv++ checkpoint layout (cfi_amd.sepconv_spec), its loader and seeded weights, and the torch restatement of its forward
(tests/sepconv_restated.py) against the reference's own outputs (tests/golden/sepconv_net.npz / sepconv_node.npz,
tools/make_golden_sepconv.py)."""
import math
import os

import numpy as np
import pytest
import torch

import cain_restated
import sepconv_restated
from cfi_amd import sepconv_spec


def test_key_table_counts():
    shapes = sepconv_spec.sepconv_shapes()
    assert len(shapes) == 88
    assert sum(math.prod(s) for s in shapes.values()) == 13560102
    assert list(shapes)[:3] == ["netInput.weight", "netInput.bias", "netEncode.0.netVer.1.netMain.0.weight"]
    assert shapes["netDecode.0.netVer.1.netMain.2.weight"] == (256, 512, 3, 3)
    assert shapes["netDecode.0.netHor.0.netMain.1.weight"] == (512, 512, 3, 3)      # netHor.i = row 4 - i
    assert shapes["netDecode.0.netHor.3.netMain.3.weight"] == (64, 64, 3, 3)
    assert shapes["netEncode.0.netVer.4.netMain.1.weight"] == (512, 256, 3, 3)
    assert shapes["netHortwo.netMain.3.weight"] == (51, 64, 3, 3)
    assert "netDecode.0.netHor.4.netMain.0.weight" not in shapes and "netDecode.0.netVer.0.netMain.0.weight" not in shapes
    assert sum(1 for s in shapes.values() if s == (1,)) == 8 + 8 + 6 + 4       # one scalar slope per PReLU


@pytest.fixture(scope="module")
def sd():
    return sepconv_spec.seeded_state_dict(1)


def test_seeded_slopes_are_distinct(sd):
    slopes = [float(v) for k, v in sd.items() if v.shape == (1,)]
    assert len(set(slopes)) == len(slopes) and 0.09 < min(slopes) and max(slopes) < 0.4


def test_loader_reads_a_plain_state_dict(sd, tmp_path):
    p = tmp_path / "sepconv.pth"
    torch.save(sd, p)
    got = sepconv_spec.load_file(str(p))
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)


def test_missing_extra_or_misshapen_keys_raise(sd, tmp_path):
    bad = dict(sd)
    bad.pop("netHortwo.netMain.3.bias")
    with pytest.raises(RuntimeError, match="Missing key"):
        sepconv_spec.check_state_dict(bad)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        sepconv_spec.check_state_dict({"module." + k: v for k, v in sd.items()})     # no DataParallel prefix in the real file
    bad = dict(sd)
    bad["netInput.bias"] = torch.zeros(17)
    with pytest.raises(RuntimeError, match="size mismatch"):
        sepconv_spec.check_state_dict(bad)
    sepconv_spec.check_state_dict(sd)


NET_SIZES = ((64, 96, 1), (90, 160, 2), (101, 179, 2), (24, 40, 1))     # as tools/make_golden_sepconv.py
NODE_CASES = {"m2": (3, 3, 2, None), "m3": (2, 3, 3, None), "m5": (2, 3, 5, None), "skip": (3, 3, 3, [1]), "rgba": (2, 4, 2, None)}


def test_restatement_matches_reference_golden(sd, golden_dir):
    g = np.load(os.path.join(golden_dir, "sepconv_net.npz"))
    assert int(g["seed"]) == 1
    for i, (h, w, stride) in enumerate(NET_SIZES):
        f = cain_restated.seeded_frames(2, h, w, 3, 200 + i).permute(0, 3, 1, 2).contiguous()
        keep = f.clone()
        out, min_n = sepconv_restated.sepconv_forward(sd, f[0:1], f[1:2], min_norm=True)
        assert torch.equal(f, keep)
        # the 0.01 threshold decides no golden pixel: a restatement without it gives the same output
        assert min_n >= 0.05, (h, w, min_n)
        d, sums_ok = cain_restated.compare(out[0].permute(1, 2, 0), g, f"{h}x{w}_", stride, 1e-6)
        assert d <= 1e-6 and sums_ok, (h, w, d)


def test_levels_of_the_golden_sizes():
    """the cases the golden sizes were chosen for: odd rows at 90x160, both odd dimensions at 101x179, 2..3-pixel levels at 24x40"""
    def levels(h, w):
        h, w = h + h % 2, w + w % 2
        out = [(h, w)]
        for _ in range(4):
            h, w = (h + 1) // 2, (w + 1) // 2
            out.append((h, w))
        return out

    assert levels(64, 96)[4] == (4, 6) and all(a % 2 == 0 and b % 2 == 0 for a, b in levels(64, 96)[:4])
    assert [h for h, _ in levels(90, 160)] == [90, 45, 23, 12, 6]
    assert levels(101, 179) == [(102, 180), (51, 90), (26, 45), (13, 23), (7, 12)]
    assert levels(24, 40)[3:] == [(3, 5), (2, 3)]
    assert levels(1080, 1920)[3:] == [(135, 240), (68, 120)]


def test_node_restatement_matches_reference_node_golden(sd, golden_dir):
    """the restated frame loop (sepconv_restated.node_frames) that the GPU node test compares every pixel against"""
    g = np.load(os.path.join(golden_dir, "sepconv_node.npz"))
    assert int(g["seed"]) == 1
    for name, (n, c, m, skip) in NODE_CASES.items():
        out = sepconv_restated.node_frames(sd, cain_restated.seeded_frames(n, 48, 72, c, 9), m, skip)
        assert tuple(out.shape) == tuple(g[name + "_shape"]), name
        d, sums_ok = cain_restated.compare(out, g, name + "_", 3, 1e-6)
        assert d <= 1e-6 and sums_ok, (name, d)
