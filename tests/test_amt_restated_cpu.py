"""CPU: the volume-free restatement of AMT (tests/amt_restated.py) against the reference's own outputs (tools/make_golden_amt.py).

Lookup (tests/golden/amt_lookup.npz): the float64 restatement against the reference's fp32 BidirCorrBlock, within
lookup_tolerance (gamma_lookup(D) * 2^-24 * M + 2^-23 C) + coord_slack * C (amt_restated's docstring derives both; the reference's own fp32 summation of D products,
its pooling of the volume and its bilinear blend make at most as many roundings per term as gamma_lookup counts).

Forward (tests/golden/amt_net.npz): per-pixel |d| <= 1e-3, the project's gate, S and L at 128x128, 144x208 and 130x200, t = 0.5 and 0.2;
the restatement runs in float64 (the reference in fp32 differs from itself in float64 by less than 1e-6 at these shapes).  Maxima measured
here are recorded in docs/design/amt.md."""
import os

import numpy as np
import pytest
import torch

import amt_restated
import cain_restated
from cfi_amd import amt_spec

from amt_restated import NET_SHAPES, NET_STRIDE, NET_TS, SEED, TOL, frames_of, state_dict64


def lookup_bound(name, which):
    """(want, tol, M, mn) of one direction of a golden lookup case in float64, all [196,h,w]; tol is the kernel bound (no coordinate slack)"""
    f0, f1, c0, c1 = amt_restated.lookup_case(name)
    fq, ft, c = (f0, f1, c0) if which == 0 else (f1, f0, c1)
    want, M, Cn, mn = amt_restated.lookup(fq.double(), ft.double(), c.double(), bound=True)
    return want, amt_restated.lookup_tolerance(fq.shape[0], M, Cn), M, Cn, mn, c


@pytest.mark.parametrize("name", sorted(amt_restated.LOOKUP_CASES))
def test_lookup_restatement_matches_the_reference(name, golden_dir):
    golden = np.load(os.path.join(golden_dir, "amt_lookup.npz"))
    h, w, D, _ = amt_restated.LOOKUP_CASES[name]
    iy, ix = cain_restated.sample_index(h, amt_restated.LOOKUP_STRIDE), cain_restated.sample_index(w, amt_restated.LOOKUP_STRIDE)
    for which in (0, 1):
        want, tol, M, Cn, mn, c = lookup_bound(name, which)
        ref = torch.from_numpy(golden[f"{name}_out{which}"]).double()
        # the reference's sampling position: per level the coordinate magnitude |c| / 2^lvl and the level's size
        slack = torch.zeros_like(want)
        for lvl in range(amt_restated.LEVELS):
            s = amt_restated.coord_slack(c.abs().amax(0) / 2 ** lvl, max(h >> lvl, w >> lvl))
            slack[lvl * 49:(lvl + 1) * 49] = s[None] * 2           # x and y
        tol = tol + slack * Cn
        sub = lambda v: v[:, iy][:, :, ix]          # noqa: E731
        err = (sub(want) - ref).abs()
        print(f"{name} direction {which}: max |d| {float(err.max()):.3e}, max d / tol {float((err / sub(tol).clamp_min(1e-30)).max()):.3f}, "
              f"max |out| {float(ref.abs().max()):.3f}")
        assert ref.shape == sub(want).shape and (err <= sub(tol)).all()
        # the cases do what they are for: windows off every side, all-zero windows, integer positions, a non-trivial signal
        assert (want == 0).all(0).any() and (c[0] < 0).any() and (c[0] > w - 1).any() and (c[1] < 0).any() and (c[1] > h - 1).any()
        assert (c == torch.round(c)).all(0).any() and float(want.abs().max()) > 1


@pytest.mark.parametrize("variant", amt_spec.VARIANTS)
@pytest.mark.parametrize("shape_name", sorted(NET_SHAPES))
def test_forward_restatement_matches_the_reference(variant, shape_name, golden_dir):
    golden = np.load(os.path.join(golden_dir, "amt_net.npz"))
    f0, f1 = frames_of(shape_name)
    with torch.no_grad():
        out = amt_restated.amt_forward(state_dict64(variant), variant, f0.double(), f1.double(), NET_TS)
    assert out.shape == (2, 3) + tuple(f0.shape[2:])
    for i, t in enumerate(NET_TS):
        d, sums_ok = cain_restated.compare(out[i].permute(1, 2, 0), golden, f"{variant}_{shape_name}_t{t}_", NET_STRIDE, TOL)
        print(f"AMT-{variant} {shape_name} t={t}: max |d| vs the reference {d:.3e}")
        assert d <= TOL and sums_ok


@pytest.mark.parametrize("variant", amt_spec.VARIANTS)
def test_seeded_weights_make_the_lookup_visible(variant, golden_dir):
    """The two conditions on the stand-in weights: the lookup moves the frame by >= 1e-2 on average, and <= 5 % of the output values are
    clamped — by the goldens' record of the reference, and again through the restatement."""
    golden = np.load(os.path.join(golden_dir, "amt_net.npz"))
    for shape_name in NET_SHAPES:
        assert float(golden[f"{variant}_{shape_name}_corr_effect_mean"]) >= 1e-2
        assert float(golden[f"{variant}_{shape_name}_saturated_frac"]) <= 0.05
    f0, f1 = frames_of("128x128")
    sd = amt_spec.seeded_state_dict(variant, SEED)
    with torch.no_grad():
        out = amt_restated.amt_forward(sd, variant, f0, f1, [0.5])
        blind = amt_restated.amt_forward(sd, variant, f0, f1, [0.5], zero_lookup=True)
    effect, sat = float((out - blind).abs().mean()), float(((out <= 0) | (out >= 1)).float().mean())
    print(f"AMT-{variant}: corr_effect_mean {effect:.4f}, saturated_frac {sat:.4f}")
    assert effect >= 1e-2 and sat <= 0.05
    assert abs(effect - float(golden[f"{variant}_128x128_corr_effect_mean"])) < 1e-3


def test_size_guard_and_padding():
    assert amt_restated.pad16(130, 200) == (4, 4, 7, 7) and amt_restated.pad16(1080, 1920) == (0, 0, 4, 4)
    f = torch.zeros(1, 3, 100, 300)
    with pytest.raises(ValueError, match="at least 128"):
        amt_restated.amt_forward({}, "S", f, f, [0.5])
