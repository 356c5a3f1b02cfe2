"""CPU: the torch restatement of ATM-lite (tests/atm_restated.py) against the reference's own outputs (tools/make_golden_atm.py), and the
conditions on the seeded weights that make those outputs worth comparing against.

Restatement vs goldens (atm_attn.npz: both windowed blocks on the eight token maps; atm_net.npz: the forward at 64x64, 128x192, 192x320, both
global-motion modes), in float32: the project's golden_tol convention — 0 on the host that wrote the goldens (the restatement runs the
reference's operations in the reference's order and memory layouts, so it reproduces its bits), 2e-4 elsewhere.

Liveliness: with default initialisation the network is dead (final flows 0.05 px, motion read-out effect 2e-8), and a whole-network test
would pass with a broken motion kernel.  At every golden shape, in both modes: zeroing the ATM blocks' motion read-out moves the float64
frame by >= 1e-3 on average, the largest final flow is >= 0.5 px, <= 10 % of the output is clamped, and float32 and float64 differ by <=
1e-4 at every pixel (a tenfold margin below the 1e-3 gate).  Conditions on the inputs, not measurements of the code under test.
Measured here (On / Off): effect 1.0e-2 .. 2.9e-2 / 1.1e-3 .. 1.6e-3, flows 0.99 .. 1.10 / 0.82 .. 0.98 px, clamped <= 4.7 % / <= 0.6 %."""
import os

import numpy as np
import pytest
import torch

import atm_restated as R
import cain_restated
from oracle import golden_stats


@pytest.fixture(scope="module")
def tol(golden_dir):
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))      # as the golden writer
    return golden_stats.golden_tol(os.path.join(golden_dir, "atm_host.json"))


@pytest.mark.parametrize("cross", [True, False], ids=["cross", "self"])
@pytest.mark.parametrize("name", sorted(R.ATTN_CASES))
def test_block_restatement_matches_the_reference(name, cross, golden_dir, tol):
    golden = np.load(os.path.join(golden_dir, "atm_attn.npz"))
    h, w, win, shift = R.ATTN_CASES[name]
    p, x = R.attn_case(name, cross)
    with torch.no_grad():
        y, mot = R.window_block(p, x, win, shift, cross)
    kind = "cross" if cross else "self"
    d = float((y[..., ::R.ATTN_CH_STRIDE] - torch.from_numpy(golden[f"{name}_{kind}_x"])).abs().max())
    dm = float((mot - torch.from_numpy(golden[f"{name}_{kind}_motion"])).abs().max()) if cross else 0.0
    print(f"{name} {kind}: max |d| {d:.3e}, motion {dm:.3e} (tolerance {tol:g})")
    assert d <= tol and dm <= tol
    if cross:      # the case does what it is for: a read-out of pixels, not of rounding noise
        assert float(mot.abs().max()) > 1.0


@pytest.mark.parametrize("mode", sorted(R.MODES))
@pytest.mark.parametrize("shape_name", sorted(R.NET_SHAPES))
def test_forward_restatement_matches_the_reference(shape_name, mode, golden_dir, tol):
    golden = np.load(os.path.join(golden_dir, "atm_net.npz"))
    f0, f1 = R.frames_of(shape_name)
    with torch.no_grad():
        out = R.atm_forward(R.state_dict_as(torch.float32), f0, f1, R.MODES[mode])
    key = f"{shape_name}_{'on' if R.MODES[mode] else 'off'}_"
    d, _ = cain_restated.compare(out[0].permute(1, 2, 0), golden, key, R.NET_STRIDE, tol)
    got = cain_restated.summary(out[0].permute(1, 2, 0), R.NET_STRIDE)
    rows = float(abs(got["rows"] - golden[key + "rows"]).max()) / out.shape[3]
    cols = float(abs(got["cols"] - golden[key + "cols"]).max()) / out.shape[2]
    print(f"ATM-lite {shape_name} {mode}: max |d| vs the reference {d:.3e}, row / column means {rows:.3e} / {cols:.3e} (tolerance {tol:g})")
    assert d <= tol and rows <= tol + 1e-9 and cols <= tol + 1e-9      # (1e-9: float32 frames summed in float64 by two routes)


@pytest.mark.parametrize("mode", sorted(R.MODES))
@pytest.mark.parametrize("shape_name", sorted(R.NET_SHAPES))
def test_seeded_weights_exercise_the_motion_path(shape_name, mode, golden_dir):
    golden = np.load(os.path.join(golden_dir, "atm_net.npz"))
    gm = R.MODES[mode]
    key = f"{shape_name}_{'on' if gm else 'off'}_"
    # the reference's own record
    assert float(golden[key + "motion_effect_mean"]) >= 1e-3 and float(golden[key + "max_flow"]) >= 0.5 and float(golden[key + "clamped_frac"]) <= 0.10
    f0, f1 = R.frames_of(shape_name)
    sd64, taps = R.state_dict_as(torch.float64), {}
    with torch.no_grad():
        out = R.atm_forward(sd64, f0.double(), f1.double(), gm, taps=taps)
        dark = R.atm_forward(sd64, f0.double(), f1.double(), gm, zero_motion=True)
        out32 = R.atm_forward(R.state_dict_as(torch.float32), f0, f1, gm)
    effect = float((out - dark).abs().mean())
    flow = float(max(taps["flow0"].abs().max(), taps["flow1"].abs().max()))
    clamped = float(((out <= 0) | (out >= 1)).double().mean())
    d32 = float((out32.double() - out).abs().max())
    print(f"{shape_name} {mode}: motion effect {effect:.3e}, largest flow {flow:.3f} px, clamped {clamped:.4f}, float32 vs float64 {d32:.3e}")
    assert effect >= 1e-3
    assert flow >= 0.5
    assert clamped <= 0.10
    assert d32 <= 1e-4


def test_region_labels_reproduce_the_pad_and_shift_quirk():
    """8x12 tokens, window 12, shift 6: rows padded 2 / 2.  The pad labels are taken at the ROLLED position: rolled rows 0..1 carry the label of
    padding although they hold map rows 4..5, and rolled rows 4..5, which hold the bottom padding, carry the label of the map."""
    lab = R.region_labels(12, 12, 8, 12, 12, 6)
    pad_part = lab // 9
    assert pad_part[0, 0] != pad_part[2, 0] and pad_part[2, 0] == pad_part[5, 0] and pad_part[9, 0] != pad_part[10, 0]
    assert len(torch.unique(lab % 9)) == 4 and len(torch.unique(R.region_labels(8, 8, 8, 8, 8, 4))) == 4
    assert int(R.region_labels(16, 24, 16, 24, 8, 0).max()) == 0
    assert R.pad64(100, 180) == (14, 14, 6, 6) and R.pad64(64, 64) == (0, 0, 0, 0)
