"""CPU: tests/rife_stage_restated.py tied to the ORACLE, not to the kernels, and its tables checked without a device.

  * A float64 forward of RIFE 4.7 / 4.17 / 4.26 whose glue (block inputs, flow / mask / carried-feature update, fractional block scales,
    final blend) is the restated ops and whose trunks are the oracle's own convolutions agrees with oracle/rife_oracle.py's
    ifnet47_forward / ifnet426_forward in float64 to 1e-11, on every block's flow and on the frame, for the scale lists [8, 4, 2, 1],
    [16, 8, 4, 2] and [4, 2, 1, 0.5] (4.26: each behind a fifth, leading block at twice the first scale as the node builds them, 16 at most:
    the lists its oracle accepts at 64 x 128).
  * Every case of the tables on a perfect device (the float64 result rounded to fp32): every bound is finite, positive where the op is
    not declared exact, and the summand conditions mn > tol hold — compare() asserts them before it looks at a result.
  * Every deliberately wrong restatement differs from the right one by more than the bound on at least 1 % of the elements (those not declared exact)
    of one of the case's outputs, in every case it applies to: the device run (tests/test_gpu_rife_stage.py) can see it."""
import pytest
import torch

import rife_stage_restated as rs
from cfi_amd import synth
from oracle import rife_oracle


def _restated_forward(sd, img0, img1, ts, scales, arch):
    nx = arch == "4.26"
    enc = rife_oracle.encode if arch == "4.7" else rife_oracle.encode417
    cl = lambda x: x.permute(0, 2, 3, 1)
    pk0, pk1 = torch.cat([cl(img0), cl(enc(sd, img0))], -1), torch.cat([cl(img1), cl(enc(sd, img1))], -1)
    nf4 = pk0.shape[-1] - 3
    F = M = FEAT = None
    flows = []
    for i, sc in enumerate(scales):
        s, u = (int(sc), 1) if sc >= 1 else (1, int(round(1 / sc)))
        z = lambda q: None if q is None else torch.zeros_like(q)
        nch = 7 + 2 * nf4 + (0 if F is None else 5 + (8 if nx else 0))
        x = rs.stage_x(pk0, pk1, ts, F, M, z(M), FEAT, z(FEAT), s, nch)[0]
        if u > 1:          # IFBlock's own up-resize of its input and down-resize of its output (planar4_up / t_down)
            x = rs.up(x, u)[0]
            x[..., -4:] *= u
        T = cl(torch.cat(rife_oracle.ifblock(sd, f"block{i}.", x.permute(0, 3, 1, 2), None, 1.0, with_feat=nx), 1))
        if u > 1:
            T = rs.resize(T, T.shape[1] // u, T.shape[2] // u)[0]
            T[..., :4] /= u
        F = rs.flow_update(F, T[..., 0:4], s)[0]
        M = rs.up(T[..., 4:5], s)[0]
        FEAT = rs.up(T[..., 5:13], s)[0] if nx else None
        flows.append(F)
    a, b = rs.warp(pk0[..., :3], F[..., 0:2])[0], rs.warp(pk1[..., :3], F[..., 2:4])[0]
    return rs.blend(a, 0.0, b, 0.0, M, 0.0)[0], flows


@pytest.mark.parametrize("arch", ["4.7", "4.17", "4.26"])
@pytest.mark.parametrize("scales", [(8, 4, 2, 1), (16, 8, 4, 2), (4, 2, 1, 0.5)], ids=lambda s: "-".join(str(v) for v in s))
def test_restated_glue_matches_the_oracle_in_float64(arch, scales):
    sd = {"4.7": synth.rife47_synth_state_dict, "4.17": synth.rife417_synth_state_dict, "4.26": synth.rife426_synth_state_dict}[arch](4321)
    sd = {k: v.double() for k, v in sd.items()}
    if arch == "4.26":
        scales = (min(2 * scales[0], 16),) + scales      # 64 x 128 at block scale 32 is below the two stride-2 convolutions: the oracle refuses it
    fr = synth.noise_frames(4, 64, 128, seed=3).double().permute(0, 3, 1, 2)
    img0, img1, ts = fr[0:2], fr[2:4], torch.tensor([0.3, 0.75])
    before = torch.get_default_dtype()
    try:      # the oracle's warp builds (and caches) its grid in the default dtype
        torch.set_default_dtype(torch.float64)
        rife_oracle._grid_cache.clear()
        with torch.inference_mode():
            want, aux = rife_oracle.ifnet47_forward(sd, img0, img1, ts.double().view(-1, 1, 1, 1), [float(s) for s in scales], return_aux=True, arch=arch)
            got, flows = _restated_forward(sd, img0, img1, ts.double(), scales, arch)
    finally:
        torch.set_default_dtype(before)
        rife_oracle._grid_cache.clear()
    for i, (f, a) in enumerate(zip(flows, aux)):
        err = (f - a[0].permute(0, 2, 3, 1)).abs().max().item()
        assert err <= 1e-11, f"flow after block {i}: {err:.3e}"
    err = (got - want.permute(0, 2, 3, 1)).abs().max().item()
    assert err <= 1e-11, f"frame: {err:.3e}"
    assert float(flows[-1].abs().max()) > 0.1 and float(got.std()) > 0.01, "a trivial forward proves nothing"


EXACT_OPS = {"stage_in0_staged"}


@pytest.mark.parametrize("case", rs.ALL_CASES, ids=lambda c: c.id)
def test_table_case_on_a_perfect_device(case):
    """bounds finite and positive, mn > tol, and every applicable wrong restatement visible on >= 1 % of an output's elements"""
    run = rs.emulate(case)
    right = rs.expectations(run)
    positive = 0.0
    for e in right:
        if e["tol"] is None:
            assert case.op in EXACT_OPS
            continue
        tol = e["tol"]
        assert bool(torch.isfinite(tol).all()) and bool((tol >= 0).all()), f"{case.id}:{e['buf']}: a bound is not finite"
        positive = max(positive, float((tol > 0).double().mean()))
    # zero bounds are the declared-exact elements: copies (scale 1), the timestep, padding channels, Fdbg outside H x W
    copy = case.op in ("flow_up", "feat_up", "stage_in") and case.p["s"] == 1 and not case.p.get("has_prev") and not case.p.get("has_flow")
    assert positive > 0.05 or case.op in EXACT_OPS or copy, f"{case.id}: hardly any positive bound"
    assert rs.check(case, run) <= 1.0
    for mut in rs.MUTATIONS:
        if not rs.applies(mut, case):
            continue
        share = 0.0
        for e, r in zip(rs.expectations(run, mut), right):
            tol = torch.zeros_like(r["want"]) if r["tol"] is None else r["tol"].reshape(r["want"].shape)
            moved = ((e["want"].reshape(r["want"].shape) - r["want"]).abs() > tol).sum().item()
            share = max(share, moved / max(1, int((tol > 0).sum()) or tol.numel()))      # of the elements that are not declared exact
        assert share >= 0.01, f"{case.id}: '{rs.MUTATIONS[mut]}' moves only {share:.2%} of the elements by more than the bound"
        with pytest.raises(AssertionError, match="outside the bound|differ from the exact result"):
            rs.check(case, run, mut)


def test_every_launcher_and_mutation_has_cases():
    assert set(rs.TABLES) == {"stage_in", "stage_in0_staged", "flow_up", "feat_up", "stage_trans", "stage_trans_x", "trans1_conv0a", "final_blend", "planar4_up", "t_down"}
    ids = [c.id for c in rs.ALL_CASES]
    assert len(ids) == len(set(ids))
    for mut in rs.MUTATIONS:
        assert any(m == mut for m, _ in rs.NEGATIVE), mut
    sizes = {(c.p["Hp"], c.p["Wp"]) for c in rs.ALL_CASES}
    assert set(rs.SIZES) <= sizes
    for op in ("stage_trans", "stage_trans_x", "final_blend"):
        assert any(c.p["xcd"] == 1 for c in rs.TABLES[op]) and any(c.p["xcd"] == 0 for c in rs.TABLES[op])
    for op, table in rs.TABLES.items():
        if op in ("flow_up", "feat_up", "planar4_up", "t_down"):
            assert any(c.p["B"] > 1 for c in table)
        else:
            assert {"b1", "b3", "b32"} <= {c.p["tasks"].rstrip("p") for c in table}, op
