"""CPU: everything about tests/gen_ops_restated.py that needs no device.

  * every restatement against the oracle's own torch expression in float64 at 1e-11, or exactly: oracle/film_oracle.warp, F.avg_pool2d,
    F.interpolate (nearest in float32: torch's own rule; bilinear with a size and with a scale factor through oracle/ifrnet_oracle.resize),
    oracle/ifrnet_oracle.warp inside the output formula of IFRNet_L_arch.py:290-294, F.conv2d + F.prelu, and the expressions of
    oracle/ifunet_oracle.cbam piece by piece (avg / max pooling, the two-layer MLP, torch.max / torch.mean over channels, the 7x7
    convolution with the folded batch norm);
  * every condition a case claims, from the reference alone: mn > tol, the four clamp sides of the +-30 flows, the planted shifts name
    their displacement, both signs of the 7x7 pre-activation, the clamp of the output kernel binding at 0, at 1 and not at all, hidden
    units of both signs and none within its bound of zero, the strip counts the case ids state, the float32 'nearest' search;
  * every wrong restatement differs from the right one by more than both bounds together, in every case it is listed for;
  * the four CBAM entry points through the host build of their bodies (tests/hostcheck) under the same buffers and bounds."""
import math

import pytest
import torch
import torch.nn.functional as F

import gen_ops_restated as gr
import hostcheck
from oracle import film_oracle, ifrnet_oracle

IDS = dict(ids=lambda v: v.id if isinstance(v, gr.Case) else str(v).replace(" ", "-"))


@pytest.fixture(scope="module")
def lib():
    return hostcheck.load()


def _inputs(case):
    """{buffer: [px, C] window} of the case's operands, and its expectations"""
    B, _, es = gr._build(case, None, "cpu")
    return {n: b.host[b.G:b.G + b.px * b.cs].view(b.px, b.cs)[:, b.off:b.off + b.C] for n, b in B.b.items()}, es


def _close(a, b, eps=1e-11):
    d = (a.reshape(b.shape) - b).abs().max().item()
    assert d <= eps, d


def _nchw(t, N, H, W):
    return t.double().view(N, H, W, -1).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def test_tables_are_complete():
    ids = [c.id for c in gr.ALL_CASES]
    assert len(ids) == len(set(ids))
    assert set(gr.TABLES) == set(gr.OPS) and all(gr.TABLES[k] for k in gr.TABLES)
    assert all(cs for cs in gr.MUTATIONS.values())
    # every entry point of the three files is refused or launched by name
    called = {gr._build(t[0], None, "cpu")[1][0][0] for t in gr.TABLES.values()}
    assert called == {"vfi_avgpool2", "vfi_upsample_nearest", "vfi_resize_bilinear", "vfi_warp_film", "vfi_axpby", "vfi_ifrnet_prep", "vfi_ifrnet_center",
                      "vfi_conv7x7s2_prelu", "vfi_sigmoid", "vfi_fill_items", "vfi_resize_bilinear_ratio", "vfi_ifrnet_output", "vfi_channel_pool", "vfi_cbam_gate",
                      "vfi_cbam_scale_compress", "vfi_cbam_spatial"}


# ---------------------------------------------------------------------------------------------------------------- oracle ties

@pytest.mark.parametrize("case", gr.AVGPOOL_CASES, **IDS)
def test_avgpool_restated_is_torchs(case):
    p = case.p
    x, es = _inputs(case)
    xi = _nchw(x["in"], p["N"], p["H"], p["W"])[:, :, :p["H"] // 2 * 2, :p["W"] // 2 * 2]
    want = _nhwc(F.avg_pool2d(xi, 2, 2))
    _close(es[1]["want"], want)
    assert bool(((es[0]["want"] - es[1]["want"]).abs() <= es[1]["tol"]).all()), "the fp32 evaluation in the kernel's order lies within the float64 bound"
    assert torch.isfinite(es[0]["want"]).all() and torch.isfinite(es[1]["want"]).all()
    if p["H"] % 2 or p["W"] % 2:
        assert torch.isnan(x["in"]).any(), "the dropped row / column should hold NaN"


@pytest.mark.parametrize("case", gr.NEAREST_CASES, **IDS)
def test_nearest_restated_is_torchs_float32_rule(case):
    p = case.p
    x, es = _inputs(case)
    want = _nhwc(F.interpolate(x["in"].view(p["N"], p["Hi"], p["Wi"], -1).permute(0, 3, 1, 2), size=(p["Ho"], p["Wo"]), mode="nearest"))
    assert torch.equal(es[0]["want"].float().reshape(want.shape), want)


def test_nearest_float32_rule_leaves_the_rational_one():
    """for in, out <= 64 the float32 rule min(floor(dst * fl32(in / out)), in - 1) and floor(dst * in / out) disagree at a few (size pair, dst):
    two such pairs are cases (the kernel must follow torch), and torch itself follows the float32 rule there"""
    dis = gr.nearest_disagreements(64)
    assert dis, "no disagreement: drop the fp32-rule cases and say so in docs/design/gen_ops_coverage.md"
    pairs = sorted({(a, b) for a, b, _ in dis})
    assert [(c.p["Hi"], c.p["Ho"]) for c in gr.NEAREST_EXTRA] == pairs[:2]
    for n_in, n_out in pairs[:2]:
        x = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in)
        got = F.interpolate(x, size=(1, n_out), mode="nearest").view(-1).long()
        assert torch.equal(got, gr.nearest_index(n_in, n_out))
        assert not torch.equal(got, (torch.arange(n_out) * n_in // n_out).clamp_max(n_in - 1))


@pytest.mark.parametrize("case", gr.BILINEAR_CASES, **IDS)
def test_bilinear_restated_is_torchs(case):
    p = case.p
    x, es = _inputs(case)
    mul = gr._f32(p["mul"])
    want = _nhwc(F.interpolate(mul * _nchw(x["in"], p["N"], p["Hi"], p["Wi"]), size=(p["Ho"], p["Wo"]), mode="bilinear", align_corners=False))
    _close(es[0]["want"], want)


@pytest.mark.parametrize("case", gr.FILM_CASES, **IDS)
def test_warp_film_restated_is_the_oracles(case):
    p = case.p
    x, es = _inputs(case)
    img, fl = _nchw(x["in"], p["N"], p["H"], p["W"]), _nchw(x["flow"], p["N"], p["H"], p["W"])
    want = _nhwc(film_oracle.warp(img, fl * gr._f32(p["flow_mul"])))
    _close(es[0]["want"], want)


@pytest.mark.parametrize("case", gr.AXPBY_CASES, **IDS)
def test_axpby_fp32_order_is_within_the_float64_bound(case):
    es = gr.expectation(case)
    assert bool(((es[0]["want"] - es[1]["want"]).abs() <= es[1]["tol"]).all())


@pytest.mark.parametrize("case", gr.CONV7_CASES, **IDS)
def test_conv7x7s2_restated_is_torchs(case):
    p = case.p
    x, w, b, sl = gr.conv7_inputs(gr.SimpleNamespace(**p))
    want = F.prelu(F.conv2d(x.double(), w.double(), b.double(), 2, 3), sl.double())
    e = gr.expectation(case)[0]
    _close(e["want"], _nhwc(want))
    assert (e["pre"] > 0).any() and (e["pre"] < 0).any(), "both signs of the pre-activation"
    assert sl.min() >= 0.1 and sl.max() <= 0.4


@pytest.mark.parametrize("s", [0.5, 0.75, 1 / 0.75, 2.0, 4.0, 1.0])
@pytest.mark.parametrize("hw", [(8, 12), (7, 9), (3, 3)])
def test_resize_ratio_restated_is_the_oracles(s, hw):
    """with the ratio 1 / s in float64, as torch derives it for a float64 tensor; the op itself takes fl32(1 / s), the kernel's input"""
    x = torch.randn(2, 3, *hw, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    want = ifrnet_oracle.resize(x, s)
    ho, wo = int(math.floor(hw[0] * s)), int(math.floor(hw[1] * s))
    assert want.shape[2:] == (ho, wo)
    _close(gr._resize(_nhwc(x).contiguous(), 1 / s, 1 / s, ho, wo, gr.R_RATIO)[0], _nhwc(want))


@pytest.mark.parametrize("case", gr.RATIO_CASES, **IDS)
def test_resize_ratio_cases_take_the_float32_ratio(case):
    p = case.p
    x, es = _inputs(case)
    ho, wo = int(math.floor(p["Hi"] * p["s"])), int(math.floor(p["Wi"] * p["s"]))
    exact = gr._resize(x["in"].double().view(p["N"], p["Hi"], p["Wi"], -1), 1 / p["s"], 1 / p["s"], ho, wo, gr.R_RATIO)[0] * gr._f32(p["post_mul"])
    # fl32(1 / s) is within U of 1 / s: the position moves by less than U * size, far inside the position term of the bound
    assert bool(((es[0]["want"] - exact).abs() <= es[0]["tol"] + 1e-11).all())


@pytest.mark.parametrize("case", gr.OUTPUT_CASES, **IDS)
def test_ifrnet_output_restated_is_the_oracles(case):
    p = case.p
    x, es = _inputs(case)
    N, Hp, Wp, Hf, Wf, H, W = (p[k] for k in ("N", "Hp", "Wp", "Hf", "Wf", "H", "W"))
    fin = _nchw(x["fin"], N, Hf, Wf)
    i0, i1 = _nchw(x["img0"], N, Hp, Wp), _nchw(x["img1"], N, Hp, Wp)
    w0, w1 = ifrnet_oracle.warp(i0, fin[:, 0:2]), ifrnet_oracle.warp(i1, fin[:, 2:4])
    m = fin[:, 4:5]
    pre = m * w0 + (1 - m) * w1 + x["mean"].double().view(N, 1, 1, 1) + fin[:, 5:8]
    # the oracle builds its linspace grid in float32 before it follows the image to float64: each coordinate carries up to U of 1, half an
    # image size of pixels after the un-normalisation, on values of spread below 1 (images in [0.2, 0.8])
    _close(es[0]["want"], _nhwc(pre.clamp(0, 1))[:, :H, :W], gr.U * (Hp + Wp))
    v = es[0]["pre"]
    assert (v < 0).any() and (v > 1).any() and ((v > 0) & (v < 1)).any(), "the clamp binds at 0, at 1, and not at all"
    mk = x["fin"][:, 4]
    assert (mk == 0).any() and (mk == 1).any() and (((mk > 0) & (mk < 1)).any() or mk.numel() < 6)


@pytest.mark.parametrize("case", gr.CENTER_CASES, **IDS)
def test_center_restated_is_the_reference_mean(case):
    """mean_ = cat([img0, img1], 2).mean(1, 2, 3) (IFRNet_L_arch.py:242-247) from per-image channel means over equal pixel counts"""
    p = case.p
    x, es = _inputs(case)
    cm = x["cm"].double()
    mean = torch.stack([cm[:p["N"]], cm[p["N"]:]], 1).mean((1, 2))
    _close(es[1]["want"], mean.view(1, -1))
    _close(es[0]["want"], x["img"].double() - mean.repeat(2).repeat_interleave(p["px"]).unsqueeze(1), 1e-9 * p["scale"])


@pytest.mark.parametrize("case", gr.POOL_CASES, **IDS)
def test_channel_pool_restated_is_torchs(case):
    p = case.p
    x, es = _inputs(case)
    t = x["x"].double().view(p["N"], p["HW"], 1, p["C"]).permute(0, 3, 1, 2)
    _close(es[0]["want"], F.avg_pool2d(t, (p["HW"], 1)).reshape(-1, 1), 1e-11 * max(1.0, p["mean"]))
    assert torch.equal(es[1]["want"], F.max_pool2d(t, (p["HW"], 1)).reshape(-1, 1))
    strips = gr.pool_strips(p["ws_bytes"], p["N"], p["C"])[0]
    want = 128 if "capped" in case.id else int(case.id.split("strips")[1].split("-")[0]) if "strips" in case.id else 64
    assert strips == want


@pytest.mark.parametrize("case", gr.GATE_CASES, **IDS)
def test_gate_restated_is_the_oracles_mlp(case):
    x, es = _inputs(case)
    p = case.p
    st = x["stats"].double().view(p["N"], p["C"], 2)
    att = None
    for k in range(2):
        v = F.linear(F.relu(F.linear(st[..., k], x["w1"].double(), x["b1"].double().view(-1))), x["w2"].double(), x["b2"].double().view(-1))
        att = v if att is None else att + v
    e = es[0]
    _close(e["want"], torch.sigmoid(att))
    assert (e["hid"] > 0).any() and (e["hid"] < 0).any(), "hidden units of both signs"
    assert bool((e["hid"].abs() > e["hid_tol"]).all()), "a hidden unit within its bound of zero makes the ReLU ambiguous: reseed the case"


@pytest.mark.parametrize("case", gr.SCALE_CASES, **IDS)
def test_scale_compress_restated_is_the_oracles(case):
    x, es = _inputs(case)
    p = case.p
    xs = x["x"].double().view(p["N"], p["HW"], p["C"]) * x["scale"].double().view(p["N"], 1, p["C"])
    assert torch.equal(es[0]["want"].float(), xs.float().view(-1, p["C"]))
    r = es[0]["want"].view(p["N"], p["HW"], p["C"]).permute(0, 2, 1)          # the fp32 products, as ChannelPool sees them
    assert torch.equal(es[1]["want"].view(-1), torch.max(r, 1)[0].reshape(-1))
    _close(es[2]["want"].view(-1), torch.mean(r, 1).reshape(-1))


@pytest.mark.parametrize("case", gr.SPATIAL_CASES, **IDS)
def test_spatial_restated_is_the_oracles(case):
    x, es = _inputs(case)
    p = case.p
    comp = _nchw(x["comp"], p["N"], p["H"], p["W"])
    s = F.conv2d(comp, x["w"].double().view(7, 7, 2).permute(2, 0, 1)[None], None, 1, 3)
    s = s * gr._f32(p["bn_a"]) + gr._f32(p["bn_b"])                             # the eval-mode batch norm, folded
    want = x["xs"].double().view(p["N"], p["H"], p["W"], p["C"]) * _nhwc(torch.sigmoid(s))
    _close(es[0]["want"], want.reshape(-1, p["C"]))


def test_sigmoid_fill_prep_are_torchs():
    for case in gr.SIGMOID_CASES:
        x, es = _inputs(case)
        _close(es[0]["want"], torch.sigmoid(x["x"].double()))
    big = _inputs(gr.SIGMOID_CASES[1])[0]["x"].view(-1).tolist()
    assert all(v in big for v in gr.SIGMOID_PLANTED)
    for case in gr.PREP_CASES:
        p = case.p
        x, es = _inputs(case)
        for k in range(2):
            f = x[f"f{k}"].view(p["H"], p["W"], p["C"])[..., :3].permute(2, 0, 1)
            want = F.pad(torch.cat([f, torch.zeros(1, p["H"], p["W"])]), (0, p["Wp"] - p["W"], 0, p["Hp"] - p["H"])).permute(1, 2, 0)
            assert torch.equal(es[k]["want"].float().view(p["Hp"], p["Wp"], 4), want)
            assert p["C"] == 3 or torch.isnan(x[f"f{k}"][:, 3:]).all()


# ---------------------------------------------------------------------------------------------------------------- conditions

@pytest.mark.parametrize("case", gr.ALL_CASES, **IDS)
def test_every_summand_is_above_the_bound(case):
    for e in gr.expectation(case):
        if e.get("mn") is not None:
            assert bool((e["mn"] > e["tol"]).all()), case.id
        if e.get("tol") is not None:
            assert torch.isfinite(e["tol"]).all() and torch.isfinite(e["want"]).all()


@pytest.mark.parametrize("case", [c for c in gr.FILM_CASES if c.p["flow"] == "far"], **IDS)
def test_far_flows_clamp_on_all_four_sides(case):
    e = gr.expectation(case)[0]
    p = case.p
    assert (e["px"] < 0).any() and (e["px"] > p["W"] - 1).any() and (e["py"] < 0).any() and (e["py"] > p["H"] - 1).any()
    assert bool(((e["px"] < 0) | (e["px"] > p["W"] - 1)).all()) and bool(((e["py"] < 0) | (e["py"] > p["H"] - 1)).all())


@pytest.mark.parametrize("case", gr.FILM_PLANTED, **IDS)
def test_planted_shift_names_the_displacement(case):
    p = case.p
    e = gr.expectation(case)[0]
    dx, dy = (v * p["flow_mul"] for v in p["flow"])
    assert dx != dy and dx == int(dx) and dy == int(dy) and {dx > 0, dy > 0} == {True, False}
    X = (torch.arange(p["W"], dtype=torch.float64) + dx).clamp(0, p["W"] - 1).view(1, 1, -1, 1)
    Y = (torch.arange(p["H"], dtype=torch.float64) + dy).clamp(0, p["H"] - 1).view(1, -1, 1, 1)
    assert bool(((e["want"] - (X + 10 * Y)).abs() <= e["tol"]).all()) and float(e["tol"].max()) < 0.01


# ---------------------------------------------------------------------------------------------------------------- mutations

@pytest.mark.parametrize("case,mut", gr.NEGATIVE, **IDS)
def test_wrong_restatement_is_further_than_both_bounds(case, mut):
    right, wrong = gr.expectation(case), gr.expectation(case, mut)
    far = False
    for a, b in zip(right, wrong):
        ta, tb = (0 if e["tol"] is None else e["tol"] for e in (a, b))
        far = far or bool(((a["want"] - b["want"]).abs() > ta + tb).any())
    assert far, f"{case.id}: '{mut}' stays within the bounds everywhere"


# ---------------------------------------------------------------------------------------------------------------- host bodies

@pytest.mark.parametrize("case", gr.HOST_CASES, **IDS)
def test_cbam_case_on_the_host_build_of_the_bodies(lib, case):
    gr.run_case(lib, case)


@pytest.mark.parametrize("case,mut", [(c, m) for c, m in gr.NEGATIVE if c in gr.HOST_CASES], **IDS)
def test_wrong_restatement_fails_on_the_host_result(lib, case, mut):
    with pytest.raises(AssertionError, match="outside the bound"):
        gr.run_case(lib, case, mut=mut)


def test_channel_pool_refuses_a_short_workspace_on_the_host(lib):
    B, calls, _ = gr._build(gr.POOL_REFUSED, None, "cpu")
    assert gr.pool_strips(gr.POOL_REFUSED.p["ws_bytes"], 1, 17)[0] == 63
    assert lib.vfi_channel_pool(*calls[0][1], None) != 0
    for b in B.b.values():
        b.win[:] = False
    B.finish()
