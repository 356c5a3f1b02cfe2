"""tests/conv_restated.py checked without a GPU: the exactness certificate of every case the GPU tables run, the restatement against
torch's own float64 operators on the same data, negative controls, and the tables' copy of the tile-variant list against the sources."""
import os
import re

import pytest
import torch

import conv_exact_cases as cc
import conv_restated as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one representative call per interface feature, for the operator comparison and the controls
FAMILIES = [
    cr.Case(k=3, cin=5, cphys=8, cout=9, n=2, h=9, w=11, act=1, slope=-0.5, wino=True, cmap=True),
    cr.Case(k=3, pad=1, cin=8, cphys=8, cout=9, n=1, h=7, w=10, act=3, res=True, wino=True),
    cr.Case(k=3, pad=2, cin=8, cphys=8, cout=9, n=1, h=7, w=10, act=2, post=(-2.0, 1.0), wino=True),
    cr.Case(k=3, stride=2, cin=8, cphys=8, cout=9, n=2, h=8, w=12, act=4),
    cr.Case(k=3, stride=2, pad=1, cin=8, cphys=8, cout=9, n=1, h=9, w=13, odd=True, act=5),
    cr.Case(k=3, stride=2, pad=2, cin=8, cphys=8, cout=9, n=1, h=9, w=13, odd=True),
    cr.Case(k=2, stride=2, cin=8, cphys=8, cout=9, n=2, h=8, w=12, act=3),
    cr.Case(k=1, cin=21, cphys=24, cout=9, n=2, h=5, w=7, act=4, post=(0.5, 3.0), cmap=True),
    cr.Case(api="plain", k=3, cin=8, cphys=8, cout=9, n=1, h=9, w=11, act=1, slope=0.25, wino=True),
    cr.Case(api="plain", k=2, cin=8, cphys=8, cout=9, n=1, h=9, w=11, act=1, slope=0.25),
    cr.Case(api="plain", k=1, cin=8, cphys=8, cout=9, n=1, h=9, w=11),
    cr.Case(api="up2", k=2, cin=5, cphys=8, cout=64, n=2, h=5, w=7, act=1, slope=0.25),
    cr.Case(kind=1, k=4, stride=2, cin=8, cphys=8, cout=9, n=2, h=5, w=7, act=3, wino=True),
    cr.Case(kind=1, k=4, stride=2, pad=1, cin=8, cphys=8, cout=9, n=1, h=5, w=7, act=1, slope=2.0, wino=True),
]


@pytest.mark.parametrize("job", cc.ALL_JOBS, ids=lambda j: j.id)
def test_certificate_holds_for_every_gpu_case(job):
    """make() asserts the certificate(s); here also: the cases of one job share one layer, x is odd, no weight is zero."""
    first = None
    for case in job.cases:
        d = cr.make(case)
        assert d.cert["direct"] < cr.LIMIT and (not case.wino or d.cert["wino"] < cr.LIMIT)
        assert bool((d.x.abs() % 2 == 1).all()) and d.x.abs().max() <= d.X and bool((d.w != 0).all())
        assert d.X >= 1 and (d.X + 1) & d.X == 0
        if first is None:
            first = d
        assert torch.equal(d.w, first.w) and torch.equal(d.b, first.b) and torch.equal(d.prelu, first.prelu) and d.cmap == first.cmap


def test_short_reductions_carry_many_bits():
    assert cr.make(cr.Case(k=3, cin=8, cphys=8, cout=9)).X == 2 ** 15 - 1
    assert cr.make(cr.Case(k=3, cin=8, cphys=8, cout=9, wino=True)).X >= 2 ** 12 - 1
    assert cr.make(cr.Case(k=1, cin=1184, cphys=1184, cout=9)).X >= 2 ** 12 - 1


@pytest.mark.parametrize("case", FAMILIES, ids=lambda c: f"{c.api}-kind{c.kind}-k{c.k}s{c.stride}p{c.pad}")
def test_restatement_equals_torch_operators(case):
    d = cr.make(case)
    v, y = cr.restate(case, d)
    want = cr.torch_preact(case, d)
    if d.res is not None:
        want = want + d.res
    assert torch.equal(v, want), (v - want).abs().max()      # exact data: float64 has no rounding either, in either order
    tv = v.permute(0, 3, 1, 2)
    act = {0: lambda t: t, 1: lambda t: torch.where(t > 0, t, t * case.slope), 2: lambda t: t.clamp(0, 1),
           3: lambda t: torch.nn.functional.prelu(t, d.prelu), 4: torch.sigmoid, 5: torch.nn.functional.gelu}[case.act](tv)
    if case.post:
        act = act * case.post[0] + case.post[1]
    assert (y - act.permute(0, 2, 3, 1)).abs().max() <= 1e-15 * max(1.0, float(y.abs().max()))
    if case.act < 4:
        assert torch.equal(cr.tolerance(case, v, y), torch.zeros_like(y))
    else:
        assert bool((cr.tolerance(case, v, y) > 0).all())


@pytest.mark.parametrize("case", FAMILIES, ids=lambda c: f"{c.api}-kind{c.kind}-k{c.k}s{c.stride}p{c.pad}")
@pytest.mark.parametrize("how", ["sign", "swap", "shift"])
def test_negative_controls_change_the_result(case, how):
    d = cr.make(case)
    v, _ = cr.restate(case, d)
    v2, _ = cr.restate(case, d, shift=1) if how == "shift" else cr.restate(case, cr.mutate(case, d, how))
    assert not torch.equal(v, v2)


def test_one_dropped_term_always_shows():
    """every term is an odd multiple of the unit: removing any single one changes the sum (here: each input pixel of one channel zeroed)"""
    case = cr.Case(k=3, cin=8, cphys=8, cout=9, n=1, h=5, w=6)
    d = cr.make(case)
    v, _ = cr.restate(case, d)
    for y in range(case.h):
        for x in range(case.w):
            xz = d.x.clone()
            xz[0, y, x, 3] = 0
            v2 = cr.preact(case, xz, d.w, d.b)
            changed = (v2 != v).any(dim=-1)[0]
            assert bool(changed[max(0, y - 1):y + 2, max(0, x - 1):x + 2].all()), (y, x)


def test_window_fill_and_channel_map():
    case = cr.Case(k=1, cin=5, cphys=8, cout=9, n=1, h=2, w=3, cmap=True)
    d = cr.make(case)
    win = cr.window(case, d)
    assert win.shape == (1, 2, 3, 8) and sorted(d.cmap) != d.cmap and len(set(d.cmap)) == 5
    for i, pc in enumerate(d.cmap):
        assert torch.equal(win[..., pc].double(), d.x[..., i])
    rest = [c for c in range(8) if c not in d.cmap]
    assert bool((win[..., rest] == cr.FILL).all())


def test_variant_table_copy_matches_sources():
    rows = {}
    for fname, base in (("conv_mfma.hip", 0), ("conv_mfma2.hip", 32)):
        with open(os.path.join(ROOT, "comfyui-frame-interpolation_amd", "csrc", fname)) as fh:
            text = fh.read()
        body = text[text.index("static const ConvVariant kVariants"):]
        body = body[:body.index("};")]
        found = re.findall(r'\{"(\w+)",\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+)\}', body)
        for i, f in enumerate(found):
            rows[base + i] = tuple(int(v) for v in f[1:])
    assert rows == cc.VARIANTS
    covered = {j.variant for j in cc.VARIANT_JOBS}
    assert covered == set(cc.VARIANTS), "a tile variant without a forced case"


def test_job_ids_unique():
    ids = [j.id for j in cc.ALL_JOBS]
    assert len(ids) == len(set(ids))
