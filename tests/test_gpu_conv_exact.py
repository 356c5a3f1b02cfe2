"""Every convolution form a layer object can take, against the float64 restatement of tests/conv_restated.py on data whose fp32 sums are
exact in any order: the pre-activation tolerance is ZERO, so act 0 - 3 (with residual and post affine) are compared bit for bit, no
element left out; sigmoid and GELU within the derived bounds of conv_restated.tolerance (their max err / tol is printed).

Which kernel ran is not guessed: after every call vfi_test_last_conv_launch (include/vfi_hip_test.h) says family, tile variant or
Winograd region shape, EXT / MASKED / MODE, store form, split-K slices, grid.x and tiles — and the case asserts the form it meant to
run.  Tables: tests/conv_exact_cases.py — (a) every direct tile variant forced by trace name, plain and EXT, + one persistent launch,
(b) split-K with every epilogue in the reduce kernel, equal to the unsplit call, (c) both Winograd region shapes x every MODE, the
transposed-convolution and embedded 2x2 forms, equal to the direct kernel, (d) where the default heuristics send a table of shapes.

Buffers: the input is a Cin_phys-channel window of a wider NaN tensor with a NaN pixel row before the first and after the last image;
positions of the window no logical channel maps to hold 12345 (finite: the interface allows anything finite there, their weights are
zero); the output is NaN-filled with guard channels on both sides and guard pixels before and after; the residual likewise.  One NaN
read, one stray write or one missing write fails the case."""
import ctypes as C

import pytest
import torch

import conv_exact_cases as cc
import conv_restated as cr

pytestmark = pytest.mark.gpu

NAN = float("nan")
IN_OFF, OUT_OFF, RES_OFF = 8, 3, 2          # channel offsets of the windows (floats); the input's keeps 16-byte alignment
OPTION_DEFAULTS = {"splitk": 1, "deconv_wino": 1}


def _ck(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


def _last_launch(lib):
    rec = (C.c_int32 * 8)()
    assert lib.vfi_test_last_conv_launch(rec, 8) == 8
    return list(rec)


def _create(lib, case, d):
    """-> handle, keep-alive list"""
    cm = torch.tensor(d.cmap, dtype=torch.int32) if d.cmap is not None else None
    w, b, pre = d.w.float().contiguous(), d.b.float().contiguous(), d.prelu.float().contiguous()
    assert torch.equal(w.double(), d.w) and torch.equal(b.double(), d.b)          # the fp32 the library gets IS the exact data
    if case.api == "up2":
        h = lib.vfi_conv_create_up2x2(w.data_ptr(), b.data_ptr(), case.cout, case.cin, cm.data_ptr() if cm is not None else None, case.cphys)
    elif case.api == "plain":
        h = lib.vfi_conv_create(w.data_ptr(), b.data_ptr(), case.cout, case.cin, case.k, case.k, cm.data_ptr() if cm is not None else None, case.cphys)
    else:
        cmc = (C.c_int * len(d.cmap))(*d.cmap) if d.cmap is not None else None
        h = lib.vfi_conv_create_ex(case.kind, w.data_ptr(), b.data_ptr(), case.cout, case.cin, case.k, case.stride, case.pad, cmc, case.cphys, pre.data_ptr())
    assert h, "create failed"
    return h


def _forward(lib, h, case, d):
    """One call inside NaN surroundings -> (output window [N, Ho, Wo, Cout] on the host, launch record)."""
    n, hh, ww = case.n, case.h, case.w
    ho, wo = case.out_hw
    in_cs, out_cs, res_cs = IN_OFF + case.cphys + 8, OUT_OFF + case.cout + 5, RES_OFF + case.cout + 4
    xin = torch.full((ww + n * hh * ww + ww, in_cs), NAN)
    xin[ww:ww + n * hh * ww, IN_OFF:IN_OFF + case.cphys] = cr.window(case, d).reshape(-1, case.cphys)
    xd = xin.cuda()
    out = torch.full((1 + n * ho * wo + 2, out_cs), NAN, device="cuda")
    in_ptr = xd.data_ptr() + 4 * (ww * in_cs + IN_OFF)
    out_ptr = out.data_ptr() + 4 * (out_cs + OUT_OFF)
    res_ptr, rd = None, None
    if d.res is not None:
        r = torch.full((1 + n * ho * wo + 1, res_cs), NAN)
        r[1:-1, RES_OFF:RES_OFF + case.cout] = d.res.float().reshape(-1, case.cout)
        rd = r.cuda()
        res_ptr = rd.data_ptr() + 4 * (res_cs + RES_OFF)
    before = _last_launch(lib)[7]
    if case.api == "ex":
        ps, sh = case.post if case.post is not None else (0.0, 0.0)
        _ck(lib.vfi_conv_forward_ex(h, in_ptr, in_cs, hh, ww, out_ptr, out_cs, n, case.act, case.slope, ps, sh, res_ptr, res_cs if rd is not None else 0, None), "forward_ex")
    else:
        assert d.res is None and case.post is None
        _ck(lib.vfi_conv_forward(h, in_ptr, in_cs, out_ptr, out_cs, n, hh, ww, case.act, case.slope, None), "forward")
    torch.cuda.synchronize()
    rec = _last_launch(lib)
    assert rec[7] == before + 1, f"{rec[7] - before} launches recorded for one call"
    got = out.cpu()
    assert torch.isnan(got[0]).all() and torch.isnan(got[-2:]).all(), "wrote a guard pixel before / after the output"
    body = got[1:-2]
    assert torch.isnan(body[:, :OUT_OFF]).all() and torch.isnan(body[:, OUT_OFF + case.cout:]).all(), "wrote a guard channel"
    win = body[:, OUT_OFF:OUT_OFF + case.cout].reshape(n, ho, wo, case.cout)
    nan = torch.isnan(win)
    assert not nan.any(), f"{int(nan.sum())} of {nan.numel()} outputs NaN (unwritten, or a NaN was read); first at {nan.nonzero()[0].tolist()}"
    return win, rec


def _check_launch(rec, case, expect, algo, what):
    fam, var, form, store, ks, gx, work, _ = rec
    exp = dict(expect)
    if "form" not in exp and fam in (cc.GEN1, cc.GEN2):
        exp["form"] = cc.EXT if (case.kind == 1 or case.pad or case.act >= 3 or case.post is not None) else cc.PLAIN
    exp.setdefault("ks", 1)
    desc = f"{what}: launch family {fam} variant {var} form {form} store {store} ks {ks} grid.x {gx} work {work}"
    if algo == 1:
        assert fam in (cc.GEN1, cc.GEN2), desc
    for key, have in (("family", fam), ("variant", var), ("form", form), ("store", store)):
        assert key not in exp or exp[key] == have, f"{desc}; expected {key} {exp[key]}"
    assert (ks > 1) if exp["ks"] == ">1" else ks == exp["ks"], f"{desc}; expected ks {exp['ks']}"
    if exp.get("persistent"):
        assert gx < work, f"{desc}; expected a persistent launch (grid.x < tiles)"


def _compare(got, case, v, y, what):
    want = y.float()
    if case.act < 4:
        assert torch.equal(want.double(), y) or case.post is not None      # the cast is exact (one rounding with a post affine)
        if not torch.equal(got, want):
            bad = got != want
            i = bad.nonzero()[0].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result; first at {i}: got {got[tuple(i)].item()!r} "
                                 f"want {want[tuple(i)].item()!r} (pre-activation {v[tuple(i)].item()!r})")
        return None
    err = (got.double() - y).abs()
    tol = cr.tolerance(case, v, y)
    rel = torch.where(err == 0, torch.zeros_like(err), err / tol)      # GELU(0): tol = 0 and the kernels give exactly 0
    ratio = float(rel.max())
    print(f"  {what}: {'sigmoid' if case.act == 4 else 'GELU'} max err / tol = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: err / tol = {ratio:.3f} at flat index {rel.argmax().item()}"
    return ratio


def _run_job(lib, job):
    datas = [cr.make(c) for c in job.cases]
    refs = [cr.restate(c, d) for c, d in zip(job.cases, datas)]
    for d in datas[1:]:
        assert torch.equal(d.w, datas[0].w) and d.cmap == datas[0].cmap, "the cases of a job share one layer"
    setups = [dict(algo=job.algo, opts=job.opts, variant=job.variant, expect=job.expect)]
    setups += [dict(algo=s.get("algo", 0), opts=s.get("opts", {}), variant=s.get("variant"), expect=s.get("expect", {})) for s in job.same_bits]
    h = _create(lib, job.cases[0], datas[0])
    results = []
    try:
        if any(c.odd for c in job.cases):
            _ck(lib.vfi_conv_accept_odd(h, 1), "accept_odd")
        for si, s in enumerate(setups):
            outs = []
            try:
                lib.vfi_test_conv_algo(s["algo"])
                for name, val in s["opts"].items():
                    assert lib.vfi_test_set_option(name.encode(), val) == 0
                if s["variant"] is not None:
                    lib.vfi_test_variant_override(f"{cc.trace_name(job.cases[0])}={s['variant']}".encode())
                for ci, (case, d) in enumerate(zip(job.cases, datas)):
                    what = f"{job.id}[setup {si}, call {ci}: n{case.n} {case.h}x{case.w} act{case.act}]"
                    got, rec = _forward(lib, h, case, d)
                    _check_launch(rec, case, s["expect"], s["algo"], what)
                    _compare(got, case, *refs[ci], what)
                    outs.append(got)
            finally:
                lib.vfi_test_variant_override(b"")
                lib.vfi_test_conv_algo(0)
                for name in s["opts"]:
                    lib.vfi_test_set_option(name.encode(), OPTION_DEFAULTS[name])
            results.append(outs)
    finally:
        lib.vfi_conv_destroy(h)
    for si in range(1, len(results)):
        for ci, case in enumerate(job.cases):
            same = torch.equal(results[si][ci], results[0][ci])
            if case.act < 4:
                assert same, f"{job.id}: set-up {si} and set-up 0 differ on call {ci}"
            elif not same:      # both are within the bound of the float64 value; the two epilogues round expf / erff differently
                print(f"  {job.id}: call {ci} act{case.act}: set-up {si} differs from set-up 0 by {(results[si][ci] - results[0][ci]).abs().max().item():.3e}")


@pytest.mark.parametrize("job", cc.VARIANT_JOBS, ids=lambda j: j.id)
def test_forced_tile_variant(hip_lib, job):
    _run_job(hip_lib, job)


def test_persistent_launch(hip_lib, oracle_threads):
    _run_job(hip_lib, cc.PERSISTENT_JOB)


@pytest.mark.parametrize("job", cc.SPLIT_JOBS, ids=lambda j: j.id)
def test_split_k_epilogue_in_reduce_kernel(hip_lib, job):
    _run_job(hip_lib, job)


@pytest.mark.parametrize("job", cc.WINO_JOBS, ids=lambda j: j.id)
def test_winograd(hip_lib, oracle_threads, job):
    _run_job(hip_lib, job)


@pytest.mark.parametrize("job", cc.DEFAULT_JOBS, ids=lambda j: j.id)
def test_default_choice(hip_lib, oracle_threads, job):
    _run_job(hip_lib, job)


def test_one_wrong_weight_is_seen(hip_lib):
    """Negative control through the GPU path: the library gets ONE weight with the wrong sign.  Output channel 0 must differ from the
    exact result of the right weights wherever that tap is inside the image, every other channel must still match bit for bit."""
    case = cr.Case(k=3, cin=8, cphys=8, cout=9, n=1, h=9, w=11, wino=True)
    d = cr.make(case)
    want = cr.restate(case, d)[1].float()
    for algo in (1, 2):
        h = _create(hip_lib, case, cr.mutate(case, d, "sign"))
        try:
            hip_lib.vfi_test_conv_algo(algo)
            got, rec = _forward(hip_lib, h, case, d)
        finally:
            hip_lib.vfi_test_conv_algo(0)
            hip_lib.vfi_conv_destroy(h)
        assert (rec[0] == cc.WINO) == (algo == 2)
        assert torch.equal(got[..., 1:], want[..., 1:])
        assert bool((got[0, 1:, 1:, 0] != want[0, 1:, 1:, 0]).all())      # tap (0, 0) of channel 0 reads pixel (y - 1, x - 1): odd x, never zero
