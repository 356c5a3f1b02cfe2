"""cfi_amd.ops on the MI355X: the reference's custom-op interface on the HIP kernels of csrc/ref_ops.hip (sepconv, AdaCoF,
correlation, distance transform) and csrc/m2m_ops.hip (softsplat, costvol) through their NCHW wrappers.

  * goldens: tests/golden/ref_ops_golden.npz (tools/make_golden_ops.py: the reference's own kernel text for sepconv_out,
    kernel_AdaCoF_updateOutput, kernel_dt; a torch restatement for the correlation) and tests/golden/m2m_ops_ref.npz
    (the reference's softsplat_out / costvol_out);
  * 1080p-class shapes: sepconv and AdaCoF against the float64 restatements of tests/ref_ops_restated.py (run on the GPU) under
    their magnitude bound and the project's 1e-3 gate, the distance transform bit for bit against the exact one, correlation and
    softsplat against torch restatements here (<= 1e-3 per element);
  * channel-slice operands == .contiguous() ones and a batch of N == N single calls, bit for bit;
  * stream ordering by events only, and the errors of the interface."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_ops_restated as rs

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops(hip_lib):
    from cfi_amd import ops as m

    m.init()
    return m


@pytest.fixture(scope="module")
def gold(golden_dir):
    d = np.load(os.path.join(golden_dir, "ref_ops_golden.npz"))
    return {k: torch.from_numpy(d[k]).to(DEV) for k in d.files}


def _maxdiff(a, b):
    return (a.float() - b.float()).abs().max().item()


def _report(name, d):
    print(f"{name}: max|d| = {d:.3e}")


def _within_bound(got, want, M, gamma):
    """max|got - want| (for the 1e-3 gate) after asserting |got - want| <= gamma * 2^-24 * M everywhere"""
    d = (got.double() - want).abs()
    bad = ~(d <= rs.tolerance(M, gamma))
    assert not bad.any(), f"{int(bad.sum())} elements outside gamma*u*M"
    return d.max().item()


# ---- torch restatements ------------------------------------------------------------------------------------------------------

def corr_torch(a, b):
    N, C, H, W = a.shape
    bp = F.pad(b, (4, 4, 4, 4))
    out = torch.empty(N, 81, H, W, device=a.device)
    for dy in range(-4, 5):
        for dx in range(-4, 5):
            out[:, 9 * (dy + 4) + (dx + 4)] = (a * bp[:, :, 4 + dy:4 + dy + H, 4 + dx:4 + dx + W]).sum(1) / C
    return out


# ---- goldens (the reference's kernel text) -----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["sepconv_k51", "sepconv_k5"])
def test_sepconv_golden(ops, gold, case):
    got = ops.sepconv_func.apply(gold[f"{case}_in"], gold[f"{case}_ver"], gold[f"{case}_hor"])
    d = _maxdiff(got, gold[f"{case}_out"])
    _report(case, d)
    assert d <= 1e-4


@pytest.mark.parametrize("case,dil", [("adacof_f5", 1), ("adacof_f3d2", 2)])
def test_adacof_golden(ops, gold, case, dil):
    got = ops.FunctionAdaCoF.apply(gold[f"{case}_in"], gold[f"{case}_w"], gold[f"{case}_oi"], gold[f"{case}_oj"], dil)
    d = _maxdiff(got, gold[f"{case}_out"])
    _report(case, d)
    assert d <= 1e-4


@pytest.mark.parametrize("case", ["corr_c32", "corr_c196"])
def test_correlation_golden(ops, gold, case):
    got = ops.FunctionCorrelation(gold[f"{case}_a"], gold[f"{case}_b"])
    d = _maxdiff(got, gold[f"{case}_out"])
    _report(case, d)
    assert d <= 1e-4


@pytest.mark.parametrize("case", ["edt_mask3", "edt_mask4"])
def test_edt_golden_bit_exact(ops, gold, case):
    got = ops.batch_edt(gold[case])
    assert got.shape == gold[f"{case}_out"].shape
    assert torch.equal(got, gold[f"{case}_out"]), _maxdiff(got, gold[f"{case}_out"])


def test_softsplat_summation_golden(ops, golden_dir):
    d = np.load(os.path.join(golden_dir, "m2m_ops_ref.npz"))
    names = sorted({k[:-4] for k in d.files if k.startswith("splat_") and k.endswith("_out")})
    assert names
    worst = 0.0
    for nm in names:
        a, b, want = (torch.from_numpy(d[f"{nm}_{s}"]).to(DEV) for s in ("a", "b", "out"))
        got = ops.softsplat(a, b, None, "sum")
        worst = max(worst, _maxdiff(got, want))
    _report("softsplat sum vs softsplat_out", worst)
    assert worst <= 1e-4


def test_costvol_golden(ops, golden_dir):
    d = np.load(os.path.join(golden_dir, "m2m_ops_ref.npz"))
    worst = 0.0
    for nm in ("costvol_random", "costvol_tiny", "costvol_same"):
        a, b, want = (torch.from_numpy(d[f"{nm}_{s}"]).to(DEV) for s in ("a", "b", "out"))
        worst = max(worst, _maxdiff(ops.costvol_func.apply(a, b), want))
    _report("costvol vs costvol_out", worst)
    assert worst <= 1e-4


def _splat_modes_restated(ops, x, flow, metric, mode):
    """the reference wrappers' arithmetic (softsplat.py:325-435) around the summation op"""
    base = mode.split("-")[0]
    if base == "avg":
        x = torch.cat([x, x.new_ones(x.shape[0], 1, x.shape[2], x.shape[3])], 1)
    elif base == "linear":
        x = torch.cat([x * metric, metric], 1)
    elif base == "soft":
        x = torch.cat([x * metric.exp(), metric.exp()], 1)
    out = ops.softsplat_func.apply(x, flow)
    if base == "sum":
        return out
    nrm = out[:, -1:]
    eps = mode.split("-")[1] if "-" in mode else "addeps"
    if eps == "addeps":
        nrm = nrm + 1e-7
    elif eps == "zeroeps":
        nrm = torch.where(nrm == 0, torch.ones_like(nrm), nrm)
    else:
        nrm = nrm.clip(1e-7, None)
    return out[:, :-1] / nrm


@pytest.mark.parametrize("mode", ["avg", "linear", "soft", "soft-addeps", "soft-zeroeps", "soft-clipeps", "linear-zeroeps"])
def test_softsplat_modes(ops, mode):
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.rand(2, 3, 40, 56, device=DEV, generator=g)
    flow = (torch.rand(2, 2, 40, 56, device=DEV, generator=g) - 0.5) * 12
    metric = None if mode == "avg" else torch.rand(2, 1, 40, 56, device=DEV, generator=g) - 0.5
    got = ops.softsplat(x, flow, metric, mode)
    want = _splat_modes_restated(ops, x, flow, metric, mode)
    assert torch.equal(got, want)


@pytest.mark.parametrize("strType", ["summation", "average", "linear", "softmax"])
def test_function_softsplat_legacy(ops, strType):
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.rand(1, 3, 33, 47, device=DEV, generator=g)
    flow = (torch.rand(1, 2, 33, 47, device=DEV, generator=g) - 0.5) * 30      # far flows: some targets receive nothing
    metric = torch.rand(1, 1, 33, 47, device=DEV, generator=g) - 0.5
    got = ops.ModuleSoftsplat(strType)(x, flow, None if strType in ("summation", "average") else metric)
    if strType == "summation":
        want = ops.softsplat_func.apply(x, flow)
    else:
        xi = {"average": torch.cat([x, torch.ones_like(x[:, :1])], 1), "linear": torch.cat([x * metric, metric], 1),
              "softmax": torch.cat([x * metric.exp(), metric.exp()], 1)}[strType]
        o = ops.softsplat_func.apply(xi, flow)
        n = o[:, -1:]
        want = o[:, :-1] / torch.where(n == 0, torch.ones_like(n), n)
    assert torch.equal(got, want)


def test_softsplat_soft_golden(ops, golden_dir):
    """softsplat(..., "soft") against the reference's own execution of that wrapper in m2m_ops_ref.npz"""
    d = np.load(os.path.join(golden_dir, "m2m_ops_ref.npz"))
    a, f, m, want = (torch.from_numpy(d[k]).to(DEV) for k in ("soft_in", "soft_flow", "soft_metric", "soft_out"))
    dd = _maxdiff(ops.softsplat(a, f, m, "soft"), want)
    _report("softsplat soft vs reference", dd)
    assert dd <= 1e-4


# ---- 1080p-class shapes --------------------------------------------------------------------------------------------------------

def test_sepconv_1080p(ops):
    g = torch.Generator(device=DEV).manual_seed(5)
    K, Ho, Wo = 51, 1080, 1920
    x = torch.rand(1, 4, Ho + K - 1, Wo + K - 1, device=DEV, generator=g)
    ver = torch.rand(1, K, Ho, Wo, device=DEV, generator=g)
    hor = torch.rand(1, K, Ho, Wo, device=DEV, generator=g)
    ver, hor = ver / ver.sum(1, keepdim=True), hor / hor.sum(1, keepdim=True)
    got = ops.sepconv_func.apply(x, ver, hor)
    d = _within_bound(got, *rs.sepconv(x, ver, hor), rs.gamma_sepconv(K))
    _report("sepconv 1080p", d)
    assert d <= 1e-3


def test_adacof_1080p(ops):
    g = torch.Generator(device=DEV).manual_seed(6)
    Fs, Ho, Wo = 5, 1080, 1920
    x = torch.rand(1, 3, Ho + Fs - 1, Wo + Fs - 1, device=DEV, generator=g)
    w = torch.rand(1, Fs * Fs, Ho, Wo, device=DEV, generator=g)
    w = w / w.sum(1, keepdim=True)
    oi = (torch.rand(1, Fs * Fs, Ho, Wo, device=DEV, generator=g) - 0.5) * 8
    oj = (torch.rand(1, Fs * Fs, Ho, Wo, device=DEV, generator=g) - 0.5) * 8
    got = ops.FunctionAdaCoF.apply(x, w, oi, oj, 1)
    d = _within_bound(got, *rs.adacof(x, w, oi, oj, 1), rs.gamma_adacof(Fs))
    _report("adacof 1080p", d)
    assert d <= 1e-3


@pytest.mark.parametrize("C,H,W", [(32, 272, 480), (64, 136, 240), (196, 17, 30)])
def test_correlation_pwc_levels(ops, C, H, W):
    g = torch.Generator(device=DEV).manual_seed(C)
    a = torch.randn(1, C, H, W, device=DEV, generator=g)
    b = torch.randn(1, C, H, W, device=DEV, generator=g)
    d = _maxdiff(ops.FunctionCorrelation(a, b), corr_torch(a, b))
    _report(f"correlation C{C} {H}x{W}", d)
    assert d <= 1e-3


def test_edt_1080p(ops):
    """1080p bit for bit against the exact distance transform (int64 squared distances, correctly rounded square root)"""
    g = torch.Generator(device=DEV).manual_seed(7)
    m = (torch.rand(1, 1080, 1920, device=DEV, generator=g) > 0.9995)
    got = ops.batch_edt(m.unsqueeze(1))
    assert got.shape == (1, 1, 1080, 1920) and got.dtype == torch.bool
    got = ops.batch_edt(m.float()).cpu()
    want = rs.batch_edt(m.float())
    assert torch.equal(got, want), f"{int((got != want).sum())} pixels not bit-identical, max|d| = {_maxdiff(got, want):.3e}"


def test_softsplat_nchw_1080p(ops):
    g = torch.Generator(device=DEV).manual_seed(8)
    x = torch.rand(1, 4, 1088, 1920, device=DEV, generator=g)
    flow = (torch.rand(1, 2, 1088, 1920, device=DEV, generator=g) - 0.5) * 16
    got = ops.softsplat_func.apply(x, flow)
    # scatter-add restatement (softsplat_out's four atomicAdds)
    N, C, H, W = x.shape
    gy, gx = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    fx, fy = gx + flow[0, 0], gy + flow[0, 1]
    x0, y0 = fx.floor(), fy.floor()
    want = torch.zeros(C, H * W, device=DEV)
    for ox, oy, wgt in ((0, 0, (x0 + 1 - fx) * (y0 + 1 - fy)), (1, 0, (fx - x0) * (y0 + 1 - fy)),
                        (0, 1, (x0 + 1 - fx) * (fy - y0)), (1, 1, (fx - x0) * (fy - y0))):
        tx, ty = (x0 + ox).long(), (y0 + oy).long()
        ok = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        idx = (ty * W + tx)[ok]
        want.index_add_(1, idx, (x[0] * wgt)[:, ok])
    d = _maxdiff(got[0], want.view(C, H, W))
    _report("softsplat NCHW 1088x1920", d)
    assert d <= 1e-3


# ---- strides and batch -----------------------------------------------------------------------------------------------------------

def test_channel_slices_equal_contiguous(ops):
    g = torch.Generator(device=DEV).manual_seed(9)
    K = 51
    big = torch.rand(2, 6, 40 + K - 1, 70 + K - 1, device=DEV, generator=g)
    taps = torch.rand(2, 2 * K + 3, 40, 70, device=DEV, generator=g)
    x, ver, hor = big[:, 1:5], taps[:, 1:1 + K], taps[:, 2 + K:2 + 2 * K]
    assert not x.is_contiguous() and not ver.is_contiguous()
    assert torch.equal(ops.sepconv_func.apply(x, ver, hor), ops.sepconv_func.apply(x.contiguous(), ver.contiguous(), hor.contiguous()))
    # a transposed (x-major) view as well
    xt = big.transpose(2, 3).contiguous().transpose(2, 3)[:, :3]
    assert torch.equal(ops.sepconv_func.apply(xt, ver, hor), ops.sepconv_func.apply(xt.contiguous(), ver, hor))

    feat = torch.randn(2, 40, 30, 44, device=DEV, generator=g)
    a, b = feat[:, :32], feat[:, 8:40]
    assert torch.equal(ops.FunctionCorrelation(a, b), ops.FunctionCorrelation(a.contiguous(), b.contiguous()))

    s = torch.rand(2, 5, 30, 44, device=DEV, generator=g)
    fl = (torch.rand(2, 3, 30, 44, device=DEV, generator=g) - 0.5) * 10
    assert torch.equal(ops.softsplat_func.apply(s[:, :-1], fl[:, 1:]), ops.softsplat_func.apply(s[:, :-1].contiguous(), fl[:, 1:].contiguous()))
    assert torch.equal(ops.costvol_func.apply(feat[:, :32], feat[:, 4:36]),
                       ops.costvol_func.apply(feat[:, :32].contiguous(), feat[:, 4:36].contiguous()))


def test_batch_equals_single_calls(ops):
    g = torch.Generator(device=DEV).manual_seed(10)
    K, N = 51, 3
    x = torch.rand(N, 4, 24 + K - 1, 80 + K - 1, device=DEV, generator=g)
    ver = torch.rand(N, K, 24, 80, device=DEV, generator=g)
    hor = torch.rand(N, K, 24, 80, device=DEV, generator=g)
    one = lambda f, *t: torch.cat([f(*(u[i:i + 1] for u in t)) for i in range(N)])
    assert torch.equal(ops.sepconv_func.apply(x, ver, hor), one(ops.sepconv_func.apply, x, ver, hor))
    a = torch.randn(N, 32, 20, 36, device=DEV, generator=g)
    b = torch.randn(N, 32, 20, 36, device=DEV, generator=g)
    assert torch.equal(ops.FunctionCorrelation(a, b), one(ops.FunctionCorrelation, a, b))
    assert torch.equal(ops.costvol_func.apply(a, b), one(ops.costvol_func.apply, a, b))
    fl = (torch.rand(N, 2, 20, 36, device=DEV, generator=g) - 0.5) * 10
    assert torch.equal(ops.softsplat_func.apply(a, fl), one(ops.softsplat_func.apply, a, fl))
    xi = torch.rand(N, 3, 24, 40, device=DEV, generator=g)
    w = torch.rand(N, 25, 20, 36, device=DEV, generator=g)
    oi = torch.randn(N, 25, 20, 36, device=DEV, generator=g)
    oj = torch.randn(N, 25, 20, 36, device=DEV, generator=g)
    assert torch.equal(ops.FunctionAdaCoF.apply(xi, w, oi, oj, 1), one(lambda *t: ops.FunctionAdaCoF.apply(*t, 1), xi, w, oi, oj))
    m = torch.rand(N, 30, 50, device=DEV, generator=g) > 0.95
    assert torch.equal(ops.batch_edt(m.float()), one(lambda t: ops.batch_edt(t.float()), m))


# ---- streams -----------------------------------------------------------------------------------------------------------------------

def test_side_stream_ordering(ops):
    """inputs produced on a side stream, the op issued on the same side stream, the result consumed on the default stream after
    an event: correct without any device synchronisation (the ops launch on torch.cuda.current_stream())."""
    g = torch.Generator(device=DEV).manual_seed(11)
    K = 51
    x0 = torch.rand(1, 4, 200 + K - 1, 300 + K - 1, device=DEV, generator=g)
    ver = torch.rand(1, K, 200, 300, device=DEV, generator=g) / K
    hor = torch.rand(1, K, 200, 300, device=DEV, generator=g) / K
    a0 = torch.randn(1, 64, 120, 200, device=DEV, generator=g)
    want_s = ops.sepconv_func.apply(x0 * 2, ver, hor)
    want_c = ops.FunctionCorrelation(a0 * 2, a0)
    want_e = ops.batch_edt(a0[:, 0] > 2)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x = x0 * 2            # produced on the side stream: the op must be ordered behind it by the stream alone
        a = a0 * 2
        got_s = ops.sepconv_func.apply(x, ver, hor)
        got_c = ops.FunctionCorrelation(a, a0)
        got_e = ops.batch_edt(a0[:, 0] > 2)
        ev = torch.cuda.Event()
        ev.record(side)
    torch.cuda.current_stream().wait_event(ev)
    for t in (got_s, got_c, got_e):
        t.record_stream(torch.cuda.current_stream())
    assert torch.equal(got_s, want_s) and torch.equal(got_c, want_c) and torch.equal(got_e, want_e)


# ---- errors ------------------------------------------------------------------------------------------------------------------------

def test_dtype_errors_and_casts(ops):
    h = torch.rand(1, 3, 20, 20, device=DEV, dtype=torch.float16)
    with pytest.raises(TypeError, match="float16"):
        ops.FunctionAdaCoF.apply(h, torch.rand(1, 25, 16, 16, device=DEV).half(), torch.zeros(1, 25, 16, 16, device=DEV).half(),
                                 torch.zeros(1, 25, 16, 16, device=DEV).half(), 1)
    with pytest.raises(TypeError, match="float64"):
        ops.FunctionCorrelation(h.double(), h.double())
    with pytest.raises(TypeError, match="bfloat16"):
        ops.softsplat_func.apply(h.bfloat16(), torch.zeros(1, 2, 20, 20, device=DEV, dtype=torch.bfloat16))
    # sepconv_func / costvol_func cast to float32 like the reference's custom_fwd(cast_inputs=float32)
    x = torch.rand(1, 4, 14, 14, device=DEV)
    v = torch.rand(1, 5, 10, 10, device=DEV)
    assert torch.equal(ops.sepconv_func.apply(x.half(), v.half(), v.half()), ops.sepconv_func.apply(x.half().float(), v.half().float(), v.half().float()))
    c = torch.rand(1, 8, 6, 6, device=DEV)
    out = ops.costvol_func.apply(c.half(), c.half())
    assert out.dtype == torch.float32 and torch.equal(out, ops.costvol_func.apply(c.half().float(), c.half().float()))


def test_backward_raises(ops):
    x = torch.rand(1, 4, 14, 14, device=DEV, requires_grad=True)
    v = torch.rand(1, 5, 10, 10, device=DEV)
    with pytest.raises(NotImplementedError, match="backward"):
        ops.sepconv_func.apply(x, v, v).sum().backward()
    a = torch.rand(1, 8, 6, 6, device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError, match="backward"):
        ops.FunctionCorrelation(a, a).sum().backward()
    with pytest.raises(NotImplementedError, match="backward"):
        ops.softsplat(a, torch.zeros(1, 2, 6, 6, device=DEV), None, "sum").sum().backward()
    with pytest.raises(NotImplementedError, match="backward"):
        ops.costvol_func.apply(a, a).sum().backward()
    xi = torch.rand(1, 3, 10, 10, device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError, match="backward"):
        ops.FunctionAdaCoF.apply(xi, torch.rand(1, 25, 6, 6, device=DEV), torch.zeros(1, 25, 6, 6, device=DEV),
                                 torch.zeros(1, 25, 6, 6, device=DEV), 1).sum().backward()
