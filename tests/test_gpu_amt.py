"""-m gpu: AMT's new kernels (csrc/amt_net.hip) on the MI355X, each pinned on its own against a float64 restatement, inputs and outputs
inside NaN surroundings, with bounds in the style of tests/ref_ops_restated.py: |got - want| <= gamma * 2^-24 * M, M = sum |term| of the
element and gamma the longest chain of fp32 roundings on the way to it.

  lookup      amt_restated.lookup_tolerance: gamma_lookup(D) = D + 19 on M, plus 2 U C for the fractions of negative coordinates (both
              derived in tests/amt_restated.py); the kernel takes floor and fraction of c / 2^lvl directly, so there is no coordinate term.  The test computes c = grid + flow * scale itself in fp32 with two roundings, as
              the kernel and torch do.  Cases: tests/golden/amt_lookup.npz's (windows off every side, queries exactly on integer
              positions, all-zero windows, a map with odd pooled sizes, D = 84 and 128), also compared with the reference's own fp32 output
              (with its coordinate slack), and a positive case whose smallest summand exceeds the bound, so a dropped corner or channel
              could not hide.
  conv7x7     49 Cin products + bias: gamma = 49 Cin + 2, + 1 for the activation's product.
  combine     warps: the kernel follows the reference's fp32 coordinate arithmetic, float64 does not round: the sampling position differs
              by up to 6 U (size + |flow|) pixels per axis, which moves a bilinear sample by at most that times twice the image's range
              per axis; sigmoid within 4 U; eight roundings over the blend's terms.  tail: n - 1 additions, a division, an addition.
  object      vfi_amt_create / _forward (AmtEngine) and the node: see the tests at the end of the file.
  in place    the fp32 forward of tests/amt_restated.py with these kernels in the place of its torch code, against the reference's own
              forward (tests/golden/amt_net.npz) and the float64 restatement: per-pixel |d| <= 1e-3, the project's gate, every pixel.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import amt_restated
import cain_restated
from amt_restated import NET_STRIDE, NET_TS, SEED, TOL, frames_of, pack7x7
from gpu_util import describe_diff, ptr

pytestmark = pytest.mark.gpu
NAN = float("nan")
U = amt_restated.U
PLANES = 196


def _check(rc, what):
    from cfi_amd import _lib

    _lib.check(rc, what)


@pytest.fixture(scope="module")
def lib(hip_lib):
    from cfi_amd import _lib

    _lib.check(hip_lib.vfi_init(0), "vfi_init")
    return hip_lib


def _bounded(got, want, tol, name):
    assert torch.isfinite(got).all(), f"{name}: NaN in the output: a stray read or an unwritten element"
    err = (got.double() - want).abs()
    print(f"{name}: max |d| {float(err.max()):.3e}, max d / tol {float((err / tol.clamp_min(1e-300)).max()):.3f}")
    bad = err > tol
    assert not bad.any(), describe_diff(got.double(), want, name) + f", {int(bad.sum())} over the float64 bound"


def pooled_floats(h, w, D):
    return sum((h >> l) * (w >> l) for l in (1, 2, 3)) * D


def run_lookup(lib, fq, ft, flow, scale):
    """fq, ft [D,h,w], flow [2,h,w] host fp32 -> [196,h,w] host, through NHWC device buffers between NaN guards"""
    D, h, w = fq.shape
    q = fq.permute(1, 2, 0).contiguous().cuda()
    t = ft.permute(1, 2, 0).contiguous().cuda()
    pooled = torch.full((pooled_floats(h, w, D) + 64,), NAN, device="cuda")
    fl = torch.full((h, w, 5), NAN, device="cuda")
    fl[..., :2] = flow.permute(1, 2, 0).cuda()
    out = torch.full((h * w + 2, PLANES + 7), NAN, device="cuda")
    _check(lib.vfi_amt_pool_features(ptr(t), h, w, D, ptr(pooled), None), "vfi_amt_pool_features")
    _check(lib.vfi_amt_corr_lookup(ptr(q), ptr(t), ptr(pooled), ptr(fl), 5, C.c_float(scale), h, w, D, ptr(out), PLANES + 7, None), "vfi_amt_corr_lookup")
    torch.cuda.synchronize()
    assert torch.isnan(pooled[pooled_floats(h, w, D):]).all() and torch.isfinite(pooled[:pooled_floats(h, w, D)]).all(), "pooling wrote astray"
    assert torch.isnan(out[h * w:]).all() and torch.isnan(out[:, PLANES:]).all(), "the lookup wrote outside its 196 channels"
    return out[:h * w, :PLANES].reshape(h, w, PLANES).permute(2, 0, 1).cpu()


def kernel_coords(c, scale):
    """flow and the fp32 coordinates the kernel derives from it: grid + flow * scale, two roundings"""
    _, h, w = c.shape
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xs, ys])
    flow = (c - grid) / scale
    return flow, grid + flow * torch.tensor(scale, dtype=torch.float32)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", sorted(amt_restated.LOOKUP_CASES))
def test_corr_lookup_vs_float64_and_the_reference(lib, name, which, golden_dir):
    f0, f1, c0, c1 = amt_restated.lookup_case(name)
    fq, ft, c = (f0, f1, c0) if which == 0 else (f1, f0, c1)
    D, h, w = fq.shape
    for scale in (1.0, 1.25):                    # 1.0 keeps the golden case's integer positions exact
        flow, ck = kernel_coords(c, scale)
        got = run_lookup(lib, fq, ft, flow, scale)
        want, M, Cn, _ = amt_restated.lookup(fq.double(), ft.double(), ck.double(), bound=True)
        assert (want == 0).all(0).any() and (ck[0] < 0).any() and (ck[0] > w - 1).any() and (ck[1] < 0).any() and (ck[1] > h - 1).any()
        _bounded(got, want, amt_restated.lookup_tolerance(D, M, Cn), f"lookup {name} direction {which} scale {scale}")
        if scale != 1.0:
            continue
        assert ((ck == torch.round(ck)).all(0) & (ck[0] >= 0) & (ck[0] < w) & (ck[1] >= 0) & (ck[1] < h)).any()
        # the reference's own fp32 output for the golden coordinates c: its coordinate slack, plus the ulp of c by which grid + (c - grid)
        # may miss c
        golden = np.load(os.path.join(golden_dir, "amt_lookup.npz"))
        iy, ix = cain_restated.sample_index(h, amt_restated.LOOKUP_STRIDE), cain_restated.sample_index(w, amt_restated.LOOKUP_STRIDE)
        ref = torch.from_numpy(golden[f"{name}_out{which}"]).double()
        slack = torch.zeros_like(want)
        for lvl in range(amt_restated.LEVELS):
            cabs = c.abs().amax(0) / 2 ** lvl
            slack[lvl * 49:(lvl + 1) * 49] = 2 * (amt_restated.coord_slack(cabs, max(h >> lvl, w >> lvl)) + 2 * U * cabs)[None]
        tol = 2 * amt_restated.lookup_tolerance(D, M, Cn) + slack * Cn          # both sides round
        _bounded(got[:, iy][:, :, ix], ref, tol[:, iy][:, :, ix], f"lookup {name} direction {which} vs the reference")


@pytest.mark.parametrize("h,w,D", [(17, 19, 12), (16, 33, 84)])
def test_corr_lookup_sees_every_summand(lib, h, w, D):
    """Positive features, and level-0 fractions in [0.25, 0.75] so that every corner weighs at least 1/16: at level 0 every summand of
    every element is larger than the bound, so one dropped corner, tap or channel would break it (min_term of tests/ref_ops_restated.py).
    A dropped channel or a wrong tap order at a coarser level moves those elements by as much."""
    g = torch.Generator().manual_seed(h * w + D)
    fq, ft = torch.rand(D, h, w, generator=g) + 0.5, torch.rand(D, h, w, generator=g) + 0.5
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    c = torch.stack([xs, ys]) + torch.randint(-5, 6, (2, h, w), generator=g).float() + 0.25 + 0.5 * torch.rand(2, h, w, generator=g)
    flow, ck = kernel_coords(c, 1.0)
    got = run_lookup(lib, fq, ft, flow, 1.0)
    want, M, Cn, mn = amt_restated.lookup(fq.double(), ft.double(), ck.double(), bound=True)
    tol = amt_restated.lookup_tolerance(D, M, Cn)
    _bounded(got, want, tol, f"lookup positive {h}x{w} D{D}")
    lvl0 = slice(0, 49)
    live = M[lvl0] > 0
    assert live.any() and (mn[lvl0][live] > tol[lvl0][live]).all(), "a summand is below the tolerance; the case cannot see a dropped one"


def test_corr_lookup_at_1080p_size(lib):
    """Both directions of one lookup at the 1/8 map of a padded 1080p pair (136x240, D = 84: AMT-S) written side by side into the 392
    channels convc1 reads; every element against the float64 restatement on the device.  32 640 workgroups; the buffers the lookup needs
    are the two pooled pyramids, 7.2 MB, where the reference's level-0 volume alone is 4 261 478 400 bytes."""
    h, w, D = 136, 240, 84
    g = torch.Generator().manual_seed(5)
    f = [torch.randn(h, w, D, generator=g).cuda() for _ in range(2)]
    flows = [(torch.randn(h, w, 2, generator=g) * 4).cuda() for _ in range(2)]
    pooled = [torch.empty(pooled_floats(h, w, D), device="cuda") for _ in range(2)]
    assert sum(p.numel() for p in pooled) * 4 == 7197120 and 4 * (h * w) ** 2 == 4261478400
    out = torch.full((h * w, 2 * PLANES), NAN, device="cuda")
    scales = (2.0, 1.0 / (1.0 - 0.5))
    for k in range(2):
        _check(lib.vfi_amt_pool_features(ptr(f[k]), h, w, D, ptr(pooled[k]), None), "vfi_amt_pool_features")
    for k in range(2):      # direction k: queries of frame k against frame 1 - k
        _check(lib.vfi_amt_corr_lookup(ptr(f[k]), ptr(f[1 - k]), ptr(pooled[1 - k]), ptr(flows[k]), 2, C.c_float(scales[k]), h, w, D,
                                       C.c_void_p(out.data_ptr() + 4 * PLANES * k), 2 * PLANES, None), "vfi_amt_corr_lookup")
    torch.cuda.synchronize()
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32, device="cuda"), torch.arange(w, dtype=torch.float32, device="cuda"), indexing="ij")
    for k in range(2):
        ck = torch.stack([xs, ys]) + flows[k].permute(2, 0, 1) * torch.tensor(scales[k], dtype=torch.float32, device="cuda")
        want, M, Cn, _ = amt_restated.lookup(f[k].permute(2, 0, 1).double(), f[1 - k].permute(2, 0, 1).double(), ck.double(), bound=True)
        got = out[:, PLANES * k:PLANES * (k + 1)].reshape(h, w, PLANES).permute(2, 0, 1)
        _bounded(got, want, amt_restated.lookup_tolerance(D, M, Cn), f"lookup 136x240 direction {k}")


def test_lookup_refuses_small_maps(lib):
    from cfi_amd import _lib

    x = torch.zeros(16 * 16 * 8, device="cuda")
    assert lib.vfi_amt_corr_lookup(ptr(x), ptr(x), ptr(x), ptr(x), 2, C.c_float(1.0), 15, 16, 8, ptr(x), PLANES, None) != 0
    assert "at least 16" in _lib.last_error()
    assert lib.vfi_amt_pool_features(ptr(x), 16, 12, 8, ptr(x), None) != 0 and "at least 16" in _lib.last_error()


# ---- conv7x7 -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("act", [0, 1, 3])
@pytest.mark.parametrize("N,H,W", [(1, 8, 8), (2, 9, 13), (1, 33, 47)])
@pytest.mark.parametrize("Cin,Cout", [(4, 40), (15, 30), (30, 3)])
def test_conv7x7_vs_float64(lib, Cin, Cout, N, H, W, act):
    g = torch.Generator().manual_seed(Cin * 1000 + Cout * 10 + H + act)
    x = torch.rand(N, H, W, Cin, generator=g) * 2 - 1
    w = (torch.rand(Cout, Cin, 7, 7, generator=g) * 2 - 1) / (49 * Cin) ** 0.5
    b = torch.rand(Cout, generator=g) - 0.5
    slopes = torch.rand(Cout, generator=g) * 0.5
    in_cs, out_cs = Cin + 3, Cout + 5
    xd = torch.full((N * H * W + 2, in_cs), NAN, device="cuda")          # channels beyond Cin are NaN: never read
    xd[1:1 + N * H * W, :Cin] = x.reshape(-1, Cin).cuda()
    out = torch.full((N * H * W + 2, out_cs), NAN, device="cuda")
    wd, bd, sd = pack7x7(w).cuda(), b.cuda(), slopes.cuda()              # held until the kernel has run
    _check(lib.vfi_conv7x7(ptr(xd[1]), in_cs, ptr(wd), ptr(bd), ptr(sd) if act == 3 else None, C.c_float(0.1), act, Cin, Cout, ptr(out[1]),
                           out_cs, N, H, W, None), "vfi_conv7x7")
    torch.cuda.synchronize()
    assert torch.isnan(out[0]).all() and torch.isnan(out[-1]).all() and torch.isnan(out[:, Cout:]).all(), "stray write"
    xn = x.permute(0, 3, 1, 2).double()
    want = F.conv2d(xn, w.double(), b.double(), padding=3)
    M = F.conv2d(xn.abs(), w.double().abs(), b.double().abs(), padding=3)
    if act == 1:
        want = F.leaky_relu(want, 0.1)
    elif act == 3:
        want = F.prelu(want, slopes.double())
    got = out[1:1 + N * H * W, :Cout].reshape(N, H, W, Cout).permute(0, 3, 1, 2).cpu()
    _bounded(got, want, (49 * Cin + 3) * U * M, f"conv7x7 {Cin}->{Cout} {N}x{H}x{W} act {act}")


# ---- combine -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nf", [3, 5])
@pytest.mark.parametrize("Hp,Wp,H,W,top,left", [(16, 16, 16, 16, 0, 0), (33, 47, 30, 41, 2, 5)])
def test_combine_vs_float64(lib, nf, Hp, Wp, H, W, top, left):
    g = torch.Generator().manual_seed(nf * 100 + Hp)
    img = torch.rand(2, 3, Hp, Wp, generator=g) - 0.5
    fin = torch.randn(8 * nf, Hp, Wp, generator=g)
    fin[:4 * nf] *= 8.0                                                  # flows that leave the frame
    fin[:4 * nf:7] = torch.round(fin[:4 * nf:7])                         # and some exactly on pixels
    mean = torch.tensor([0.4375])
    img_cs, fin_cs, out_cs = 4, 8 * nf + 3, 3 * nf + 2
    imd = torch.full((2, Hp * Wp, img_cs), NAN, device="cuda")
    imd[..., :3] = img.permute(0, 2, 3, 1).reshape(2, -1, 3).cuda()
    fd = torch.full((Hp * Wp, fin_cs), NAN, device="cuda")
    fd[:, :8 * nf] = fin.permute(1, 2, 0).reshape(-1, 8 * nf).cuda()
    md = mean.cuda()
    warps = torch.full((Hp * Wp + 1, out_cs), NAN, device="cuda")
    _check(lib.vfi_amt_combine_warps(ptr(imd[0]), ptr(imd[1]), img_cs, ptr(fd), fin_cs, ptr(md), nf, ptr(warps), out_cs, Hp, Wp, None),
           "vfi_amt_combine_warps")
    torch.cuda.synchronize()
    assert torch.isnan(warps[-1]).all() and torch.isnan(warps[:, 3 * nf:]).all(), "stray write"
    i64, f64 = img.double(), fin.double()[None]
    want = amt_restated.combine_warps(i64[0:1], i64[1:2], f64[:, :2 * nf], f64[:, 2 * nf:4 * nf], f64[:, 4 * nf:5 * nf], f64[:, 5 * nf:], mean.double())
    res_abs = f64[:, 5 * nf:].abs()
    flow_abs = torch.maximum(f64[:, :2 * nf].abs().reshape(nf, 2, Hp, Wp).amax(1), f64[:, 2 * nf:4 * nf].abs().reshape(nf, 2, Hp, Wp).amax(1))
    shift = 6 * U * (max(Hp, Wp) + flow_abs)                             # [nf,Hp,Wp] pixels, per axis
    tol = 24 * U * (0.5 + 0.4375 + res_abs) + (4 * 0.5 * 2 * shift).repeat_interleave(3, 0)[None]
    got = warps[:Hp * Wp, :3 * nf].reshape(Hp, Wp, 3 * nf).permute(2, 0, 1)[None].cpu()
    _bounded(got, want, tol, f"combine warps n{nf} {Hp}x{Wp}")
    assert float(tol.max()) < 2e-4

    comb = torch.randn(Hp, Wp, 3, generator=g) * 0.3
    cd = torch.full((Hp * Wp, 4), NAN, device="cuda")
    cd[:, :3] = comb.reshape(-1, 3).cuda()
    out = torch.full((H * W + 1, 3), NAN, device="cuda")
    _check(lib.vfi_amt_combine_out(ptr(warps), out_cs, ptr(cd), 4, nf, ptr(out), Hp, Wp, top, left, H, W, None), "vfi_amt_combine_out")
    torch.cuda.synchronize()
    assert torch.isnan(out[-1]).all(), "stray write"
    wr = warps[:Hp * Wp, :3 * nf].reshape(Hp, Wp, nf, 3).cpu().double()      # the tail on the kernel's own warps
    pre = wr.mean(2) + comb.double()
    want_o = pre.clamp(0, 1)[top:top + H, left:left + W]
    tol_o = ((nf + 3) * U * (wr.abs().sum(2) / nf + comb.double().abs()))[top:top + H, left:left + W]
    _bounded(out[:H * W].reshape(H, W, 3).cpu(), want_o, tol_o, f"combine out n{nf} {H}x{W}")
    assert (want_o == 0).any() and (want_o == 1).any() and ((want_o > 0) & (want_o < 1)).any()


_RESTATED = {}


def restated64(variant, shape_name):
    """the float64 restatement of a forward golden case at NET_TS, computed once on the device and shared: [2,3,h,w] on the host"""
    key = (variant, shape_name)
    if key not in _RESTATED:
        f0, f1 = frames_of(shape_name)
        sd = {k: v.cuda() for k, v in amt_restated.state_dict64(variant).items()}
        with torch.no_grad():
            _RESTATED[key] = amt_restated.amt_forward(sd, variant, f0.double().cuda(), f1.double().cuda(), NET_TS).cpu()
    return _RESTATED[key]


# ---- the kernels inside the forward they were written for ---------------------------------------------------------------------------

class KernelOps:
    """amt_restated.amt_forward's ops: the lookup, every 7x7 layer and both halves of multi_flow_combine run on the HIP kernels (NHWC on the
    device, between NaN guards where run_lookup provides them); everything else stays the host's torch restatement."""

    def __init__(self, lib):
        self.lib, self.calls = lib, {"lookup": 0, "conv7x7": 0, "combine_warps": 0, "combine_out": 0}

    @staticmethod
    def _nhwc(x, cs=None):
        _, c, h, w = x.shape
        buf = torch.full((h * w, cs or c), NAN, device="cuda")
        buf[:, :c] = x[0].permute(1, 2, 0).reshape(h * w, c).cuda()
        return buf

    def lookup(self, fq, ft, flow, scale):
        self.calls["lookup"] += 1
        return run_lookup(self.lib, fq.contiguous(), ft.contiguous(), flow.contiguous(), scale)

    def conv7x7(self, x, w, b, act, slopes):
        self.calls["conv7x7"] += 1
        _, cin, h, wd = x.shape
        cout = w.shape[0]
        xd, out = self._nhwc(x), torch.full((h * wd, cout), NAN, device="cuda")
        wp, bd, sl = pack7x7(w).cuda(), b.cuda(), slopes.cuda() if slopes is not None else None
        _check(self.lib.vfi_conv7x7(ptr(xd), cin, ptr(wp), ptr(bd), ptr(sl) if sl is not None else None, C.c_float(0.1), act, cin, cout, ptr(out),
                                    cout, 1, h, wd, None), "vfi_conv7x7")
        torch.cuda.synchronize()
        return out.reshape(h, wd, cout).permute(2, 0, 1)[None].cpu()

    def combine_warps(self, img0, img1, fin, mean, nf):
        self.calls["combine_warps"] += 1
        _, _, hp, wp = img0.shape
        i0, i1, fd, md = self._nhwc(img0, 4), self._nhwc(img1, 4), self._nhwc(fin), mean.reshape(1).cuda()
        out = torch.full((hp * wp, 3 * nf), NAN, device="cuda")
        _check(self.lib.vfi_amt_combine_warps(ptr(i0), ptr(i1), 4, ptr(fd), 8 * nf, ptr(md), nf, ptr(out), 3 * nf, hp, wp, None), "vfi_amt_combine_warps")
        torch.cuda.synchronize()
        return out.reshape(hp, wp, 3 * nf).permute(2, 0, 1)[None].cpu()

    def combine_out(self, wr, comb, nf, top, left, H, W):
        self.calls["combine_out"] += 1
        _, _, hp, wp = wr.shape
        wd, cd = self._nhwc(wr), self._nhwc(comb, 4)
        out = torch.full((H * W, 3), NAN, device="cuda")
        _check(self.lib.vfi_amt_combine_out(ptr(wd), 3 * nf, ptr(cd), 4, nf, ptr(out), hp, wp, top, left, H, W, None), "vfi_amt_combine_out")
        torch.cuda.synchronize()
        return out.reshape(H, W, 3).permute(2, 0, 1)[None].cpu()


@pytest.mark.parametrize("variant", ["S", "L"])
@pytest.mark.parametrize("shape_name", ["128x128", "144x208", "130x200"])
def test_forward_with_the_kernels_in_place(lib, variant, shape_name, golden_dir, oracle_threads):
    """The fp32 forward with the lookup, the 7x7 layers and multi_flow_combine on the HIP kernels, the rest on the host's torch: per-pixel
    |d| <= 1e-3 against the reference's own forward (tests/golden/amt_net.npz) and, for every pixel, against the float64 restatement, at
    t = 0.5 and 0.2.  This pins what a kernel test cannot: the order of the 392 lookup channels convc1 reads, which flow and scale go with
    which direction, the 7x7 weight pack, the layout of comb_block's input and the un-pad offsets."""
    from cfi_amd import amt_spec

    golden = np.load(os.path.join(golden_dir, "amt_net.npz"))
    f0, f1 = frames_of(shape_name)
    sd = amt_spec.seeded_state_dict(variant, SEED)
    ops = KernelOps(lib)
    with torch.no_grad():
        got = amt_restated.amt_forward(sd, variant, f0, f1, NET_TS, ops=ops)
    want = restated64(variant, shape_name)
    n7 = 3 + (2 if variant == "L" else 0)
    assert ops.calls == {"lookup": 6 * len(NET_TS), "conv7x7": n7 * len(NET_TS), "combine_warps": len(NET_TS), "combine_out": len(NET_TS)}
    assert torch.isfinite(got).all()
    for i, t in enumerate(NET_TS):
        d, sums_ok = cain_restated.compare(got[i].permute(1, 2, 0), golden, f"{variant}_{shape_name}_t{t}_", NET_STRIDE, TOL)
        dr = float((got[i].double() - want[i]).abs().max())
        print(f"AMT-{variant} {shape_name} t={t}: sampled max |d| vs the reference {d:.3e}, max |d| vs the float64 restatement {dr:.3e}")
        assert d <= TOL and sums_ok and dr <= TOL, describe_diff(got[i].double(), want[i], f"AMT-{variant} {shape_name} t={t}", chan_last=False)


# ---- the network object and the node -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def engine_of(lib):
    """variant -> AmtEngine on the seeded weights, built once per variant and closed (weights and workspace freed) after the file's tests"""
    from cfi_amd import amt, amt_spec

    engines = {}

    def get(variant):
        if variant not in engines:
            engines[variant] = amt.AmtEngine(amt_spec.seeded_state_dict(variant, SEED))
        return engines[variant]

    yield get
    for e in engines.values():
        e.close()
    _RESTATED.clear()


def hwc(f):
    return f[0].permute(1, 2, 0).contiguous().cuda()


@pytest.mark.parametrize("variant", ["S", "L"])
@pytest.mark.parametrize("shape_name", ["128x128", "144x208", "130x200"])
def test_object_forward_matches_the_reference_and_the_restatement(lib, engine_of, variant, shape_name, golden_dir):
    """vfi_amt_forward (layer objects, instance norm, 7x7 stride-2 stems, channel windows, resizes, workspace) against the reference's own
    forward (tests/golden/amt_net.npz) and, for every pixel, the float64 restatement on the device: |d| <= 1e-3, t = 0.5 and 0.2 in ONE call."""
    golden = np.load(os.path.join(golden_dir, "amt_net.npz"))
    f0, f1 = frames_of(shape_name)
    eng = engine_of(variant)
    got = eng.forward(hwc(f0), hwc(f1), NET_TS).cpu()
    want = restated64(variant, shape_name)
    assert torch.isfinite(got).all() and got.shape == (len(NET_TS),) + tuple(f0.shape[2:]) + (3,)
    for i, t in enumerate(NET_TS):
        d, sums_ok = cain_restated.compare(got[i], golden, f"{variant}_{shape_name}_t{t}_", NET_STRIDE, TOL)
        dr = float((got[i].double() - want[i].permute(1, 2, 0)).abs().max())
        print(f"AMT-{variant} object {shape_name} t={t}: sampled max |d| vs the reference {d:.3e}, max |d| vs the float64 restatement {dr:.3e}")
        assert d <= TOL and sums_ok and dr <= TOL, describe_diff(got[i].double(), want[i].permute(1, 2, 0), f"AMT-{variant} {shape_name} t={t}")
    assert 0 < eng.workspace_bytes() < 1 << 30


@pytest.mark.parametrize("variant", ["S", "L"])
def test_per_pair_reuse_is_exact_and_does_not_leak(lib, engine_of, variant):
    """forward(ts = [0.25, 0.5, 0.75]) is bit-identical to three single-timestep calls, and a call with another pair in between leaves no
    trace: what is computed once per pair (pad, mean, encoders, pooled maps) belongs to that call alone."""
    a0, a1 = (hwc(f) for f in frames_of("130x200"))
    b0, b1 = a1.flip(0).contiguous(), a0.flip(1).contiguous()
    eng = engine_of(variant)
    ts = [0.25, 0.5, 0.75]
    together = eng.forward(a0, a1, ts).clone()
    other = eng.forward(b0, b1, [0.5]).clone()
    single = torch.cat([eng.forward(a0, a1, [t]) for t in ts])
    assert torch.equal(together, single)
    assert float((together[1] - other[0]).abs().max()) > 1e-2, "the second pair must give another frame"
    assert torch.equal(eng.forward(b0, b1, [0.5]), other) and torch.equal(eng.forward(a0, a1, ts), together)
    assert float((together[0] - together[2]).abs().max()) > 1e-3, "the timestep must matter"


def test_size_guard_of_the_object(lib, engine_of):
    eng = engine_of("S")
    f = torch.zeros(100, 300, 3, device="cuda")
    before = eng.workspace_bytes()
    with pytest.raises(ValueError, match="at least 128"):
        eng.forward(f, f, [0.5])
    from cfi_amd import _lib
    rc = eng.lib.vfi_amt_forward(eng.handle, ptr(f), ptr(f), 3, 100, 300, (C.c_float * 1)(0.5), 1, ptr(f), None)      # refused before any launch
    assert rc != 0 and "at least 128" in _lib.last_error() and eng.workspace_bytes() == before


@pytest.mark.parametrize("case", ["m2", "m3", "list", "skip", "rgba", "odd"])
def test_node_matches_the_reference_node(lib, engine_of, case, golden_dir, monkeypatch):
    """AMT_VFI.vfi on the device against the reference node's own output (tests/golden/amt_node.npz): <= 1e-3 per sampled pixel and line sum"""
    golden = np.load(os.path.join(golden_dir, "amt_node.npz"))
    amt_restated.check_node_case(case, amt_restated.run_node(case, monkeypatch, engine_of), golden)


def test_1080p_call_builds_no_volume(lib, engine_of):
    """One 1080x1920 AMT-S call at 2x: finite, within 1e-3 of the float64 restatement on the device on a strided sample of rows and
    columns (the restatement is evaluated whole; the sample bounds the comparison's host traffic), and the object's whole workspace is
    smaller than ONE level-0 correlation volume of the reference at this size: no volume exists."""
    H, W = 1080, 1920
    f = cain_restated.seeded_frames(2, H, W, 3, 77).cuda()
    eng = engine_of("S")
    got = eng.forward(f[0].contiguous(), f[1].contiguous(), [0.5])[0]
    torch.cuda.synchronize()
    ws = eng.workspace_bytes()
    eng.release_workspace()
    assert eng.workspace_bytes() == 0
    print(f"AMT-S 1080p workspace: {ws} bytes ({ws / 2 ** 20:.0f} MiB); one level-0 volume of the reference: {4 * (136 * 240) ** 2} bytes")
    assert 0 < ws < 4 * (136 * 240) ** 2 == 4261478400
    assert torch.isfinite(got).all()
    sd = {k: v.cuda() for k, v in amt_restated.state_dict64("S").items()}
    with torch.no_grad():
        want = amt_restated.amt_forward(sd, "S", f[0:1].permute(0, 3, 1, 2).double(), f[1:2].permute(0, 3, 1, 2).double(), [0.5])[0].permute(1, 2, 0)
    iy, ix = torch.arange(0, H, 7, device="cuda"), torch.arange(0, W, 11, device="cuda")
    d = float((got[iy][:, ix].double() - want[iy][:, ix]).abs().max())
    print(f"AMT-S 1080p: max |d| vs the float64 restatement on the sample {d:.3e}")
    assert d <= TOL
