"""CPU: the float64 / exact restatements of tests/ref_ops_restated.py against the reference's own kernel outputs in
tests/golden/ref_ops_golden.npz (tools/make_golden_ops.py), under the same magnitude bound the GPU tests use; the distance transform
bit for bit.  The GPU tests of the ops backend (tests/test_gpu_ref_ops*.py) rest on these restatements."""
import os

import numpy as np
import pytest
import torch

import ref_ops_restated as rs


@pytest.fixture(scope="module")
def gold(golden_dir):
    d = np.load(os.path.join(golden_dir, "ref_ops_golden.npz"))
    return {k: torch.from_numpy(d[k]) for k in d.files}


def _assert_within(got, want, M, gamma, what):
    tol = rs.tolerance(M, gamma)
    d = (got.double() - want).abs()
    bad = ~(d <= tol)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {d.numel()} elements outside gamma*u*M; worst excess {(d - tol).max():.3e}"


@pytest.mark.parametrize("case", ["sepconv_k51", "sepconv_k5"])
def test_sepconv_restated_vs_golden(gold, case):
    ver = gold[f"{case}_ver"]
    want, M = rs.sepconv(gold[f"{case}_in"], ver, gold[f"{case}_hor"])
    _assert_within(gold[f"{case}_out"], want, M, rs.gamma_sepconv(ver.shape[1]), case)


@pytest.mark.parametrize("case,dil", [("adacof_f5", 1), ("adacof_f3d2", 2)])
def test_adacof_restated_vs_golden(gold, case, dil):
    w = gold[f"{case}_w"]
    Fs = int(round(w.shape[1] ** 0.5))
    want, M = rs.adacof(gold[f"{case}_in"], w, gold[f"{case}_oi"], gold[f"{case}_oj"], dil)
    _assert_within(gold[f"{case}_out"], want, M, rs.gamma_adacof(Fs), case)
    # the golden's offsets reach beyond the border and have both signs: the clamp and the extrapolating fraction are exercised
    assert (gold[f"{case}_oi"] < 0).any() and (gold[f"{case}_oi"].abs() > 2).any()


@pytest.mark.parametrize("case", ["corr_c32", "corr_c196"])
def test_correlation_restated_vs_golden(gold, case):
    a = gold[f"{case}_a"]
    want, M = rs.correlation(a, gold[f"{case}_b"])
    _assert_within(gold[f"{case}_out"], want, M, rs.gamma_correlation(a.shape[1]), case)


@pytest.mark.parametrize("case", ["edt_mask3", "edt_mask4"])
def test_edt_restated_bit_exact(gold, case):
    m = gold[case]
    m3 = m.squeeze(1) if m.dim() == 4 else m
    want = gold[f"{case}_out"].reshape(m3.shape)
    got = rs.batch_edt(m3)
    assert torch.equal(got, want)
    # the fp32 emulation (the path of non-binary masks) agrees with the int64 path on a 0/1 mask
    data, diam2 = rs.edt_data(m3)
    assert torch.equal(rs.edt_fp32(data, diam2), want)


def test_sensitivity_bound_is_tight_enough():
    """the tolerance the GPU edge tests use sits below one summand for operands in [0.5, 1] (weights in [0.5, 1] / K): a dropped
    or doubled tap or channel breaks the bound.  Here on a perturbed restatement, so the claim is checked without a GPU."""
    g = torch.Generator().manual_seed(0)
    K, Ho, Wo = 51, 3, 5
    x = 0.5 + 0.5 * torch.rand(1, 3, Ho + K - 1, Wo + K - 1, generator=g)
    ver = (0.5 + 0.5 * torch.rand(1, K, Ho, Wo, generator=g)) / K
    hor = (0.5 + 0.5 * torch.rand(1, K, Ho, Wo, generator=g)) / K
    out, M, mn = rs.sepconv(x, ver, hor, min_term=True)
    tol = rs.tolerance(M, rs.gamma_sepconv(K))
    assert (mn > tol).all()
    hor_dropped = hor.clone()
    hor_dropped[:, K - 1] = 0                            # the last horizontal tap missing
    dropped, _ = rs.sepconv(x, ver, hor_dropped)
    assert ((dropped - out).abs() > tol).all()

    a = 0.5 + 0.5 * torch.rand(1, 33, 6, 7, generator=g)
    b = 0.5 + 0.5 * torch.rand(1, 33, 6, 7, generator=g)
    out, M, mn = rs.correlation(a, b, min_term=True)
    tol = rs.tolerance(M, rs.gamma_correlation(33))
    inside = M > 0
    assert (mn[inside] > tol[inside]).all()
    short, _ = rs.correlation(a[:, :32], b[:, :32])      # the last channel missing (and / 32 instead of / 33)
    assert ((short * 32 / 33 - out).abs()[inside] > tol[inside]).all()


def test_edt_exact_paths_agree():
    """int64 path == fp32 emulation on binary masks below 2^24 (edges: empty, full, corner pixel); sqrt_rn is correctly rounded"""
    g = torch.Generator().manual_seed(1)
    for h, w in ((1, 1), (1, 7), (9, 1), (23, 37), (64, 65)):
        masks = torch.stack([torch.zeros(h, w), torch.ones(h, w), torch.zeros(h, w), (torch.rand(h, w, generator=g) > 0.9).float()])
        masks[2, h - 1, w - 1] = 1
        data, diam2 = rs.edt_data(masks)
        assert torch.equal(rs.edt_rows_exact(masks).float(), rs.edt_rows_fp32(data, diam2))
        got = rs.batch_edt(masks)
        assert torch.equal(got, rs.edt_fp32(data, diam2))
        assert torch.equal(got[0], torch.full((h, w), float(np.float32(np.sqrt(float(h * h + w * w))))))
        assert not got[1].any()
    v = np.arange(1 << 20, dtype=np.float32)
    s = rs.sqrt_rn(torch.from_numpy(v)).numpy().astype(np.float64)
    # correctly rounded: v lies inside the square of s's rounding interval
    up, dn = np.nextafter(s.astype(np.float32), np.float32(np.inf)), np.nextafter(s.astype(np.float32), np.float32(0))
    lo, hi = 0.5 * (s + dn.astype(np.float64)), 0.5 * (s + up.astype(np.float64))
    assert ((lo * lo <= v) & (v <= hi * hi)).all()
