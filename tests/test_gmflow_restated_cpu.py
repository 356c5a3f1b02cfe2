"""CPU: everything about tests/gmflow_restated.py that needs no device.

  * the restatements against oracle/gmfss_oracle.py (what tests/test_gpu_attention.py and tests/test_gpu_gmfss_ops.py compare with):
    window attention and local propagation in float64 at 1e-11, local match against the oracle's fp32 grid_sample form within the
    restated bound of the per-pixel body (the oracle computes in fp32); the restated label map against cfi_amd.gmfss.shift_labels;
  * the conditions the case tables rely on, from the reference alone: mn > tol for every positive-input case, the planted rows
    overflow / underflow without the maximum, the rising-maximum row rises in every block, the one-key range holds one key, the
    restated split rule gives the range count each case id states, the planted displacements carry > 0.99 of the softmax mass;
  * every wrong restatement differs from the right one by more than both bounds together, in every case it is listed for;
  * att_row's float division (csrc/attention.hip) equals l // ww for every window width 1..2048 and every l the kernel can see;
  * the host build of the bodies (tests/hostcheck) through the same cases and bounds for vfi_layernorm*, vfi_local_match and
    vfi_local_propagate."""
import re

import numpy as np
import pytest
import torch

import gmflow_restated as gr
import hostcheck
from oracle import gmfss_oracle as G


@pytest.fixture(scope="module")
def lib():
    return hostcheck.load()


def test_case_ids_are_unique_and_cover_every_entry_point():
    ids = [c.id for c in gr.ALL_CASES]
    assert len(ids) == len(set(ids))
    assert {c.op for c in gr.ALL_CASES} == {"attention", "window_attention", "local_match", "local_propagate", "layernorm"}
    assert {m for _, m in gr.NEGATIVE} == {m for ms in gr.MUTATIONS.values() for m in ms}, "a wrong restatement applies to no case"


# ---------------------------------------------------------------------------------------------------------------- oracle ties

@pytest.mark.parametrize("shape", gr.WINDOW_SHAPES[:5], ids=str)
def test_window_attention_restated_is_the_oracles(shape):
    B, h, w, K, sh, sw = shape
    assert (sh, sw) == ((h // K) // 2 if sh else 0, (w // K) // 2 if sw else 0), "the oracle shifts by half a window"
    g = torch.Generator().manual_seed(h + w)
    q, k, v = (torch.randn(B, h * w, 128, generator=g, dtype=torch.float64) for _ in range(3))
    shifted = bool(sh or sw)
    mask = G._shift_mask(h, w, h // K, w // K).double() if shifted else None
    want = G._window_attention(q, k, v, K, shifted, h, w, mask).view(B, h, w, 128)
    labels = gr.shift_labels_restated(h, w, K, sh, sw) if shifted else None
    tw = lambda t: gr.to_windows(t.view(B, h, w, 128), K, sh, sw)
    o = gr.attention_f64(tw(q), tw(k), tw(v), 1.0 / 128 ** 0.5, labels, K * K, 1)[0]
    assert (gr.from_windows(o, B, h, w, K, sh, sw) - want).abs().max().item() <= 1e-11


@pytest.mark.parametrize("shape", gr.WINDOW_SHAPES, ids=str)
def test_label_map_restated_is_the_engines(shape):
    from cfi_amd.gmfss import shift_labels

    _, h, w, K, _, _ = shape
    wh, ww = h // K, w // K
    if wh // 2 and ww // 2:
        assert torch.equal(gr.shift_labels_restated(h, w, K, wh // 2, ww // 2), shift_labels(h, w, K))
    # and the -100 mask the labels stand for is the reference construction's (oracle._shift_mask)
    if wh // 2 and ww // 2:
        lab = gr.shift_labels_restated(h, w, K, wh // 2, ww // 2)
        mask = torch.where(lab[:, :, None] != lab[:, None, :], -100.0, 0.0)
        assert torch.equal(mask, G._shift_mask(h, w, wh, ww).permute(0, 2, 1).contiguous()) and torch.equal(mask, mask.permute(0, 2, 1))


@pytest.mark.parametrize("shape", gr.LM_SHAPES, ids=str)
def test_local_match_restated_is_the_oracles(shape):
    N, H, W = shape
    g = torch.Generator().manual_seed(H * W)
    f0, f1 = torch.randn(N, H, W, 128, generator=g), torch.randn(N, H, W, 128, generator=g)
    want, tol = gr.local_match_f64(f0.double(), f1.double(), torch.zeros(N, H, W, 2, dtype=torch.float64), 4, True)[:2]
    got = G.local_match(f0.permute(0, 3, 1, 2).contiguous(), f1.permute(0, 3, 1, 2).contiguous(), 4).permute(0, 2, 3, 1).double()
    assert bool(((got - want).abs() <= tol).all()), (got - want).abs().max().item()


@pytest.mark.parametrize("shape", [(c.p["N"], c.p["H"], c.p["W"]) for c in gr.LP_CASES[:5]], ids=str)
def test_local_propagate_restated_is_the_oracles(shape):
    N, H, W = shape
    g = torch.Generator().manual_seed(H + W)
    f0 = torch.randn(N, 128, H, W, generator=g, dtype=torch.float64)
    flow = torch.randn(N, 2, H, W, generator=g, dtype=torch.float64) * 3
    sd = {f"feature_flow_attn.{n}": torch.randn(*s, generator=g, dtype=torch.float64) * 0.1
          for n, s in (("q_proj.weight", (128, 128)), ("q_proj.bias", (128,)), ("k_proj.weight", (128, 128)), ("k_proj.bias", (128,)))}
    want = G.propagate(sd, f0, flow, 1).permute(0, 2, 3, 1)
    tok = f0.permute(0, 2, 3, 1)
    q = torch.nn.functional.linear(tok, sd["feature_flow_attn.q_proj.weight"], sd["feature_flow_attn.q_proj.bias"])
    k = torch.nn.functional.linear(tok, sd["feature_flow_attn.k_proj.weight"], sd["feature_flow_attn.k_proj.bias"])
    assert (gr.local_prop_f64(q, k, flow.permute(0, 2, 3, 1))[0] - want).abs().max().item() <= 1e-11


def test_layernorm_restated_is_torchs():
    g = torch.Generator().manual_seed(3)
    x, ga, be = torch.randn(7, 65, generator=g, dtype=torch.float64), torch.randn(65, generator=g, dtype=torch.float64), torch.randn(65, generator=g, dtype=torch.float64)
    want = torch.nn.functional.layer_norm(x, (65,), ga, be, gr._f32(1e-5))
    assert (gr.layernorm_f64(x, ga, be, None)[0] - want).abs().max().item() <= 1e-11


# ---------------------------------------------------------------------------------------------------------------- conditions

@pytest.mark.parametrize("case", [c for c in gr.ALL_CASES if c.p["kind"] == "pos"], ids=lambda c: c.id)
def test_every_summand_of_a_positive_case_is_above_the_bound(case):
    seen = 0
    for e in gr.expectation(case):
        if e.get("mn") is not None:
            assert bool((e["mn"] > e["tol"]).all()), case.id
            seen += 1
    assert seen or case.p.get("Lk") == 1


def _planted_logits(case):
    from types import SimpleNamespace

    P = SimpleNamespace(**case.p, alpha=gr._f32(1.0 / 128 ** 0.5))
    q, k, _ = gr.attention_inputs(P)
    return torch.matmul(q.double(), k.double().transpose(1, 2)) * P.alpha


@pytest.mark.parametrize("case", [c for c in gr.ATT_CASES if c.p["kind"] == "planted" and not c.p["period"]], ids=lambda c: c.id)
def test_planted_rows_do_what_they_are_planted_for(case):
    t = _planted_logits(case).float()
    Lq, Lk = case.p["Lq"], case.p["Lk"]
    nblk = -(-Lk // 32)
    assert torch.isinf(torch.exp(t[:, 0]).sum(-1)).all() and (t[:, 0].amax(-1) > 250).all(), "row 0 does not overflow without the maximum"
    if Lq > 1:
        assert (torch.exp(t[:, 1]).sum(-1) == 0).all(), "row 1 does not underflow without the maximum"
    if Lq > 3 and nblk > 1:
        assert (t[:, 2].argmax(-1) < 32).all() and (t[:, 3].argmax(-1) // 32 == nblk - 1).all()
    if Lq > 4:
        pad = torch.cat([t[:, 4], torch.full((t.shape[0], nblk * 32 - Lk), -float("inf"))], 1).view(-1, nblk, 32).amax(-1)
        assert bool((pad[:, 1:] > pad[:, :-1]).all()), "the running maximum does not rise in every block"


def test_split_cases_state_the_split_that_runs():
    seen = set()
    for c in gr.ATT_CASES:
        m = re.search(r"split(\d+|-automatic)-runs(\d+)", c.id)
        if not m:
            assert c.p["ks"] == 0 and c.p["ks_ran"] == 1 and -(-c.p["Lk"] // 32) < 16, c.id      # the automatic rule needs 16 blocks to split
            continue
        if m.group(1) == "-automatic":      # 16 blocks, one workgroup: min(CUs, 16 / 8, 8) = 2 on any device with two CUs
            assert c.p["ks"] == 0 and c.p["Lk"] == 512 and c.p["nb"] * -(-c.p["Lq"] // 128) == 1 and c.p["ks_ran"] == 2
            continue
        assert c.p["ks"] == int(m.group(1)) and gr.split_rule(c.p["Lk"], c.p["ks"])[0] == int(m.group(2)) == c.p["ks_ran"], c.id
        seen.add(c.p["ks_ran"])
        ks, per = gr.split_rule(c.p["Lk"], c.p["ks"])
        nblk = -(-c.p["Lk"] // 32)
        assert (ks - 1) * per < nblk <= ks * per, "an empty range"
        if "onekey" in c.id:
            assert c.p["Lk"] - (ks - 1) * per * 32 == 1
    assert {2, 3, 5, 7, 8} <= seen
    assert gr.split_rule(257, 8) == (5, 2) and gr.split_rule(256, 8) == (8, 1) and gr.split_rule(33, 2) == (2, 1) and gr.split_rule(31, 8) == (1, 1)


@pytest.mark.parametrize("case", [c for c in gr.LM_CASES if c.p["kind"] == "planted"], ids=lambda c: c.id)
def test_planted_displacement_carries_the_softmax(case):
    from types import SimpleNamespace

    P = SimpleNamespace(**case.p)
    f0, f1, prior = gr.local_match_inputs(P)
    want, tol, p, o, delta, _ = gr.local_match_f64(f0.double(), f1.double(), prior.double(), 4, False)
    dx, dy = P.d
    assert dx != dy and max(abs(dx), abs(dy)) <= 4
    j = (dy + 4) * 9 + dx + 4
    inside = gr.planted_inside(P)
    assert inside.any() and bool((p[..., j][inside] > 0.99).all())
    assert bool(((delta[inside] - torch.tensor([dx, dy], dtype=torch.float64)).abs() < 0.05).all())


# ---------------------------------------------------------------------------------------------------------------- mutations

@pytest.mark.parametrize("case,mut", gr.NEGATIVE, ids=lambda v: v.id if isinstance(v, gr.Case) else v.replace(" ", "-"))
def test_wrong_restatement_is_further_than_both_bounds(case, mut):
    right, wrong = gr.expectation(case), gr.expectation(case, mut)
    far = False
    for a, b in zip(right, wrong):
        far = far or bool(((a["want"] - b["want"]).abs() > a["tol"] + b["tol"]).any())
    assert far, f"{case.id}: '{mut}' stays within the bounds everywhere"


# ---------------------------------------------------------------------------------------------------------------- att_row

def test_att_row_division_is_exact():
    """csrc/attention.hip att_row: ly = (int)((l + 0.5f) * (1.0f / ww)) for every ww in 1..2048 and every l < min(2^20, 2048 ww)"""
    lf = np.arange(1 << 20, dtype=np.float32) + np.float32(0.5)
    li = np.arange(1 << 20, dtype=np.int32)
    for ww in range(1, 2049):
        n = min(1 << 20, 2048 * ww)
        inv = np.float32(1.0) / np.float32(ww)
        ly = (lf[:n] * inv).astype(np.int32)
        lx = li[:n] - ly * np.int32(ww)
        assert lx.min() >= 0 and lx.max() < ww, f"ww {ww}: first wrong l = {int(np.nonzero((lx < 0) | (lx >= ww))[0][0])}"


# ---------------------------------------------------------------------------------------------------------------- host bodies

@pytest.mark.parametrize("case", gr.HOST_CASES, ids=lambda c: c.id)
def test_case_on_the_host_build_of_the_bodies(lib, case):
    gr.run_case(lib, case, host=True)


@pytest.mark.parametrize("case,mut", [(c, m) for c, m in gr.NEGATIVE if c in gr.HOST_CASES], ids=lambda v: v.id if isinstance(v, gr.Case) else v.replace(" ", "-"))
def test_wrong_restatement_fails_on_the_host_result(lib, case, mut):
    with pytest.raises(AssertionError, match="outside the bound"):
        gr.run_case(lib, case, mut=mut, host=True)
