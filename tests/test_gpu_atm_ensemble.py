"""-m gpu: ATM's multi-scale global-motion ensemble on the device (config.yaml's ``atm_ensemble`` key patched on where the Python side asks).

  1. vfi_atm_alignment_loss against a float64 evaluation of global_alignmentness, within a float64 rounding bound stated below, at coarse
     maps of 1x1, 1x2, 2x3 and 4x6 and factors 16 and 64, flows that leave the image in both signs; twice the same bits.
  2. vfi_atm_select_flow: every winner and the two ties, the resize against F.interpolate(align_corners=True) x factor in float64, the
     destination's other channels untouched, the record.
  3. The existing window attention, tap gather and strided convolutions at the smallest global maps the ensemble reaches (1x1, 1x2, 2x2
     tokens, window 12, shift 0 and 6), and the pad labels of another map (vfi_atm_window_attention_labels).
  4. The forward through AtmEngine, lite and base: every case of atm_ens_net.npz / atm_base_ens_net.npz <= 1e-3 per pixel against the golden
     and the float32 restatement, the chosen level, the losses within 1e-3 relative, twice the same bits, "ensemble where level 0 wins" ==
     "On" bit for bit, "On" unchanged by an ensemble call in between.
  5. The node on the 100x180 clip; the refusals of the new entry point before any launch."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import atm_ensemble_restated as E
import atm_restated as R
import cain_restated
import test_gpu_atm as lite      # the float64 attention and its bound, the strided-convolution check
from gpu_util import ptr

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
_ck, _stream, _report = lite._ck, lite._stream, lite._report


# ---- 1. the fused score ----------------------------------------------------------------------------------------------------------------

def _up64(m, size, factor):
    """upsample_flow in float64: [h,w,c] -> [1,c,H,W]"""
    return F.interpolate(m.double().permute(2, 0, 1)[None], size=size, mode="bilinear", align_corners=True) * factor


@pytest.mark.parametrize("f", [16, 64])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 2), (2, 3), (4, 6)])
def test_alignment_loss_against_float64(hip_lib, h, w, f):
    Hp, Wp = f * h, f * w                       # 2x3 at f = 16: rows of 48 pixels, no multiple of the workgroup's 256
    g = torch.Generator().manual_seed(100 * h + 10 * w + f)
    pair = torch.full((2, Hp, Wp, 8), float("nan"))
    pair[..., :3] = torch.rand((2, Hp, Wp, 3), generator=g)
    mo = torch.full((h, w, 8), float("nan"))
    mo[..., :4] = torch.randn((h, w, 4), generator=g) * 0.4           # x f: 0.4 of a coarse cell, i.e. 6 px at f = 16 and 26 px at f = 64
    mo[0, 0, :4] = torch.tensor([0.6 * w, -0.5 * h, -0.7 * w, 0.4 * h])      # x f: most of the frame away, both signs
    n = int(hip_lib.vfi_atm_alignment_scratch_floats(Hp, Wp))
    assert n == (Hp * Wp + 255) // 256
    dp, dm = pair.cuda(), mo.cuda()
    got = []
    for _ in range(2):
        scratch, loss = torch.full((n + 1,), float("nan"), device="cuda"), torch.full((2,), float("nan"), device="cuda")
        _ck(hip_lib.vfi_atm_alignment_loss(ptr(dp), 8, Hp, Wp, ptr(dm), 8, h, w, ptr(scratch), ptr(loss), _stream()), "vfi_atm_alignment_loss")
        torch.cuda.synchronize()
        assert torch.isfinite(scratch[:n]).all() and torch.isnan(scratch[n]) and torch.isnan(loss[1])
        got.append(loss[:1].cpu())
    assert torch.equal(got[0], got[1]), "two launches, two sums"
    fl = _up64(mo[..., :4], (Hp, Wp), f)
    imgs = pair[..., :3].double().permute(0, 3, 1, 2)
    w0, w1 = R.warp(imgs[0:1], fl[:, 0:2]), R.warp(imgs[1:2], fl[:, 2:4])
    term = (w0 - w1).abs().sum(1)[0]                                   # [Hp, Wp]
    want = term.mean() / 3
    # The bound.  Flow: the interpolation weights are off by 4 u of the source coordinate (<= h + w), the four products and three sums by
    # 8 u, all times f.  Coordinate: 8 u (|coordinate| + size) through the normalise / un-normalise round trip (as the synthesis test of
    # tests/test_gpu_atm.py) plus the flow's error; a bilinear tap of an image in [0, 1] moves by at most 1 per pixel and axis.  A pixel's
    # term: three channels of two warps, and 4 u of itself.  Sum: 8 tree levels + 2 wave steps in float32 (10 u of the sum), the rest in
    # double, the quotient and its rounding 2 u.
    vmax = float(mo[..., :4].abs().max())
    ferr = f * (4 * U * (h + w) + 8 * U) * vmax
    yy, xx = torch.meshgrid(torch.arange(Hp, dtype=torch.float64), torch.arange(Wp, dtype=torch.float64), indexing="ij")
    cerr = [8 * U * ((xx + fl[0, 2 * k]).abs() + Wp + (yy + fl[0, 2 * k + 1]).abs() + Hp) + 2 * ferr for k in (0, 1)]
    term_tol = 3 * (2 * cerr[0].clamp(max=1.0) + 2 * cerr[1].clamp(max=1.0) + 16 * U) + 4 * U * term
    tol = term_tol.mean() / 3 + 12 * U * want
    outside = float((w0 == 0).all(1).double().mean()), float((w1 == 0).all(1).double().mean())
    print(f"alignment loss {h}x{w} x{f}: {float(got[0]):.7f} vs float64 {float(want):.7f}, bound {float(tol):.3e}; outside {outside}")
    assert min(outside) > 0.02, "the case has flows that leave the image, for both frames"
    _report(f"alignment loss {h}x{w} x{f}", (got[0].double() - want).abs(), tol.reshape(1))


def test_alignment_loss_refuses_bad_arguments(hip_lib):
    from cfi_amd import _lib

    z = torch.zeros(64, device="cuda")
    assert hip_lib.vfi_atm_alignment_loss(ptr(z), 8, 32, 48, ptr(z), 8, 2, 2, ptr(z), ptr(z), _stream()) != 0 and "one factor" in _lib.last_error()
    assert hip_lib.vfi_atm_alignment_loss(None, 8, 32, 32, ptr(z), 8, 2, 2, ptr(z), ptr(z), _stream()) != 0
    assert hip_lib.vfi_atm_alignment_loss(ptr(z), 8, 32, 32, ptr(z), 3, 2, 2, ptr(z), ptr(z), _stream()) != 0


# ---- 2. the choice ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("losses,level", [((0.1, 0.2, 0.3), 0), ((0.3, 0.1, 0.2), 1), ((0.3, 0.2, 0.1), 2), ((0.1, 0.1, 0.2), 0), ((0.2, 0.1, 0.1), 1),
                                          ((0.1, 0.2, 0.1), 0), ((0.1, 0.1, 0.1), 0)])
@pytest.mark.parametrize("h16,w16", [(4, 4), (4, 6), (12, 20)])      # the level maps: 4x4, 2x2, 1x1 / 4x6, 2x3, 1x1 / 12x20, 6x10, 3x5
def test_select_flow(hip_lib, h16, w16, losses, level):
    g = torch.Generator().manual_seed(h16 * w16 + level)
    maps = [torch.randn((h16 >> k, w16 >> k, 8), generator=g) * 3 for k in range(3)]
    dl, dmaps = torch.tensor(losses).cuda(), [m.cuda() for m in maps]
    out = torch.full((h16, w16, 8), float("nan"), device="cuda")
    rec = torch.full((5,), float("nan"), device="cuda")
    _ck(hip_lib.vfi_atm_select_flow(ptr(dl), ptr(dmaps[0]), ptr(dmaps[1]), ptr(dmaps[2]), 8, h16, w16, ptr(out), 8, ptr(rec), _stream()), "vfi_atm_select_flow")
    torch.cuda.synchronize()
    got, rec = out.cpu(), rec.cpu()
    assert torch.equal(rec[:3], torch.tensor(losses)) and int(rec[3]) == level and torch.isnan(rec[4])
    assert torch.isnan(got[..., 4:]).all(), "channels 4..7 of the destination are not the kernel's"
    if level == 0:
        assert torch.equal(got[..., :4], maps[0][..., :4])
        return
    src = maps[level][..., :4]
    want = _up64(src, (h16, w16), 1 << level)[0].permute(1, 2, 0)
    hi, wi = src.shape[:2]
    # weights off by 4 u of the source coordinate each (<= hi + wi in all), four products and three sums, the factor: exact
    tol = (1 << level) * (4 * U * (hi + wi) + 8 * U) * float(src.abs().max()) + 0 * want
    _report(f"select {h16}x{w16} level {level}", (got[..., :4].double() - want).abs(), tol)


def test_select_flow_without_a_record_and_bad_arguments(hip_lib):
    z = torch.zeros(4 * 4 * 8, device="cuda")
    l = torch.tensor([0.3, 0.2, 0.1]).cuda()
    _ck(hip_lib.vfi_atm_select_flow(ptr(l), ptr(z), ptr(z), ptr(z), 8, 4, 4, ptr(z), 8, None, _stream()), "vfi_atm_select_flow")
    torch.cuda.synchronize()
    assert hip_lib.vfi_atm_select_flow(ptr(l), ptr(z), ptr(z), ptr(z), 8, 2, 4, ptr(z), 8, None, _stream()) != 0
    assert hip_lib.vfi_atm_select_flow(None, ptr(z), ptr(z), ptr(z), 8, 4, 4, ptr(z), 8, None, _stream()) != 0


# ---- 3. the existing kernels at the smallest global maps ---------------------------------------------------------------------------------

def _small_case(h, w, dtype=torch.float32):
    """(parameters of the first global ATM block of the seeded lite checkpoint, token map [2,h,w,352])"""
    prefix = "global_motion_atmformer.0."
    p = {k[len(prefix):]: v for k, v in E.state_dict_as("lite", dtype).items() if k.startswith(prefix)}
    g = torch.Generator().manual_seed(3000 + 10 * h + w)
    return p, (torch.randn((2, h, w, 352), generator=g, dtype=torch.float32) * 1.5).to(dtype)


@pytest.mark.parametrize("label_hw", [None, (4, 4)], ids=["own_labels", "labels_of_4x4"])
@pytest.mark.parametrize("shift", [0, 6])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 2), (2, 2)])
def test_window_attention_at_the_smallest_global_maps(hip_lib, h, w, shift, label_hw):
    p, x = _small_case(h, w)
    C_, win, ntok = 352, 12, 2 * h * w
    tok = torch.cat([x.reshape(-1, C_), torch.zeros(1, C_)])
    xn = F.layer_norm(tok, (C_,), p["norm1.weight"], p["norm1.bias"])
    q, kv = F.linear(xn, p["attn.q.weight"]), F.linear(xn, p["attn.kv.weight"])
    q, k, v = q.contiguous(), kv[:, :C_].contiguous(), kv[:, C_:].contiguous()
    lh, lw = label_hw or (h, w)
    with E.labels_of(label_hw):
        want, tol, woffs, offs_tol = lite._attention64(q, k, v, h, w, win, shift, True)
        with torch.no_grad():
            blk, mot = R.window_block(p, x, win, shift, True)           # the reference-derived restatement of the whole block
    dq, dk, dv = q.cuda(), k.cuda(), v.cuda()
    out = torch.full((ntok, C_), float("nan"), device="cuda")
    offs = torch.full((ntok, 8, 2), float("nan"), device="cuda")
    _ck(hip_lib.vfi_atm_window_attention_labels(ptr(dq), C_, ptr(dk), C_, ptr(dv), C_, ntok, ptr(out), C_, ptr(offs), h, w, lh, lw, C_, win, shift, 1,
                                                _stream()), "vfi_atm_window_attention_labels")
    torch.cuda.synchronize()
    got, goffs = out.cpu(), offs.cpu()
    assert torch.isfinite(got).all() and torch.isfinite(goffs).all()
    _report(f"attention {h}x{w} shift {shift}", (got.double() - want).abs(), tol)
    _report(f"offsets {h}x{w} shift {shift}", (goffs.double() - woffs).abs(), offs_tol)
    with torch.no_grad():
        y = xn[:ntok] + F.linear(got, p["attn.proj.weight"], p["attn.proj.bias"])
        mine = R.mlp_block(p, y.reshape(2, h, w, C_))
    d = float((mine - blk).abs().max())
    print(f"block {h}x{w} shift {shift} labels {lh}x{lw}: max |d| vs the restated block {d:.3e}")
    assert d <= E.TOL
    if label_hw is None:      # the plain entry point is the same launch
        out2 = torch.full((ntok, C_), float("nan"), device="cuda")
        _ck(hip_lib.vfi_atm_window_attention(ptr(dq), C_, ptr(dk), C_, ptr(dv), C_, ntok, ptr(out2), C_, None, h, w, C_, win, shift, 1, _stream()),
            "vfi_atm_window_attention")
        torch.cuda.synchronize()
        assert torch.equal(out2.cpu(), got)


def test_label_map_must_pad_to_the_same_layout(hip_lib):
    from cfi_amd import _lib

    t = torch.zeros(2 * 2 * 2 + 1, 352, device="cuda")
    rc = hip_lib.vfi_atm_window_attention_labels(ptr(t), 352, ptr(t), 352, ptr(t), 352, 8, ptr(t), 352, None, 2, 2, 14, 4, 352, 12, 6, 1, _stream())
    assert rc != 0 and "label map" in _lib.last_error()


@pytest.mark.parametrize("c,stride,dil,H,W", [(96, 2, 1, 2, 2), (64, 4, 1, 4, 4), (64, 4, 2, 4, 4), (96, 2, 1, 2, 4), (64, 4, 2, 4, 8), (96, 2, 1, 4, 4),
                                              (64, 4, 1, 8, 8)])
def test_tap_gather_and_fusion_convolutions_down_to_one_token(hip_lib, c, stride, dil, H, W):
    """the global fusion's three convolutions (gather + 1x1 layer) where their output is a 1x1, 1x2 or 2x2 map"""
    lite.test_strided_dilated_convolution(hip_lib, c, stride, dil, H, W)


# ---- 4. the forward --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def engines(hip_lib):
    """variant -> its AtmEngine, made at first use and kept for the module"""
    from cfi_amd import atm, ckpt

    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    made = {}

    def get(variant):
        if variant not in made:
            real = ckpt.load_config
            ckpt.load_config = E.config_with(True, True)      # (base is created under its own key)
            try:
                made[variant] = atm.AtmEngine(E.state_dict_as(variant, torch.float32), variant)
            finally:
                ckpt.load_config = real
        return made[variant]

    yield get
    for eng in made.values():
        eng.close()


def _device_frame(eng, f0, f1, gm):
    one = lambda f: f[0].permute(1, 2, 0).contiguous().cuda()      # noqa: E731
    out = eng.forward(one(f0), one(f1), gm)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("variant,case", [(v, c) for v in ("lite", "base") for c in E.NET_CASES[v]])
def test_forward_matches_the_reference_and_the_restatement(engines, variant, case, golden_dir):
    from cfi_amd import atm

    engine = engines(variant)
    golden = np.load(os.path.join(golden_dir, E.GOLDEN_PREFIX[engine.variant] + "_net.npz"))
    f0, f1 = E.frames_of(engine.variant, case)
    on_before = _device_frame(engine, f0, f1, True)
    out = _device_frame(engine, f0, f1, atm.ENSEMBLE)
    losses, level = engine.ensemble_record()
    again = _device_frame(engine, f0, f1, atm.ENSEMBLE)
    on_after = _device_frame(engine, f0, f1, True)
    d, sums_ok = cain_restated.compare(out, golden, case + "_", E.NET_STRIDE, E.TOL)
    dr = float((out - E.restated(engine.variant, case)[0]).abs().max())
    want = [float(x) for x in golden[case + "_losses"]]
    rel = max(abs(a - b) / b for a, b in zip(losses, want))
    print(f"ATM-{engine.variant} ensemble {case}: max |d| vs the reference's golden {d:.3e}, vs the float32 restatement at every pixel {dr:.3e}; "
          f"losses {losses} vs {want}: relative {rel:.3e}; level {level}")
    assert torch.equal(out, again), "the same pair twice, two results"
    assert torch.equal(on_before, on_after), "an ensemble call in between changed \"On\""
    assert level == int(golden[case + "_level"])
    assert rel <= E.LOSS_TOL
    assert d <= E.TOL and sums_ok and dr <= E.TOL
    if level == 0:
        assert torch.equal(out, on_before), "level 0 won: the ensemble is \"On\", bit for bit"
    else:
        assert float((out - on_before).abs().max()) > 1e-2


def test_record_needs_an_ensemble_forward(hip_lib):
    from cfi_amd import atm, atm_spec

    eng = atm.AtmEngine(atm_spec.seeded_state_dict(E.SEED))
    try:
        with pytest.raises(RuntimeError, match="no ensemble forward has run"):
            eng.ensemble_record()
        f0, f1 = E.frames_of("lite", "64x64")
        _device_frame(eng, f0, f1, True)
        with pytest.raises(RuntimeError, match="no ensemble forward has run"):
            eng.ensemble_record()
        before = eng.workspace_bytes()
        _device_frame(eng, f0, f1, atm.ENSEMBLE)
        assert eng.workspace_bytes() > before, "the ensemble's buffers are the workspace's"
        assert eng.ensemble_record()[1] in (0, 1, 2)
    finally:
        eng.close()


# ---- 5. the node, the refusals -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["odd", "rgba"])
@pytest.mark.parametrize("variant", ["lite", "base"])
def test_node_cases_match_the_reference_node(engines, variant, case, golden_dir, monkeypatch):
    engine = engines(variant)
    golden = np.load(os.path.join(golden_dir, E.GOLDEN_PREFIX[engine.variant] + "_node.npz"))
    R.check_node_case(case, E.run_node(engine.variant, case, monkeypatch, engine), golden)


@pytest.mark.parametrize("variant", ["lite", "base"])
def test_refusals_before_any_launch(engines, variant, hip_lib):
    from cfi_amd import _lib

    engine = engines(variant)
    z = torch.zeros(8, device="cuda")
    assert hip_lib.vfi_atm_forward_ensemble(None, ptr(z), ptr(z), 3, 64, 64, ptr(z), _stream()) != 0 and "vfi_atm_forward_ensemble" in _lib.last_error()
    before = engine.workspace_bytes()
    rc = engine.lib.vfi_atm_forward_ensemble(engine.handle, ptr(z), ptr(z), 3, 2176, 4096, ptr(z), _stream())
    msg = _lib.last_error()
    assert rc != 0 and "vfi_atm_forward_ensemble" in msg and "size limit of ATM-" + engine.variant in msg and engine.workspace_bytes() == before
    assert engine.lib.vfi_atm_forward_ensemble(engine.handle, ptr(z), None, 3, 64, 64, ptr(z), _stream()) != 0
    assert engine.lib.vfi_atm_forward(engine.handle, ptr(z), ptr(z), 3, 64, 64, 2, ptr(z), _stream()) != 0 and "vfi_atm_forward_ensemble's" in _lib.last_error()
