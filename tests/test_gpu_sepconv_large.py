"""-m gpu: Sepconv VFI's banded head stage (csrc/sepconv_net.hip, csrc/sepconv_bands.h; docs/design/sepconv.md "4K") — bands forced at
small frames through the test option ``sepconv_band_rows`` against the whole-frame form bit for bit, and against the goldens and the fp32
restatement at the project's gate; the output stage on a band of rows (vfi_sepconv_pair_out_rows) within its float64 bound inside guarded
buffers; the banded form where the frame size demands it (1440x2560 and 2160x3840 behind config.yaml's ``sepconv_large_frames`` key, through
the node and the engine); and the object's limits.  The 4K parity against the restatement takes minutes on the host and lives in
tools/sepconv_bench.py --uhd --parity."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cain_restated
import ref_ops_restated as ror
import sepconv_restated
from gpu_util import describe_diff

pytestmark = pytest.mark.gpu
TOL = 1e-3      # the project's gate on the forward (tests/test_gpu_sepconv.py)
K = 51
NET_SIZES = ((64, 96, 1), (90, 160, 2), (101, 179, 2), (24, 40, 1))     # as tools/make_golden_sepconv.py
WHOLE, OLD, LARGE = 2097151, 4194303, 8388607


@pytest.fixture(scope="module")
def lib(hip_lib):
    from cfi_amd import _lib

    _lib.check(hip_lib.vfi_init(0), "vfi_init")
    return hip_lib


@pytest.fixture(scope="module")
def sd():
    from cfi_amd.sepconv_spec import seeded_state_dict

    return seeded_state_dict(1)


@pytest.fixture(scope="module")
def engine(lib, sd):
    from cfi_amd.sepconv import SepconvEngine

    e = SepconvEngine(sd)
    yield e
    e.close()


def config_with(**keys):
    from cfi_amd import ckpt

    real = ckpt.load_config

    def load():
        cfg = dict(real())
        cfg.update(keys)
        return cfg
    return load


class band_rows:
    """the test option for the length of a with block"""

    def __init__(self, lib, rows):
        self.lib, self.rows = lib, rows

    def __enter__(self):
        assert self.lib.vfi_test_set_option(b"sepconv_band_rows", self.rows) == 0

    def __exit__(self, *exc):
        self.lib.vfi_test_set_option(b"sepconv_band_rows", 0)


# ---- forced bands against the whole-frame form ---------------------------------------------------------------------------------------

_whole = {}


def _pair(h, w):
    f = cain_restated.seeded_frames(2, h, w, 3, 1000 + h + w).cuda()
    return f[0].contiguous(), f[1].contiguous()


def _whole_frame(engine, h, w):
    """the whole-frame form's output, computed once per size and never modified"""
    if (h, w) not in _whole:
        f0, f1 = _pair(h, w)
        _whole[(h, w)] = engine.forward([f0], [f1])[0].clone()
    return _whole[(h, w)]


BAND_CASES = [(h, w, bh) for h, w in ((64, 96), (101, 179), (90, 160), (25, 40), (24, 40)) for bh in (8, 16, 32)] + [(24, 40, 24)]
# ... at those sizes the 64 -> 51 layers have too few work items for the Winograd kernel (the 64 -> 256 layer takes it from 64x96 on); these
# two are the smallest even / odd frames where all five head layers are Winograd, the kernel every layer takes at the sizes bands serve
WINO_CASES = [(128, 192, 16), (131, 200, 32)]


def _last_conv_family(lib):
    """kernel family of the calling thread's last layer launch (include/vfi_hip_test.h): 2 direct, 3 Winograd"""
    import ctypes

    rec = (ctypes.c_int32 * 8)()
    assert lib.vfi_test_last_conv_launch(rec, 8) >= 1
    return rec[0]


@pytest.mark.parametrize("h,w,bh", BAND_CASES + WINO_CASES)
def test_forced_bands_equal_the_whole_frame_form(lib, engine, h, w, bh):
    """64x96: bands divide the height; 101x179: odd sides, a padded row and column, a short last band; 25x40: padded to 26 rows, a last band
    of 2; 24x40 with 24 / 32: a single band, and a band taller than the frame.  Bit for bit: a band's layer calls take the kernel the
    frame's call takes, on the frame's tile grid, with 4 / 2 real halo rows"""
    want = _whole_frame(engine, h, w)
    f0, f1 = _pair(h, w)
    with band_rows(lib, bh):
        got = engine.forward([f0], [f1])[0]
        again = engine.forward([f0], [f1])[0]
        family = _last_conv_family(lib)      # the last band's last 64 -> 51 layer
    assert torch.isfinite(got).all()
    if (h, w, bh) in WINO_CASES:
        assert family == 3, "this case is here for the Winograd form of the 64 -> 51 layers"
    print(f"{h}x{w} bands of {bh}: max |d| vs the whole-frame form {(got - want).abs().max().item():.3e}")
    assert torch.equal(got, want), describe_diff(got.cpu(), want.cpu(), f"{h}x{w} bands of {bh}")
    assert torch.equal(again, got)
    assert torch.equal(engine.forward([f0], [f1])[0], want), "the option left something behind"


def test_forced_bands_vs_reference_golden(lib, engine, sd, golden_dir, oracle_threads):
    gd = np.load(os.path.join(golden_dir, "sepconv_net.npz"))
    for i, (h, w, stride) in enumerate(NET_SIZES):
        f = cain_restated.seeded_frames(2, h, w, 3, 200 + i)
        fd = f.cuda()
        keep = fd.clone()
        with band_rows(lib, 16):
            got = engine.forward([fd[0]], [fd[1]])[0].cpu()
        assert torch.equal(fd, keep), "forward wrote its input frames"
        assert torch.isfinite(got).all()
        d, sums_ok = cain_restated.compare(got, gd, f"{h}x{w}_", stride, TOL)
        print(f"{h}x{w} bands of 16: sampled max |d| vs the golden {d:.3e}")
        assert d <= TOL and sums_ok, f"{h}x{w}: sampled max |d| {d}, row / column sums within tolerance: {sums_ok}"
        x = f.permute(0, 3, 1, 2).contiguous()
        want = sepconv_restated.sepconv_forward(sd, x[0:1], x[1:2])[0].permute(1, 2, 0)
        assert (got - want).abs().max().item() <= TOL, describe_diff(got, want, f"{h}x{w}")


def test_band_option_is_checked(lib, engine):
    from cfi_amd import _lib

    f0, f1 = _pair(24, 40)
    for bad in (12, 4):
        with band_rows(lib, bad):
            with pytest.raises(RuntimeError, match="no legal band height"):
                engine.forward([f0], [f1])
    assert "sepconv_band_rows" in _lib.last_error()


# ---- the output stage on a band of rows -------------------------------------------------------------------------------------------

PO_H, PO_W, PO_OFFS = 40, 70, (0, 52, 104, 156)


@pytest.fixture(scope="module")
def pair_out_case():
    """frames, heads and the float64 result of the whole 40x70 frame, shared by the band cases"""
    g = torch.Generator().manual_seed(PO_H * PO_W)
    f0, f1 = torch.rand(1, PO_H, PO_W, 3, generator=g), torch.rand(1, PO_H, PO_W, 3, generator=g)
    heads = torch.zeros(1, PO_H, PO_W, 208)
    for o in PO_OFFS:
        heads[..., o:o + K] = (torch.rand(1, PO_H, PO_W, K, generator=g) - 0.3) * (2.0 / K)
    f = lambda t: t.permute(0, 3, 1, 2).double().cuda()
    hd = heads.permute(0, 3, 1, 2).double().cuda()
    want, M = sepconv_restated.pair_out(f(f0), f(f1), *[hd[:, o:o + K] for o in PO_OFFS], PO_H, PO_W)
    return f0, f1, heads, want.permute(0, 2, 3, 1)[0].cpu(), M.permute(0, 2, 3, 1)[0].cpu()


def _guarded(x):
    """x -> a device copy between NaN guards of its own size (a stray read turns into NaN)"""
    buf = torch.full((3,) + tuple(x.shape), float("nan"), device="cuda")
    buf[1] = x.cuda()
    return buf[1]


@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("y0,y1", [(16, 32), (0, 16), (32, 40), (8, 16)])
def test_pair_out_rows_vs_float64(lib, pair_out_case, y0, y1, planar):
    """a band from the middle, the top and the bottom of a 40x70 frame (and one tile row): the heads exist for the band's rows only, between
    NaN guards, in the NHWC or the planar layout; the rows outside the band are not written"""
    from cfi_amd import _lib

    f0, f1, heads, want, M = pair_out_case
    band = heads[0, y0:y1]                                       # [rows, W, 208]
    Pb = (y1 - y0) * PO_W
    if planar:
        pl = torch.stack([band[..., o:o + K] for o in PO_OFFS]).permute(0, 3, 1, 2).reshape(4, K, Pb).contiguous()      # [4][51][Pb]
        hd = _guarded(pl)
        ptrs = [hd[k].data_ptr() for k in range(4)]
        pstr, fstr = 1, Pb
    else:
        hd = _guarded(band.contiguous())
        ptrs = [hd.data_ptr() + 4 * o for o in PO_OFFS]
        pstr, fstr = 208, 1
    a, b = _guarded(f0[0]), _guarded(f1[0])
    out = torch.full((PO_H * PO_W * 3 + 256,), float("nan"), device="cuda")
    _lib.check(lib.vfi_sepconv_pair_out_rows(a.data_ptr(), b.data_ptr(), 3, PO_H, PO_W, ptrs[0], ptrs[1], ptrs[2], ptrs[3], pstr, fstr, PO_W, y0, y1 - y0,
                                             out.data_ptr(), None), "vfi_sepconv_pair_out_rows")
    torch.cuda.synchronize()
    assert torch.isnan(out[PO_H * PO_W * 3:]).all(), "wrote past the output"
    got = out[:PO_H * PO_W * 3].view(PO_H, PO_W, 3).cpu().double()
    assert torch.isnan(got[:y0]).all() and torch.isnan(got[y1:]).all(), "a row outside the band was written"
    assert torch.isfinite(got[y0:y1]).all(), "NaN inside the band: a stray read or an unwritten pixel"
    tol = ror.tolerance(M, sepconv_restated.gamma_pair_out()) + 2 * ror.U * want.abs()
    bad = (got[y0:y1] - want[y0:y1]).abs() > tol[y0:y1]
    assert not bad.any(), describe_diff(got[y0:y1], want[y0:y1], f"rows {y0}..{y1}") + f", {int(bad.sum())} over the float64 bound"


def test_pair_out_rows_refuses_bad_bands(lib):
    from cfi_amd import _lib

    x = torch.zeros(64, device="cuda")
    p = x.data_ptr()
    for y0, rows in ((4, 8), (0, 0), (32, 9), (-8, 8)):
        assert lib.vfi_sepconv_pair_out_rows(p, p, 3, PO_H, PO_W, p, p, p, p, 208, 1, PO_W, y0, rows, p, None) != 0
        assert "vfi_sepconv_pair_out_rows" in _lib.last_error()


# ---- the banded form where the frame size demands it ---------------------------------------------------------------------------------

def _node(monkeypatch, tmp_path, sd):
    from cfi_amd import ckpt, sepconv

    path = tmp_path / "ckpts" / "sepconv" / "sepconv.pth"
    path.parent.mkdir(parents=True)
    torch.save(sd, path)      # the real file format (a plain state dict), seeded weights
    monkeypatch.setattr(sepconv, "load_file_from_github_release", lambda model_type, name: str(path))
    ckpt.clear_engine_cache()
    return sepconv.SepconvVFI()


def _smooth_pair(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand(2, 3, h // 8 + 2, w // 8 + 2, generator=g)
    return F.interpolate(lo, size=(h, w), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("h,w", [(1440, 2560), (2160, 3840)])
def test_node_serves_large_frames_behind_the_key(monkeypatch, tmp_path, lib, sd, h, w):
    from cfi_amd import ckpt

    node = _node(monkeypatch, tmp_path, sd)
    monkeypatch.setattr(ckpt, "load_config", config_with(sepconv_large_frames=True))
    frames = _smooth_pair(h, w, h + w)
    try:
        out = node.vfi("sepconv.pth", frames, 10, 2)[0]
        assert tuple(out.shape) == (3, h, w, 3) and torch.isfinite(out).all()
        assert torch.equal(out[0], frames[0]) and torch.equal(out[2], frames[1])
        again = node.vfi("sepconv.pth", frames, 10, 2)[0]
        assert torch.equal(again, out), "the same pair twice: different bits"
    finally:
        ckpt.clear_engine_cache()


def test_engine_workspace_and_forms(monkeypatch, lib, sd):
    """the key decides the form above 2 097 151 pixels only; the 4K workspace is below four 1080p workspaces"""
    from cfi_amd import ckpt
    from cfi_amd.sepconv import SepconvEngine

    e = SepconvEngine(sd)
    try:
        def run(h, w):
            f = torch.rand(2, h, w, 3, device="cuda")
            out = e.forward([f[0]], [f[1]])
            assert torch.isfinite(out).all()
            return out.clone(), e.workspace_bytes()

        monkeypatch.setattr(ckpt, "load_config", config_with(sepconv_large_frames=True))
        torch.manual_seed(3)
        on_1080, ws_1080_on = run(1080, 1920)
        _, ws_1440_on = run(1440, 2560)
        _, ws_4k = run(2160, 3840)
        assert e.max_padded_pixels() == LARGE
        monkeypatch.setattr(ckpt, "load_config", config_with(sepconv_large_frames=False))
        torch.manual_seed(3)
        off_1080, ws_1080 = run(1080, 1920)
        _, ws_1440 = run(1440, 2560)      # the whole-frame form on the layers' large-image forms, as ever
        assert e.max_padded_pixels() == OLD
        print(f"workspace bytes: 1080p {ws_1080}, 1440x2560 whole-frame {ws_1440} / banded {ws_1440_on}, 2160x3840 banded {ws_4k}")
        assert torch.equal(on_1080, off_1080) and ws_1080_on == ws_1080, "at 1080p the key changes nothing"
        assert ws_1440_on < ws_1440, "with the key on a 1440x2560 frame takes the bands"
        assert 0 < ws_4k < 4 * ws_1080
    finally:
        e.close()


def test_key_off_refuses_4k_before_anything_is_allocated(monkeypatch, tmp_path, lib, sd):
    from cfi_amd import ckpt, sepconv
    from cfi_amd.sepconv import SepconvEngine

    node = _node(monkeypatch, tmp_path, sd)
    monkeypatch.setattr(sepconv, "load_file_from_github_release", lambda *a: (_ for _ in ()).throw(AssertionError("the checkpoint was asked for")))
    frames = torch.zeros(1, 1, 1, 3).expand(2, 2160, 3840, 3)      # the check reads the shape only
    with pytest.raises(ValueError, match=r"Sepconv VFI: 2160x3840 frames \(padded 2160x3840\) are over the size limit of 4194303 padded pixels; "
                                         r"config.yaml's sepconv_large_frames: true raises it to 8388607"):
        node.vfi("sepconv.pth", frames, 10, 2)
    e = SepconvEngine(sd)
    try:
        f = torch.zeros(2160, 3840, 3, device="cuda")
        with pytest.raises(RuntimeError, match="over the size limit of 4194303 padded pixels"):
            e.forward([f], [f])
        assert e.workspace_bytes() == 0
    finally:
        e.close()


# ---- the object's limits -------------------------------------------------------------------------------------------------------------

def test_object_limit(monkeypatch, lib, sd):
    from cfi_amd import _lib, ckpt, sepconv
    from cfi_amd.sepconv import SepconvEngine

    assert lib.vfi_sepconvnet_max_pixels() == sepconv.MAX_PADDED_PIXELS == OLD
    assert lib.vfi_sepconvnet_large_max_pixels() == sepconv.LARGE_MAX_PADDED_PIXELS == LARGE
    assert sepconv.WHOLE_FRAME_PIXELS == WHOLE and sepconv.BAND_MAX_WIDTH == 131071
    assert lib.vfi_sepconvnet_object_max_pixels(None) == 0
    assert lib.vfi_sepconvnet_set_large_frames(None, 1) != 0 and "vfi_sepconvnet_set_large_frames: null object" in _lib.last_error()
    e = SepconvEngine(sd)
    try:
        assert lib.vfi_sepconvnet_object_max_pixels(e.handle) == OLD
        assert lib.vfi_sepconvnet_set_large_frames(e.handle, 1) == 0 and lib.vfi_sepconvnet_object_max_pixels(e.handle) == LARGE
        assert lib.vfi_sepconvnet_set_large_frames(e.handle, 0) == 0 and lib.vfi_sepconvnet_object_max_pixels(e.handle) == OLD
        monkeypatch.setattr(ckpt, "load_config", config_with(sepconv_large_frames=True))
        assert e.max_padded_pixels() == LARGE
        over = torch.zeros(2898, 2896, 3, device="cuda")            # 8 392 608 pixels
        with pytest.raises(RuntimeError, match=r"over the size limit with large frames on, 8388607 padded pixels.*\[Hp, Wp, 64\] must stay below 2 GiB"):
            e.forward([over], [over])
        assert e.workspace_bytes() == 0
        del over
        wide = torch.zeros(16, 131074, 3, device="cuda")            # 2 097 184 pixels: banded, and no band of 8 rows with its halo fits
        with pytest.raises(RuntimeError, match="too wide for the banded head stage"):
            e.forward([wide], [wide])
        assert e.workspace_bytes() == 0
    finally:
        e.close()
