"""CPU: XVFI's checkpoint spec, the torch restatement (tests/xvfi_restated.py) against the reference's own outputs
(tests/golden/xvfi_net.npz, tools/make_golden_xvfi.py), and the node's surface and frame loop on a stand-in engine over the restatement
against the reference node's own outputs (tests/golden/xvfi_node.npz).  tests/test_gpu_xvfi.py runs the same cases on the device.

The forward gate is |d| <= 1e-3 per pixel on the un-clamped output, as for every node.  Each golden case also carries figures the tool
measured on the reference alone (xvfi_restated.NET_CONDITIONS): they are asserted here, so that a case whose splat targets sit next to an
integer, or whose warp masks next to 0.999, cannot pass for a fair gate."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cain_restated
import cfi_amd
import xvfi_restated as xr
from cfi_amd import _lib, xvfi, xvfi_spec
from cfi_amd.schedule import InterpolationStateList

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def net_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "xvfi_net.npz"))


@pytest.fixture(scope="module")
def node_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "xvfi_node.npz"))


# ---- spec ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale,count", [(2, 72), (4, 74)])
def test_shapes_are_the_reference_modules_state_dict(scale, count, net_golden):
    shapes = xvfi_spec.xvfi_shapes(scale)
    assert len(shapes) == count
    assert list(shapes) == [str(k) for k in net_golden[f"keys_scale{scale}"]]
    assert [",".join(map(str, s)) for s in shapes.values()] == [str(s) for s in net_golden[f"shapes_scale{scale}"]]
    al = xvfi_spec.aliases(scale)
    assert len(al) == 2 * (1 + {2: 1, 4: 2}[scale]) and all(k in shapes and v in shapes and shapes[k] == shapes[v] for k, v in al.items())
    if scale == 4:
        assert {"rec_ext_ds_module.1.weight", "rec_ext_ds_module.3.weight"} <= set(al)


def test_configs_and_padding():
    assert xvfi_spec.CKPT_CONFIGS == {"XVFInet_X4K1000FPS_exp1_latest.pt": {"module_scale_factor": 4, "S_trn": 3, "S_tst": 5},
                                      "XVFInet_Vimeo_exp1_latest.pt": {"module_scale_factor": 2, "S_trn": 1, "S_tst": 1}}
    assert xvfi_spec.divide_of(xr.V) == 16 and xvfi_spec.divide_of(xr.X) == 512
    assert xvfi_spec.padded_size(10, 18, xr.V) == (16, 32) and xvfi_spec.padded_size(20, 30, xr.X) == (512, 512)
    assert xvfi_spec.padded_size(1080, 1920, xr.X) == (1536, 2048) and xvfi_spec.padded_size(16, 16, xr.V) == (16, 16)
    with pytest.raises(KeyError):
        xvfi_spec.config_of("XVFInet.pt")


def test_state_dict_check_is_strict_and_refuses_an_alias_mismatch():
    sd = xvfi_spec.seeded_state_dict(xr.X, 1)
    xvfi_spec.check_state_dict(sd, 4)
    with pytest.raises(RuntimeError, match="Missing key"):
        xvfi_spec.check_state_dict(sd, 2)                      # X4K's 74 tensors are not Vimeo's 72
    for alias in ("rec_ext_ds_module.3.weight", "rec_ext_ds_module.0.0.bias"):
        bad = dict(sd)
        bad[alias] = sd[alias].clone()
        bad[alias].view(-1)[0] += 1.0
        with pytest.raises(RuntimeError, match=alias.replace(".", r"\.") + " differs from .* refused"):
            xvfi_spec.check_state_dict(bad, 4)
    bad = dict(sd)
    bad["vfinet.conv_flow1.weight"] = sd["vfinet.conv_flow1.weight"][:, :, :1]
    with pytest.raises(RuntimeError, match="size mismatch"):
        xvfi_spec.check_state_dict(bad, 4)


def test_flow_gain_scales_the_two_flow_heads_only():
    a, b = xvfi_spec.seeded_state_dict((2, 1), 3), xvfi_spec.seeded_state_dict((2, 1), 3, 30.0)
    heads = {h + s for h in xvfi_spec.FLOW_HEADS for s in (".weight", ".bias")}
    for k in a:
        assert torch.equal(b[k], a[k] * 30.0) if k in heads else torch.equal(b[k], a[k]), k
    w = a["vfinet.conv_flow1.weight"]
    assert float(w.abs().max()) <= 1 / (w.shape[1] * 9) ** 0.5      # default initialisation magnitudes


# ---- restatement against the reference ---------------------------------------------------------------------------------------------------------

def net_inputs(name, golden):
    scale, S, h, w, gain = xr.NET_CASES[name]
    sd = xvfi_spec.seeded_state_dict((scale, S), int(golden[f"{name}_seed"]), gain)
    f = cain_restated.seeded_frames(2, h, w, 3, xr.FRAME_SEED)
    return sd, f, scale, S


@pytest.mark.parametrize("name", sorted(xr.NET_CASES))
def test_golden_conditions_hold_on_the_reference(name, net_golden):
    gained = xr.NET_CASES[name][4] != 1.0
    for t in xr.NET_TS:
        for k in xr.condition_keys(gained, t):
            v = float(net_golden[f"{name}_t{t}_{k}"])
            print(f"{name} t={t} {k}: {v:.3e} (at least {xr.NET_CONDITIONS[k]})")
            assert v >= xr.NET_CONDITIONS[k], (name, t, k, v)


@pytest.mark.parametrize("name", sorted(xr.NET_CASES))
def test_forward_restatement_matches_the_reference(name, net_golden):
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    sd, f, scale, S = net_inputs(name, net_golden)
    x = f.permute(0, 3, 1, 2).contiguous()
    for t in xr.NET_TS:
        taps = {}
        with torch.no_grad():
            out = xr.xvfi_frame(sd, x[0:1], x[1:2], t, scale, S, taps)[0].permute(1, 2, 0)
        d, sums_ok = cain_restated.compare(out, net_golden, f"{name}_t{t}_", xr.NET_STRIDE, xr.TOL)
        fs = xr.FLOW_STRIDE.get(name, 1)
        dflow = float((taps["flow_l_tmp"][0].permute(1, 2, 0)[::fs, ::fs] - torch.from_numpy(net_golden[f"{name}_flow_l_tmp"])).abs().max())
        own = xr.conditions(taps, t)
        print(f"XVFI {name} t={t}: max |d| vs the reference {d:.3e}, flow_l_tmp {dflow:.3e}, own splat distance {own['splat_dist']:.2e}")
        assert d <= xr.TOL and sums_ok, (name, t, d, sums_ok)
        assert dflow <= 1e-5


# ---- node surface ------------------------------------------------------------------------------------------------------------------------------

def test_widgets_match_the_reference():
    cls = cfi_amd.XVFI
    it = cls.INPUT_TYPES()
    assert list(it["required"]) == ["ckpt_name", "frames", "batch_size", "multipler"]
    assert it["required"]["ckpt_name"] == (["XVFInet_X4K1000FPS_exp1_latest.pt", "XVFInet_Vimeo_exp1_latest.pt"],)
    assert it["required"]["frames"] == ("IMAGE",)
    assert it["required"]["batch_size"] == ("INT", {"default": 1, "min": 1, "max": 100})
    assert it["required"]["multipler"] == ("INT", {"default": 2, "min": 2, "max": 1000})
    assert it["optional"] == {"optional_interpolation_states": ("INTERPOLATION_STATES",)}
    assert cls.RETURN_TYPES == ("IMAGE",) and cls.FUNCTION == "vfi" and cls.CATEGORY == "ComfyUI-Frame-Interpolation/VFI"
    assert xvfi.MODEL_TYPE == "xvfi"
    assert list(inspect.signature(cls.vfi).parameters)[1:] == ["ckpt_name", "frames", "batch_size", "multipler", "optional_interpolation_states", "kwargs"]
    doc = xvfi.__doc__
    assert "numeric order" in doc and "is_frame_skipped" in doc          # the two stated deviations


def _mappings(extra_nodes):
    patch = "" if extra_nodes is None else (
        "import cfi_amd.ckpt as k; real = k.load_config; k.load_config = lambda: dict(real(), extra_nodes=%r); " % extra_nodes)
    code = ("import sys; sys.path.insert(0, %r); from pkgload import load_package; load_package(); import cfi_amd; " % ROOT + patch +
            "print(sorted(cfi_amd.NODE_CLASS_MAPPINGS)); print(sorted(cfi_amd.NODE_DISPLAY_NAME_MAPPINGS))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    classes, names = [eval(line) for line in r.stdout.strip().splitlines()[-2:]]
    return set(classes), set(names)


def test_opt_in_registry_in_a_fresh_process():
    classes, names = _mappings(None)
    assert classes == {"RIFE VFI", "FILM VFI", "M2M VFI", "IFRNet VFI", "GMFSS Fortuna VFI", "IFUnet VFI", "Make Interpolation State List"}
    assert "XVFI VFI" not in names
    classes, names = _mappings("xvfi")
    assert "XVFI VFI" in classes and "XVFI VFI" in names and "ATM VFI" not in classes and names <= classes
    assert cfi_amd.EXTRA_NODES["xvfi"] == ("XVFI VFI", "XVFI VFI (MI355X HIP)")
    with pytest.raises(AssertionError, match="unknown node"):
        _mappings("xvfi_vfi")
    assert not any("XVFI" in v for v in _lib.SUPPORTED_ENV)
    with open(os.path.join(ROOT, "comfyui-frame-interpolation_amd", "config.yaml")) as fh:
        assert '"xvfi" = XVFI VFI' in fh.read()


def test_refusals_come_before_an_engine_exists(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("the refusals must come before the checkpoint and the engine")

    monkeypatch.setattr(xvfi, "load_file_from_github_release", no_engine)
    monkeypatch.setattr(xvfi, "cached_engine", no_engine)
    with pytest.raises(KeyError):
        cfi_amd.XVFI().vfi("XVFInet.pt", torch.zeros(3, 16, 16, 3), 1, 2)
    with pytest.raises(ValueError, match="index arithmetic"):
        cfi_amd.XVFI().vfi(xr.X, torch.zeros(1, 1, 1, 3).expand(2, 2160, 3840, 3), 1, 2)      # 4K pads to 2560 x 4096
    with pytest.raises(IndexError):
        cfi_amd.XVFI().vfi(xr.V, torch.zeros(2, 16, 16, 3), 1, 2, [True, True])
    assert xvfi.MAX_PADDED_PIXELS == 6710886
    xvfi.check_frame_size(1080, 1920, xvfi_spec.config_of(xr.X))      # 1080p pads to 1536 x 2048 and fits


# ---- node loop -----------------------------------------------------------------------------------------------------------------------------------

_engines = {}


def engine_for(seed):
    def make(ckpt):
        key = (ckpt, seed)
        if key not in _engines:
            _engines[key] = xr.RestatedXvfi(ckpt, seed)
        return _engines[key]
    return make


@pytest.mark.parametrize("case", sorted(xr.NODE_CASES))
def test_node_loop_matches_the_reference_node(case, node_golden, monkeypatch):
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    assert float(node_golden[case + "_splat_dist"]) >= 1e-4 and float(node_golden[case + "_mask_dist"]) >= 1e-4
    out = xr.run_node(case, monkeypatch, engine_for(int(node_golden[case + "_seed"])))
    xr.check_node_case(case, out, node_golden)
    ckpt, n, h, w, c, m, states = xr.NODE_CASES[case]
    kept = [i for i in range(n - 1) if states is None or states[i]]
    assert out.shape[0] == n + len(kept) * (m - 1)
    if case == "bools":      # the pair the list switches off has its two frames next to each other
        src = cain_restated.seeded_frames(n, h, w, c, 9)[..., :3]
        assert torch.equal(out[2], src[1]) and torch.equal(out[3], src[2])


def test_five_frames_x3_are_in_the_reference_order(node_golden):
    """'vimeo_x3' is the issue's 5 frames x 3: below 10 frames and multipler 10 the reference's string sort IS the numeric order, so the node
    golden (compared above, frame by frame) pins the order; here: the source frames sit at every third position."""
    assert tuple(node_golden["vimeo_x3_shape"]) == (13, 16, 16, 3)
    keys = sorted([str(i) for i in range(5)] + [f"{i}.{k}" for i in range(4) for k in (1, 2)])
    assert xr.numeric_order(keys) == list(range(13))


@pytest.mark.parametrize("case", sorted(xr.ORDER_CASES))
def test_order_is_numeric_where_the_reference_scrambles(case, node_golden, monkeypatch):
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    keys = [str(k) for k in node_golden[case + "_keys"]]
    order = xr.numeric_order(keys)
    assert order != list(range(len(keys))), "the reference scrambles this clip: its string-sorted keys are not in numeric order"
    want = torch.from_numpy(node_golden[case + "_frames"])[order]
    out = xr.run_node(case, monkeypatch, engine_for(int(node_golden[case + "_seed"])))
    assert out.shape == want.shape
    d = float((out - want).abs().max())
    print(f"XVFI {case}: max |d| vs the reference's frames in numeric order {d:.3e}")
    assert d <= xr.TOL
    if case == "order_12x3":      # the issue's example: the reference puts input frame 10 at output position 6
        assert keys[6] == "10"


def test_interpolation_state_list_skips_the_named_pairs(monkeypatch, node_golden):
    ckpt, n, h, w, c, m, _ = xr.NODE_CASES["bools"]
    eng = engine_for(int(node_golden["bools_seed"]))
    a = xr.run_node((ckpt, n, h, w, c, m, ("skip", [1])), monkeypatch, eng)
    b = xr.run_node((ckpt, n, h, w, c, m, [True, False, True]), monkeypatch, eng)
    k = xr.run_node((ckpt, n, h, w, c, m, ("keep", [0, 2])), monkeypatch, eng)
    assert torch.equal(a, b) and torch.equal(k, b) and a.shape[0] == n + 2
    assert isinstance(xr.node_states(("skip", [1])), InterpolationStateList)


def test_results_do_not_depend_on_batch_size(monkeypatch, node_golden):
    eng = engine_for(int(node_golden["vimeo_x2_seed"]))
    assert torch.equal(xr.run_node("vimeo_x2", monkeypatch, eng, batch_size=1), xr.run_node("vimeo_x2", monkeypatch, eng, batch_size=3))
