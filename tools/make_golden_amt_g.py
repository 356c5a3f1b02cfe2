"""Write the AMT-G goldens under tests/golden/ by running the REAL reference on this host (CPU), through oracle/ref_import:

  amt_g_net.npz    InputPadder(16) + the reference's own AMT_G forward (eval, scale_factor 1.0), un-padded, at amt_restated.NET_SHAPES
                   (128x128, 144x208, 130x200; the same frame seeds) and NET_TS (t = 0.5 and 0.2); the reference's state-dict key order
                   as a name list; and per shape, at t = 0.5, the conditions on the seeded checkpoint that make the 1e-3 gate able to see
                   a broken block: corr_effect_mean (mean |frame - frame with the lookup's output zeroed|, >= 1e-2), saturated_frac (share
                   of output values clamped at 0 or 1, <= 5 %) and, for each of the five update blocks, block_effect_<name> (mean |frame -
                   frame with that block's two outputs zeroed|, >= 5e-3).  The tool asserts them.
  amt_g_node.npz   the reference's own AMT_VFI node with amt-g.pth on amt_g_restated.NODE_CASES: 3 frames 128x128 at multiplier 2, 2 frames
                   130x200 at multiplier 3, and a skip list

Inputs are not stored: frames are cain_restated.seeded_frames(...).  Outputs are stored compactly (cain_restated.summary).  Weights:
cfi_amd.amt_spec.seeded_state_dict("G", SEED), nothing scaled.
Usage: python tools/make_golden_amt_g.py [net] [node]   (default: both; needs the reference checkout; nothing under oracle/ is changed)
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pkgload import load_package  # noqa: E402

load_package()
import amt_g_restated  # noqa: E402
import cain_restated  # noqa: E402
from cfi_amd.amt_spec import amt_shapes, seeded_state_dict  # noqa: E402
from oracle import ref_import  # noqa: E402

SEED = amt_g_restated.SEED
GOLDEN = os.path.join(ROOT, "tests", "golden")
NET_STRIDE, NET_SHAPES, NET_TS = amt_g_restated.NET_STRIDE, amt_g_restated.NET_SHAPES, amt_g_restated.NET_TS
CORR_EFFECT_MIN, SATURATED_MAX, BLOCK_EFFECT_MIN = 1e-2, 0.05, 5e-3


def make_node():
    cupy = sys.modules.get("cupy")      # einops (vfi_utils.preprocess_frames) probes every importable array library
    if cupy is not None and not hasattr(cupy, "ndarray"):
        cupy.ndarray = type("ndarray", (), {})
    import vfi_models.amt as node_mod
    import vfi_utils

    node = {}
    with tempfile.TemporaryDirectory() as d:
        torch.save({"state_dict": seeded_state_dict("G", SEED)}, os.path.join(d, "amt-g.pth"))
        node_mod.load_file_from_direct_url = lambda model_type, url: os.path.join(d, os.path.basename(url))
        for name, (ckpt, n, h, w, c, m, skip) in amt_g_restated.NODE_CASES.items():
            frames = cain_restated.seeded_frames(n, h, w, c, 9)
            states = vfi_utils.InterpolationStateList(skip, True) if skip else None
            with torch.no_grad():
                out = node_mod.AMT_VFI().vfi(ckpt, frames.clone(), 1, m, optional_interpolation_states=states)[0]
            assert torch.isfinite(out).all()
            node[f"{name}_shape"] = np.array(out.shape)
            for k, v in cain_restated.summary(out, amt_g_restated.NODE_STRIDE).items():
                node[f"{name}_{k}"] = v
            print(name, tuple(out.shape), float(out.min()), float(out.max()))
    np.savez_compressed(os.path.join(GOLDEN, "amt_g_node.npz"), seed=np.array(SEED), **node)


def make_net(arch):
    net = {}
    real_call = arch.BidirCorrBlock.__call__

    def zero_call(self, c0, c1):
        a, b = real_call(self, c0, c1)
        return torch.zeros_like(a), torch.zeros_like(b)

    model = arch.AMT_G()
    names = list(model.state_dict().keys())
    assert names == list(amt_shapes("G").keys())
    net["state_dict_keys"] = np.array(names)
    model.load_state_dict(seeded_state_dict("G", SEED))
    model.eval()
    for sname, (h, w, fseed) in NET_SHAPES.items():
        f = cain_restated.seeded_frames(2, h, w, 3, fseed).permute(0, 3, 1, 2).contiguous()
        padder = arch.InputPadder(f.shape, 16)
        f0, f1 = padder.pad(f[0:1]), padder.pad(f[1:2])

        def run(t):
            with torch.no_grad():
                return padder.unpad(model(f0, f1, embt=torch.FloatTensor([t]).view(1, 1, 1, 1), scale_factor=1.0, eval=True)["imgt_pred"])[0]

        for t in NET_TS:
            out = run(t)
            assert torch.isfinite(out).all()
            for k, v in cain_restated.summary(out.permute(1, 2, 0), NET_STRIDE).items():
                net[f"G_{sname}_t{t}_{k}"] = v
            print("G", sname, t, tuple(out.shape), float(out.min()), float(out.max()))
            if t != 0.5:
                continue
            arch.BidirCorrBlock.__call__ = zero_call
            try:
                blind = run(t)
            finally:
                arch.BidirCorrBlock.__call__ = real_call
            ce, sat = float((out - blind).abs().mean()), float(((out <= 0) | (out >= 1)).float().mean())
            net[f"G_{sname}_corr_effect_mean"], net[f"G_{sname}_saturated_frac"] = np.array(ce), np.array(sat)
            print("G", sname, "corr_effect_mean", ce, "saturated_frac", sat)
            assert ce >= CORR_EFFECT_MIN and sat <= SATURATED_MAX, (sname, ce, sat)
            for blk in amt_g_restated.UPDATE_BLOCKS:
                mod = getattr(model, blk)
                real = mod.forward
                mod.forward = lambda *a, _r=real, **k: tuple(torch.zeros_like(v) for v in _r(*a, **k))
                try:
                    eff = float((out - run(t)).abs().mean())
                finally:
                    del mod.forward
                net[f"G_{sname}_block_effect_{blk}"] = np.array(eff)
                print("G", sname, "block_effect", blk, eff)
                assert eff >= BLOCK_EFFECT_MIN, (sname, blk, eff)
    np.savez_compressed(os.path.join(GOLDEN, "amt_g_net.npz"), seed=np.array(SEED), **net)


def main():
    which = set(sys.argv[1:]) or {"net", "node"}
    ref_import.setup()
    import vfi_models.amt.amt_arch as arch

    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    if "node" in which:
        make_node()
    if "net" in which:
        make_net(arch)


if __name__ == "__main__":
    main()
