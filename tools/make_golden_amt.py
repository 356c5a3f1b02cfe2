"""Write the AMT goldens under tests/golden/ by running the REAL reference on this host (CPU), through oracle/ref_import:

  amt_lookup.npz   the reference's own BidirCorrBlock(fmap0, fmap1, num_levels=4, radius=3)(c0, c1) — the materialised all-pairs
                   volume, pooled and sampled — on the cases of amt_restated.LOOKUP_CASES (inputs from amt_restated.lookup_case);
                   both directions, every second query row / column plus the last
  amt_net.npz      InputPadder(16) + the reference's own AMT_S / AMT_L forward (eval, scale_factor 1.0), un-padded, at 128x128 (the
                   minimum: a 2x2 coarsest level), 144x208 (odd pooled sizes) and 130x200 (centred replicate pad 7/7, 4/4), t = 0.5 and
                   0.2; and per variant and shape, at t = 0.5, with the lookup's output zeroed: corr_effect_mean = mean |frame - frame
                   without lookup| and saturated_frac = share of output values clamped at 0 or 1

  amt_node.npz     the reference's own AMT_VFI node (vfi_models/amt/__init__.py) on NODE_CASES: multipliers 2 and 3, a list multiplier, a
                   skip list, RGBA input, a 130x200 clip (padded 144x208 by the node), AMT-S and one AMT-L case

Inputs are not stored: frames are cain_restated.seeded_frames(2, h, w, 3, seed).  Outputs are stored compactly (cain_restated.summary: a
strided pixel sample plus float64 sums of every row and column).  Weights: cfi_amd.amt_spec.seeded_state_dict(variant, SEED).
Usage: python tools/make_golden_amt.py [lookup] [net] [node]   (default: all three; needs the reference checkout; nothing under oracle/ is changed)
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
import amt_restated  # noqa: E402
import cain_restated  # noqa: E402
from cfi_amd.amt_spec import CONFIG, amt_shapes, seeded_state_dict  # noqa: E402
from oracle import ref_import  # noqa: E402

SEED = amt_restated.SEED
GOLDEN = os.path.join(ROOT, "tests", "golden")
# the cases live beside the restatement, so that the tool and the tests cannot drift apart
NET_STRIDE, NET_SHAPES, NET_TS = amt_restated.NET_STRIDE, amt_restated.NET_SHAPES, amt_restated.NET_TS
NODE_STRIDE, NODE_CASES = amt_restated.NODE_STRIDE, amt_restated.NODE_CASES


def make_node():
    """the reference's own AMT_VFI on seeded checkpoints in the real files' {"state_dict": ...} form"""
    cupy = sys.modules.get("cupy")      # einops (vfi_utils.preprocess_frames) probes every importable array library
    if cupy is not None and not hasattr(cupy, "ndarray"):
        cupy.ndarray = type("ndarray", (), {})
    import vfi_models.amt as node_mod
    import vfi_utils
    from cfi_amd.amt_spec import CKPT_VARIANT

    node = {}
    with tempfile.TemporaryDirectory() as d:
        for ckpt, variant in CKPT_VARIANT.items():
            if variant:
                torch.save({"state_dict": seeded_state_dict(variant, SEED)}, os.path.join(d, ckpt))
        node_mod.load_file_from_direct_url = lambda model_type, url: os.path.join(d, os.path.basename(url))
        for name, (ckpt, n, h, w, c, m, skip) in NODE_CASES.items():
            frames = cain_restated.seeded_frames(n, h, w, c, 9)
            states = vfi_utils.InterpolationStateList(skip, True) if skip else None
            with torch.no_grad():
                out = node_mod.AMT_VFI().vfi(ckpt, frames.clone(), 1, m, optional_interpolation_states=states)[0]
            assert torch.isfinite(out).all()
            node[f"{name}_shape"] = np.array(out.shape)
            for k, v in cain_restated.summary(out, NODE_STRIDE).items():
                node[f"{name}_{k}"] = v
            print(name, tuple(out.shape), float(out.min()), float(out.max()))
    np.savez_compressed(os.path.join(GOLDEN, "amt_node.npz"), seed=np.array(SEED), **node)


def main():
    which = set(sys.argv[1:]) or {"lookup", "net", "node"}
    ref_import.setup()
    import vfi_models.amt.amt_arch as arch

    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    if "node" in which:
        make_node()
    if "lookup" in which:
        make_lookup(arch)
    if "net" in which:
        make_net(arch)


def make_lookup(arch):
    look = {}
    for name in amt_restated.LOOKUP_CASES:
        f0, f1, c0, c1 = amt_restated.lookup_case(name)
        with torch.no_grad():
            o0, o1 = arch.BidirCorrBlock(f0[None], f1[None], num_levels=4, radius=3)(c0[None], c1[None])
        iy = cain_restated.sample_index(f0.shape[1], amt_restated.LOOKUP_STRIDE)
        ix = cain_restated.sample_index(f0.shape[2], amt_restated.LOOKUP_STRIDE)
        for k, o in (("out0", o0), ("out1", o1)):
            look[f"{name}_{k}"] = o[0][:, iy][:, :, ix].numpy()
        print(name, tuple(o0.shape), float(o0.abs().max()))
    np.savez_compressed(os.path.join(GOLDEN, "amt_lookup.npz"), **look)


def make_net(arch):
    net = {}
    real_call = arch.BidirCorrBlock.__call__

    def zero_call(self, c0, c1):
        a, b = real_call(self, c0, c1)
        return torch.zeros_like(a), torch.zeros_like(b)

    for variant, cls in (("S", arch.AMT_S), ("L", arch.AMT_L)):
        model = cls(corr_radius=3, corr_lvls=4, num_flows=CONFIG[variant]["num_flows"])
        sd = seeded_state_dict(variant, SEED)
        assert list(model.state_dict().keys()) == list(amt_shapes(variant).keys())
        model.load_state_dict(sd)
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
                    net[f"{variant}_{sname}_t{t}_{k}"] = v
                if t == 0.5:
                    arch.BidirCorrBlock.__call__ = zero_call
                    try:
                        blind = run(t)
                    finally:
                        arch.BidirCorrBlock.__call__ = real_call
                    net[f"{variant}_{sname}_corr_effect_mean"] = np.array(float((out - blind).abs().mean()))
                    net[f"{variant}_{sname}_saturated_frac"] = np.array(float(((out <= 0) | (out >= 1)).float().mean()))
                    print(variant, sname, "corr_effect_mean", float(net[f"{variant}_{sname}_corr_effect_mean"]), "saturated_frac",
                          float(net[f"{variant}_{sname}_saturated_frac"]))
                print(variant, sname, t, tuple(out.shape), float(out.min()), float(out.max()))
    np.savez_compressed(os.path.join(GOLDEN, "amt_net.npz"), seed=np.array(SEED), **net)


if __name__ == "__main__":
    main()
