"""Write the SepConv++ goldens under tests/golden/ by running the REAL reference on this host (CPU), through oracle/ref_import, with the
reference's own sepconv kernel text (ref_import.reference_ops(): the cupy backend's sepconv_out compiled for the host):

  sepconv_net.npz    Network().forward(x1, x2) at 64x96 (every level even), 90x160 (odd rows 45 and 23, two decoder crops),
                     101x179 (the even pad and crops in both dimensions) and 24x40 (a frame smaller than the 51-tap filter)
  sepconv_node.npz   the reference SepconvVFI node: multipliers 2, 3, 5, a list multiplier, a skip list, RGBA input (48x72 frames)

Inputs are not stored: they are cain_restated.seeded_frames(...) of the seeds below.  Outputs are stored compactly
(cain_restated.summary: a strided pixel sample plus float64 sums of every row and column).  Weights:
cfi_amd.sepconv_spec.seeded_state_dict(SEED), saved for the node as a plain state dict (the real file's format).
Usage: python tools/make_golden_sepconv.py   (needs the reference checkout; nothing under oracle/ is changed)
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
import cain_restated  # noqa: E402
from cfi_amd.sepconv_spec import seeded_state_dict  # noqa: E402
from oracle import ref_import  # noqa: E402

SEED = 1
GOLDEN = os.path.join(ROOT, "tests", "golden")
NET_SIZES = ((64, 96, 1), (90, 160, 2), (101, 179, 2), (24, 40, 1))     # h, w, sample stride; frames seeded_frames(2, h, w, 3, 200 + i)
NODE_HW, NODE_STRIDE = (48, 72), 3
# name -> (frames, channels, multiplier, skip list); frames seeded_frames(n, 48, 72, c, 9)
NODE_CASES = {"m2": (3, 3, 2, None), "m3": (2, 3, 3, None), "m5": (2, 3, 5, None), "list": (3, 3, [3, 0], None),
              "skip": (3, 3, 3, [1]), "rgba": (2, 4, 2, None)}


def main():
    ref_import.reference_ops()
    # einops (vfi_utils.preprocess_frames) probes every importable array library; the host stand-in for cupy has no array type
    cupy = sys.modules.get("cupy")
    if cupy is not None and not hasattr(cupy, "ndarray"):
        cupy.ndarray = type("ndarray", (), {})
    import vfi_models.sepconv as node_mod
    import vfi_models.sepconv.sepconv_enhanced as arch
    import vfi_utils

    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    sd = seeded_state_dict(SEED)
    net = {}
    for i, (h, w, stride) in enumerate(NET_SIZES):
        model = arch.Network()      # objScratch keeps the last call's level shapes: a fresh network per size, as the node makes one per call
        model.load_state_dict(sd)
        model.eval()
        f = cain_restated.seeded_frames(2, h, w, 3, 200 + i)
        x1, x2 = f[0:1].permute(0, 3, 1, 2).contiguous(), f[1:2].permute(0, 3, 1, 2).contiguous()
        with torch.no_grad():
            out = model(x1.clone(), x2.clone())[0]
        for k, v in cain_restated.summary(out.permute(1, 2, 0), stride).items():
            net[f"{h}x{w}_{k}"] = v
        print(h, w, float(out.min()), float(out.max()))
    np.savez_compressed(os.path.join(GOLDEN, "sepconv_net.npz"), seed=np.array(SEED), **net)

    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "sepconv.pth")
        torch.save(sd, path)
        node_mod.load_file_from_github_release = lambda model_type, ckpt: path
        # preprocess_frames' rearrange yields channels-last strides, which F.pad and torch.stack keep, and Network.forward's
        # tenStack.view(...) (sepconv_enhanced.py:626) refuses them on current torch: hand the node contiguous frames (same values)
        prep = node_mod.preprocess_frames
        node_mod.preprocess_frames = lambda f: prep(f).contiguous()
        node = {}
        for name, (n, c, m, skip) in NODE_CASES.items():
            frames = cain_restated.seeded_frames(n, *NODE_HW, c, 9)
            states = vfi_utils.InterpolationStateList(skip, True) if skip else None
            with torch.no_grad():
                out = node_mod.SepconvVFI().vfi("sepconv.pth", frames.clone(), 10, m, optional_interpolation_states=states)[0]
            node[f"{name}_shape"] = np.array(out.shape)
            for k, v in cain_restated.summary(out, NODE_STRIDE).items():
                node[f"{name}_{k}"] = v
            print(name, tuple(out.shape), float(out.min()), float(out.max()))
    np.savez_compressed(os.path.join(GOLDEN, "sepconv_node.npz"), seed=np.array(SEED), **node)


if __name__ == "__main__":
    main()
