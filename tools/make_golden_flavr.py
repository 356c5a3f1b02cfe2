"""Write the FLAVR goldens under tests/golden/ by running the REAL reference on this host (CPU), through oracle/ref_import:

  flavr_net.npz    InputPadder(16) + UNet_3D_3D("unet_18", n_inputs=4, n_outputs, "concat", "transpose")(four frames)[0], un-padded:
                   n_outputs = 1 at 64x96 (every level even), 50x70 and 101x179 (asymmetric padding in both dimensions);
                   n_outputs = 3 at 64x96 (encoder biases, output 0 of three)
  flavr_node.npz   the reference FLAVR_VFI node on 48x72 frames: 4 and 6 frames, duplicate_first_last_frames, skip lists [0, 1] (the
                   first window dropped), [2] (nothing dropped) and [2, 3] (the last window dropped), RGBA input, multiplier 3 (a
                   warning, same frames), a 50x70 clip, and the 4x checkpoint

Inputs are not stored: they are cain_restated.seeded_frames(...) of the seeds below.  Outputs are stored compactly
(cain_restated.summary: a strided pixel sample plus float64 sums of every row and column).  Weights:
cfi_amd.flavr_spec.seeded_state_dict(SEED, n_outputs), saved for the node in the real files' format ({"state_dict": ...} with the
"module." prefix).  Usage: python tools/make_golden_flavr.py   (needs the reference checkout; nothing under oracle/ is changed)
"""
import os
import sys
import tempfile
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pkgload import load_package  # noqa: E402

load_package()
import cain_restated  # noqa: E402
from cfi_amd.flavr_spec import seeded_state_dict  # noqa: E402
from oracle import ref_import  # noqa: E402

SEED = 1
GOLDEN = os.path.join(ROOT, "tests", "golden")
# name -> (n_outputs, h, w, sample stride, frame seed); frames seeded_frames(4, h, w, 3, seed)
NET_CASES = {"o1_64x96": (1, 64, 96, 1, 300), "o1_50x70": (1, 50, 70, 1, 301), "o1_101x179": (1, 101, 179, 2, 302),
             "o3_64x96": (3, 64, 96, 1, 303)}
NODE_STRIDE = 3
# name -> (frames, h, w, channels, multiplier, duplicate_first_last_frames, skip list, n_outputs); frames seeded_frames(n, h, w, c, 9)
NODE_CASES = {"n4": (4, 48, 72, 3, 2, False, None, 1), "n6": (6, 48, 72, 3, 2, False, None, 1), "dup": (5, 48, 72, 3, 2, True, None, 1),
              "skip01": (6, 48, 72, 3, 2, False, [0, 1], 1), "skip2": (6, 48, 72, 3, 2, False, [2], 1),
              "skiplast": (6, 48, 72, 3, 2, False, [2, 3], 1), "rgba": (4, 48, 72, 4, 2, False, None, 1),
              "m3": (4, 48, 72, 3, 3, False, None, 1), "odd": (5, 50, 70, 3, 2, False, None, 1), "x4": (4, 48, 72, 3, 2, False, None, 3)}


def main():
    ref_import.setup()
    import vfi_models.flavr as node_mod
    import vfi_models.flavr.flavr_arch as arch
    import vfi_models.flavr.resnet_3D as resnet_3D
    import vfi_utils

    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))

    def model_of(n_outputs):
        resnet_3D.useBias = False      # UNet_3D_3D sets it for n_outputs > 1 and never resets it
        m = arch.UNet_3D_3D("unet_18", n_inputs=4, n_outputs=n_outputs, joinType="concat", upmode="transpose")
        m.load_state_dict(seeded_state_dict(SEED, n_outputs))
        return m.eval()

    net = {}
    for name, (no, h, w, stride, fseed) in NET_CASES.items():
        model = model_of(no)
        f = cain_restated.seeded_frames(4, h, w, 3, fseed).permute(0, 3, 1, 2).contiguous()
        padder = arch.InputPadder(f.shape, 16)
        with torch.no_grad():
            out = padder.unpad(model([padder.pad(f[i:i + 1]) for i in range(4)])[0])[0]
        for k, v in cain_restated.summary(out.permute(1, 2, 0), stride).items():
            net[f"{name}_{k}"] = v
        print(name, tuple(out.shape), float(out.min()), float(out.max()))
    np.savez_compressed(os.path.join(GOLDEN, "flavr_net.npz"), seed=np.array(SEED), **net)

    node = {}
    with tempfile.TemporaryDirectory() as d:
        paths = {}
        for no, ckpt in ((1, "FLAVR_2x.pth"), (3, "FLAVR_4x.pth")):
            paths[ckpt] = os.path.join(d, ckpt)
            torch.save({"state_dict": {"module." + k: v for k, v in seeded_state_dict(SEED, no).items()}}, paths[ckpt])
        node_mod.load_file_from_github_release = lambda model_type, ckpt: paths[ckpt]
        for name, (n, h, w, c, m, dup, skip, no) in NODE_CASES.items():
            frames = cain_restated.seeded_frames(n, h, w, c, 9)
            states = vfi_utils.InterpolationStateList(skip, True) if skip else None
            resnet_3D.useBias = False
            with torch.no_grad(), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                out = node_mod.FLAVR_VFI().vfi("FLAVR_2x.pth" if no == 1 else "FLAVR_4x.pth", frames.clone(), 10, m, dup, states)[0]
            node[f"{name}_shape"] = np.array(out.shape)
            for k, v in cain_restated.summary(out, NODE_STRIDE).items():
                node[f"{name}_{k}"] = v
            print(name, tuple(out.shape), float(out.min()), float(out.max()))
    np.savez_compressed(os.path.join(GOLDEN, "flavr_node.npz"), seed=np.array(SEED), **node)


if __name__ == "__main__":
    main()
