"""Write the CAIN goldens under tests/golden/ by running the REAL reference on this host (CPU), through oracle/ref_import:

  cain_net.npz            CAIN(depth=3).forward(x1, x2)[0] at 64x96, 100x180 (both sides padded) and 256x448
  cain_node.npz           the reference CAIN_VFI node: multipliers 2, 3, 5, 7, a list multiplier, a skip list, RGBA input (48x72 frames)
  cain_schedule_kat.json  generic_frame_loop(use_timestep=False) with a probe model: output positions and model-call counts

Inputs are not stored: they are tests/cain_restated.seeded_frames(...) of the seeds below.  Outputs are stored compactly
(cain_restated.summary: a strided pixel sample plus float64 sums of every row and column).  Weights:
tests/cain_restated.seeded_state_dict(SEED), saved for the node in the real file format ({"state_dict": {"module.<key>"}}).
Usage: python tools/make_golden_cain.py   (needs the reference checkout; nothing under oracle/ is changed)
"""
import json
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
from oracle import ref_import  # noqa: E402

SEED = 1
GOLDEN = os.path.join(ROOT, "tests", "golden")
NET_SIZES = ((64, 96, 1), (100, 180, 2), (256, 448, 4))       # h, w, sample stride; frames seeded_frames(2, h, w, 3, 100 + i)
NODE_HW, NODE_STRIDE = (48, 72), 3
# name -> (frames, channels, multiplier, skip list); frames seeded_frames(n, 48, 72, c, 7)
NODE_CASES = {"m2": (3, 3, 2, None), "m3": (2, 3, 3, None), "m5": (2, 3, 5, None), "m7": (2, 3, 7, None), "list": (3, 3, [3, 0], None),
              "skip": (3, 3, 3, [1]), "rgba": (2, 4, 2, None)}
KAT_MULTIPLIERS = [2, 3, 4, 5, 7, 10, [3, 0, 4], [4, 2]]


def main():
    ref_import.setup()
    import vfi_models.cain as node_mod
    import vfi_models.cain.cain_arch as arch
    import vfi_utils

    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    sd = cain_restated.seeded_state_dict(SEED)
    model = arch.CAIN(depth=3)
    model.load_state_dict(sd)
    model.eval()
    net = {}
    for i, (h, w, stride) in enumerate(NET_SIZES):
        f = cain_restated.seeded_frames(2, h, w, 3, 100 + i)
        x1, x2 = f[0:1].permute(0, 3, 1, 2).contiguous(), f[1:2].permute(0, 3, 1, 2).contiguous()
        with torch.no_grad():
            out = model(x1.clone(), x2.clone())[0]
        for k, v in cain_restated.summary(out[0].permute(1, 2, 0), stride).items():
            net[f"{h}x{w}_{k}"] = v
    np.savez_compressed(os.path.join(GOLDEN, "cain_net.npz"), seed=np.array(SEED), **net)

    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "pretrained_cain.pth")
        torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}}, path)
        node_mod.load_file_from_github_release = lambda model_type, ckpt: path
        node = {}
        for name, (n, c, m, skip) in NODE_CASES.items():
            frames = cain_restated.seeded_frames(n, *NODE_HW, c, 7)
            states = vfi_utils.InterpolationStateList(skip, True) if skip else None
            with torch.no_grad():
                out = node_mod.CAIN_VFI().vfi("pretrained_cain.pth", frames.clone(), 10, m, optional_interpolation_states=states)[0]
            node[f"{name}_shape"] = np.array(out.shape)
            for k, v in cain_restated.summary(out, NODE_STRIDE).items():
                node[f"{name}_{k}"] = v
            print(name, tuple(out.shape), float(out.min()), float(out.max()))
    np.savez_compressed(os.path.join(GOLDEN, "cain_node.npz"), seed=np.array(SEED), **node)

    # schedule: frame i holds the value i; the probe model returns the mean of its two frames -> every output's value is its exact
    # (dyadic) position on the clip's time axis
    kat = []
    for m in KAT_MULTIPLIERS:
        for skip in (None, [1]):
            calls = []

            def probe(f0, f1, t, *a):
                calls.append(1)
                return (f0 + f1) / 2

            frames = torch.arange(4, dtype=torch.float32).view(4, 1, 1, 1).expand(4, 3, 1, 1).contiguous()
            states = vfi_utils.InterpolationStateList(skip, True) if skip else None
            out = vfi_utils.generic_frame_loop("CAIN_VFI", frames, 10, m, probe, interpolation_states=states, use_timestep=False,
                                               dtype=torch.float32)
            kat.append({"n_frames": 4, "multiplier": m, "skip": skip, "positions": [float(v) for v in out[:, 0, 0, 0]],
                        "model_calls": len(calls)})
    with open(os.path.join(GOLDEN, "cain_schedule_kat.json"), "w") as f:
        json.dump(kat, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
