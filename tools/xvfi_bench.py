"""Device-resident XVFI at 1080p, seeded weights, both configurations (Vimeo: scale 2, S_tst 1; X4K: scale 4, S_tst 5).

    python tools/xvfi_bench.py [--iters 5] [--height 1080] [--width 1920] [--trace] [--large-frames]

Prints one JSON line: per configuration the ms per interpolated frame at x2 (one timestep per pair: features + level flows + one render)
and at x8 (seven timesteps per pair: the pair-level work once), medians of `iters` pairs timed with device events around the calls with the
frames already on the device; the workspace size; and with --trace the library's per-kernel event trace (vfi_trace_*) of one extra x2 pair:
the share of the layer objects (rows conv*), of the space-to-depth pass in front of the 4x4 stride-2 layers, and of the new kernels (xvfi_*).

The tool checks three things only and fails otherwise: the output is finite, the same pair and timestep twice give the same bits, and the
workspace figure is positive and returns to zero after a release.  Whole-network parity at this size is deliberately not a gate
(docs/design/xvfi.md): tens of splat targets sit within 1e-4 of an integer in the reference itself.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--trace", action="store_true", help="per-kernel event trace of one extra x2 pair")
    ap.add_argument("--large-frames", action="store_true", help="run as with config.yaml's xvfi_large_frames on (sizes over 6 710 886 padded pixels)")
    args = ap.parse_args()
    from pkgload import load_package

    load_package()
    import cain_restated
    from cfi_amd import _lib, ckpt, xvfi, xvfi_spec

    if args.large_frames:
        real_config = ckpt.load_config
        ckpt.load_config = lambda: dict(real_config(), xvfi_large_frames=True)
    H, W = args.height, args.width
    frames = cain_restated.seeded_frames(3, H, W, 3, 5).cuda()
    result = {"tool": "xvfi_bench", "height": H, "width": W, "iters": args.iters}
    for name, ckpt in (("vimeo", "XVFInet_Vimeo_exp1_latest.pt"), ("x4k", "XVFInet_X4K1000FPS_exp1_latest.pt")):
        eng = xvfi.XvfiEngine(xvfi_spec.seeded_state_dict(ckpt, 7), ckpt)
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        pairs = [(frames[0], frames[1]), (frames[1], frames[2])]      # alternate, so that every timed pair recomputes its features
        eng.forward(*pairs[0], 0.5, out)                               # warm-up: workspace, first-launch costs
        eng.forward(*pairs[1], 0.5, out)
        row = {"padded": list(xvfi_spec.padded_size(H, W, ckpt))}
        for mult in (2, 8):
            ts = [k / mult for k in range(1, mult)]
            ms = [timed(lambda p=pairs[i % 2]: [eng.forward(p[0], p[1], t, out) for t in ts]) for i in range(args.iters)]
            row[f"x{mult}_ms_per_frame"] = round(statistics.median(ms) / len(ts), 3)
        a = eng.forward(*pairs[0], 0.5).clone()
        b = eng.forward(*pairs[0], 0.5)
        assert torch.isfinite(a).all(), "non-finite output"
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the same pair and timestep twice differ"
        row["workspace_bytes"] = eng.workspace_bytes()
        assert row["workspace_bytes"] > 0
        if args.trace:
            lib = _lib.load()
            lib.vfi_trace_reset()
            lib.vfi_trace_enable(1)
            eng.forward(*pairs[1], 0.5, out)
            torch.cuda.synchronize()
            lib.vfi_trace_enable(0)
            import ctypes

            buf = ctypes.create_string_buffer(1 << 16)
            lib.vfi_trace_report(buf, len(buf))
            rows = [ln.split() for ln in buf.value.decode().splitlines() if ln.strip()]
            total = sum(float(r[2]) for r in rows) or 1.0
            share = lambda pred: round(sum(float(r[2]) for r in rows if pred(r[0])) / total, 4)      # noqa: E731
            row["kernel_ms"] = round(total, 3)
            row["share_layers"] = share(lambda n: n.startswith(("conv", "deconv")) and n != "conv4x4s2_s2d")
            row["share_s2d"] = share(lambda n: n == "conv4x4s2_s2d")
            row["share_xvfi_kernels"] = {r[0]: round(float(r[2]) / total, 4) for r in rows if r[0].startswith("xvfi_")}
            row["share_other"] = share(lambda n: not n.startswith(("conv", "deconv", "xvfi_")))
        eng.release_workspace()
        assert eng.workspace_bytes() == 0
        eng.close()
        result[name] = row
    print(json.dumps(result))


if __name__ == "__main__":
    main()
