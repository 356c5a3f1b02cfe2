"""Device-resident SepConv++ at 1080p, multiplier 2 (one model call per interpolated frame), seeded weights.

    python tools/sepconv_bench.py [--iters 10] [--pairs 1] [--trace] [--ab]

Prints one JSON line: ms per interpolated frame (median of `iters` vfi_sepconvnet_forward calls of `pairs` pairs, timed with device
events around the call after 3 warm-up calls; frames already on the device), frames/s, direct-form TFLOP/s of the convolutions, the
workspace per pair, and with --trace the per-kernel split of one extra call from the library's event trace (vfi_trace_*), including
the fused output stage's time and fraction of the fp32 VALU peak.  The committed outputs are profiles/sepconv_bench.json and
profiles/sepconv_kernel_stats.txt (a `rocprofv3 --kernel-trace --stats` run of this script).  --ab (test library) also times the A/B forms:
the heads' first convs as four 64 -> 64 layers (option sepconv_split_heads) and the output stage reading the heads NHWC at their 208-float
pixel stride instead of planar (option sepconv_planar = 0).

FLOP model (direct form, per interpolated frame at 1080p): sum over the 3x3 convolutions of 2 * 9 * Cin * Cout * Hout * Wout.  The output
stage: 2 frames x 4 lanes (r, g, b and the normaliser) x (51 * 51 + 51) FMAs per pixel = 2 FLOP each; its useful part (3 colour channels,
as the issue counts it) is 2 x 3 x 51 * 52 FMAs.  fp32 VALU peak (MI355X_MICROARCH.md): 157.3 TFLOP/s with packed FMAs."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VALU_PEAK = 157.3e12
CH = (32, 64, 128, 256, 512)


def conv_flop(H, W):
    Hp, Wp = H + H % 2, W + W % 2
    hs, ws = [Hp], [Wp]
    for _ in range(4):
        hs.append((hs[-1] + 1) // 2), ws.append((ws[-1] + 1) // 2)
    px = [h * w for h, w in zip(hs, ws)]
    f = 2 * 2 * 9 * 3 * 16 * px[0]                # netInput on both frames
    enc = sum(2 * 9 * (CH[r - 1] * CH[r] + CH[r] * CH[r]) * px[r] for r in range(1, 5))
    hor = sum(2 * 9 * 2 * CH[r] * CH[r] * px[r] for r in range(1, 5))
    ver = sum(2 * 9 * (CH[r + 1] * CH[r] + CH[r] * CH[r]) * (2 * hs[r + 1]) * (2 * ws[r + 1]) for r in range(1, 4))
    heads = 4 * 2 * 9 * (64 * 64 + 64 * 51) * px[0]
    return {"input": f, "encoder": enc, "decoder_hor": hor, "decoder_ver": ver, "heads": heads}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=1)
    ap.add_argument("--trace", action="store_true", help="per-kernel event trace of one extra call (kernel split)")
    ap.add_argument("--ab", action="store_true", help="also time the A/B forms (needs the test library)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sepconv_bench needs the GPU"
    from pkgload import load_package

    load_package()
    from cfi_amd import _lib

    if args.ab:
        _lib.use_test_build()
    from cfi_amd.sepconv import SepconvEngine
    from cfi_amd.sepconv_spec import seeded_state_dict

    H, W, N = 1080, 1920, args.pairs
    eng = SepconvEngine(seeded_state_dict(1))
    g = torch.Generator().manual_seed(3)
    fd = torch.rand(N + 1, H, W, 3, generator=g).cuda()
    out = torch.empty((N, H, W, 3), device="cuda")
    call = lambda: eng.forward([fd[i] for i in range(N)], [fd[i + 1] for i in range(N)], out)   # noqa: E731

    def timed():
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return ts

    def split(fn):
        lib = _lib.load()
        lib.vfi_trace_reset()
        lib.vfi_trace_enable(1)
        fn()
        torch.cuda.synchronize()
        lib.vfi_trace_enable(0)
        buf = C.create_string_buffer(1 << 20)
        lib.vfi_trace_report(buf, len(buf))
        rows = {}
        for line in buf.value.decode().splitlines():
            parts = line.split()
            if len(parts) >= 3:
                try:
                    rows[parts[0]] = (int(parts[1]), float(parts[2]))
                except ValueError:
                    pass
        return rows

    ts = timed()
    ms = statistics.median(ts) / N
    fl = conv_flop(H, W)
    res = {"workload": "sepconv++ 1080p x2, device-resident", "pairs_per_call": N, "ms_per_frame": round(ms, 3), "fps": round(1000 / ms, 2),
           "ms_samples": [round(t, 3) for t in ts], "conv_direct_tflop": round(sum(fl.values()) / 1e12, 3),
           "conv_direct_tflop_by_part": {k: round(v / 1e12, 3) for k, v in fl.items()},
           "conv_direct_tflops": round(sum(fl.values()) / ms / 1e9, 2), "workspace_bytes_per_pair": eng.workspace_bytes(), "target_ms": 20.0}
    if args.trace:
        rows = split(call)
        res["trace_rows"] = rows      # name -> (calls, total ms) over this one call of N pairs
        if "sepconv_pair_out" in rows:
            cnt, tot = rows["sepconv_pair_out"]
            t = tot / cnt / 1e3
            executed = 2 * 4 * (K := 51) * (K + 1) * 2 * H * W
            useful = 2 * 3 * K * (K + 1) * 2 * H * W
            res["pair_out"] = {"ms": round(tot / cnt, 4), "target_ms": 1.4, "executed_valu_frac": round(executed / t / VALU_PEAK, 3),
                               "useful_valu_frac": round(useful / t / VALU_PEAK, 3)}
    if args.ab:
        lib = _lib.load()
        ref = out.clone()
        for name, val in (("sepconv_split_heads", 1), ("sepconv_planar", 0)):
            assert lib.vfi_test_set_option(name.encode(), val) == 0
            t = timed()
            rows = split(call)
            keys = ("conv3x3s1_64to256", "conv3x3s1_64to64", "conv3x3s1_64to51", "sepnet_heads_planar", "sepconv_pair_out")
            res[f"ab_{name}={val}"] = {"ms_per_frame": round(statistics.median(t) / N, 3), "bit_identical": bool(torch.equal(out, ref)),
                                       "max_abs_diff": float((out - ref).abs().max()),
                                       "kernels_ms": {k: round(rows[k][1] / N, 3) for k in keys if k in rows},
                                       "workspace_bytes_per_pair": eng.workspace_bytes()}
            assert lib.vfi_test_set_option(name.encode(), 1 - val) == 0
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
