"""Device-resident FLAVR at 1080p (one model call per interpolated frame: a window of four frames), seeded weights.

    python tools/flavr_bench.py [--iters 5] [--windows 1] [--n-outputs 1] [--trace] [--cpu]

Prints one JSON line: ms per interpolated frame (median of `iters` vfi_flavr_forward calls of `windows` windows, timed with device
events around the call; frames already on the device), frames/s, the workspace size, direct-form TFLOP/s, and with --trace the
library's per-kernel event trace (vfi_trace_*) of one extra call: the share of the 3x3x3 / (3,4,4) layers (the rows named conv3x3s*,
deconv4x4s2_*: the library's Winograd and direct MFMA kernels), their direct-form and executed TFLOP/s and the executed fraction of the
fp32 MFMA peak, and the rows of the new kernels (flavr_*).  The committed outputs are profiles/flavr_bench.json and
profiles/flavr_kernel_stats.txt (a `rocprofv3 --kernel-trace --stats` run of this script).

FLOP model per frame at the padded size Hp x Wp (1088 x 1920), T = 4 time slices, direct form:
  Conv3d 3x3x3              2 * 27 * Cin * Cout * T * h_out * w_out
  ConvTranspose3d (3,4,4)   2 * 48 * Cin * Cout * T * h_in * w_in          (stride (1,2,2): 48 taps leave every input value)
  stem (3,7,7) / 1x1x1 / feature_fuse / outconv 7x7 likewise.
Executed: a stride-1 3x3 layer on the Winograd F(2x2,3x3) kernel multiplies 4/9 of the direct count; a transposed layer on it (as one
3x3 layer with 4 Cout channels) 16 * 3 Cin * Cout per input pixel = its direct count; stride-2 layers run direct.
Peak (MI355X_MICROARCH.md): fp32 MFMA 157.3 TFLOP/s."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MFMA_PEAK = 157.3e12
T = 4


def flop_model(Hp, Wp):
    """-> (direct flops of the 3x3x3 / (3,4,4) layers, executed flops of them with every stride-1 layer on Winograd, all other direct flops)"""
    P2, P4, P8 = Hp * Wp // 4, Hp * Wp // 16, Hp * Wp // 64
    conv = lambda cin, cout, p: 2 * 27 * cin * cout * T * p          # noqa: E731
    s1 = [conv(64, 64, P2) * 4,                                      # layer1
          conv(128, 128, P4) * 3, conv(256, 256, P8) * 3,            # layer2 / layer3 after their stride-2 first convolution
          conv(256, 512, P8) + conv(512, 512, P8) * 3,               # layer4
          conv(512, 256, P8), conv(128, 64, P2)]                     # decoder.0, decoder.3
    s2 = [conv(64, 128, P4), conv(128, 256, P8)]
    up = [2 * 48 * 512 * 128 * T * P8, 2 * 48 * 256 * 64 * T * P4, 2 * 48 * 128 * 64 * T * P2]
    other = (2 * 3 * 147 * 64 * T * P2 + 2 * 64 * 128 * T * P4 + 2 * 128 * 256 * T * P8 + 2 * 256 * 512 * T * P8 +
             2 * 256 * 64 * Hp * Wp + 2 * 64 * 49 * 3 * Hp * Wp)
    direct = sum(s1) + sum(s2) + sum(up)
    return direct, sum(s1) * 4 / 9 + sum(s2) + sum(up), other


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--windows", type=int, default=1)
    ap.add_argument("--n-outputs", type=int, default=1)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--trace", action="store_true", help="per-kernel event trace of one extra call (kernel split)")
    ap.add_argument("--cpu", action="store_true", help="also time the torch restatement on the host")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "flavr_bench needs the GPU"
    from pkgload import load_package

    load_package()
    import flavr_restated
    from cfi_amd import _lib
    from cfi_amd.flavr import FlavrEngine
    from cfi_amd.flavr_spec import seeded_state_dict

    H, W, N = args.height, args.width, args.windows
    Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    sd = seeded_state_dict(1, args.n_outputs)
    eng = FlavrEngine(sd)
    g = torch.Generator().manual_seed(3)
    f = torch.rand(N + 3, H, W, 3, generator=g)
    fd = f.cuda()
    out = torch.empty((N, H, W, 3), device="cuda")
    call = lambda: eng.forward([fd[i + j] for i in range(N) for j in range(4)], out)   # noqa: E731
    for _ in range(2):
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
    ms = statistics.median(ts) / N
    direct, executed, other = flop_model(Hp, Wp)
    res = {"workload": f"flavr {H}x{W} x2 (n_outputs {args.n_outputs}), device-resident", "windows_per_call": N, "ms_per_frame": round(ms, 3),
           "fps": round(1000 / ms, 2), "ms_samples": [round(t, 3) for t in ts], "workspace_gb": round(eng.workspace_bytes() / 1e9, 3),
           "direct_tflop_3x3x3": round(direct / 1e12, 3), "direct_tflop_other": round(other / 1e12, 3),
           "direct_tflops": round((direct + other) / ms / 1e9, 2), "mfma_peak_floor_ms": round(direct / MFMA_PEAK * 1e3, 1)}
    if args.trace:
        import ctypes as C

        lib = _lib.load()
        lib.vfi_trace_reset()
        lib.vfi_trace_enable(1)
        call()
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
        total = sum(v[1] for v in rows.values())
        res["trace_rows"] = rows      # name -> (calls, total ms) over this one call of N windows
        res["trace_total_ms_per_frame"] = round(total / N, 3)
        big = {k: v for k, v in rows.items() if k.startswith("conv3x3s") or k.startswith("deconv4x4s2_")}
        if big:
            t = sum(v[1] for v in big.values()) / N
            res["layers_3x3x3"] = {"launches": sum(v[0] for v in big.values()) // N, "ms_per_frame": round(t, 3), "share_of_call": round(t * N / total, 3),
                                   "direct_tflops": round(direct / t / 1e9, 2), "executed_tflops": round(executed / t / 1e9, 2),
                                   "executed_mfma_frac": round(executed / (t / 1e3) / MFMA_PEAK, 3)}
        res["new_kernels_ms_per_frame"] = {k: round(v[1] / N, 3) for k, v in rows.items() if k.startswith("flavr_")}
    if args.cpu:
        torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
        x = f[:4].permute(0, 3, 1, 2).contiguous()
        t0 = time.perf_counter()
        with torch.no_grad():
            flavr_restated.flavr_forward(sd, [x[i:i + 1] for i in range(4)])
        res["cpu_restatement_s"] = round(time.perf_counter() - t0, 2)
        res["cpu_threads"] = torch.get_num_threads()
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
