"""Device-resident FLAVR at 1080p (one model call per interpolated frame: a window of four frames), seeded weights.

    python tools/flavr_bench.py [--iters 5] [--windows 1] [--n-outputs 1] [--trace] [--cpu] [--parity] [--uhd] [--out FILE]

Prints one JSON line: ms per interpolated frame (median of `iters` vfi_flavr_forward calls of `windows` windows, timed with device
events around the call; frames already on the device), frames/s, the workspace size, direct-form TFLOP/s, and with --trace the
library's per-kernel event trace (vfi_trace_*) of one extra call: the share of the 3x3x3 / (3,4,4) layers (the rows named conv3x3s*,
deconv4x4s2_*: the library's Winograd and direct MFMA kernels), their direct-form and executed TFLOP/s and the executed fraction of the
fp32 MFMA peak, and the rows of the new kernels (flavr_*).  --parity compares the timed window's frame with the float32
restatement (tests/flavr_restated.py) at every pixel: max |d| and the count over 1e-3, the project's gate.  --uhd adds a 2160x3840 leg in the
same run, with config.yaml's flavr_large_frames turned on for the tool itself (as tools/atm_bench.py --uhd does with its key): the same
figures under the key "2160x3840", its parity (unless --no-uhd-parity), and the 4K time beside 4x the same run's time at the first size.
The committed output is profiles/flavr_bench.json (`--trace --parity --uhd --out profiles/flavr_bench.json`).

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


def trace_rows(lib, call):
    import ctypes as C

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
    return rows


def heartbeat(what, every=60.0):
    """A line on stderr every minute while the host restatement runs (minutes at 2160x3840); returns the function that stops it"""
    import threading

    stop, t0 = threading.Event(), time.perf_counter()

    def beat():
        while not stop.wait(every):
            print(f"{what}: {time.perf_counter() - t0:.0f} s", file=sys.stderr, flush=True)
    threading.Thread(target=beat, daemon=True).start()
    return stop.set


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--windows", type=int, default=1)
    ap.add_argument("--n-outputs", type=int, default=1)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--trace", action="store_true", help="per-kernel event trace of one extra call (kernel split)")
    ap.add_argument("--cpu", action="store_true", help="also time the torch restatement on the host")
    ap.add_argument("--parity", action="store_true", help="compare the frame with the float32 restatement on the host, every pixel")
    ap.add_argument("--uhd", action="store_true", help="add a 2160x3840 leg (flavr_large_frames on), with its parity")
    ap.add_argument("--no-uhd-parity", action="store_true", help="skip the host restatement of the 2160x3840 frame")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "flavr_bench needs the GPU"
    from pkgload import load_package

    load_package()
    import flavr_restated
    from cfi_amd import _lib, ckpt
    from cfi_amd.flavr import FlavrEngine
    from cfi_amd.flavr_spec import seeded_state_dict

    if args.uhd:      # opt-in: the tool turns the key on for itself
        real_config = ckpt.load_config
        ckpt.load_config = lambda: dict(real_config(), flavr_large_frames=True)
    N = args.windows
    sd = seeded_state_dict(1, args.n_outputs)
    eng = FlavrEngine(sd)
    lib = _lib.load()
    host_threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or max(1, min(32, os.cpu_count() or 1))
    over = []      # parity figures over the gate: the JSON line is printed first, then the tool fails

    def run_size(H, W, trace, parity, cpu):
        Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
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
               "workspace_bytes": eng.workspace_bytes(),
               "direct_tflop_3x3x3": round(direct / 1e12, 3), "direct_tflop_other": round(other / 1e12, 3),
               "direct_tflops": round((direct + other) / ms / 1e9, 2), "mfma_peak_floor_ms": round(direct / MFMA_PEAK * 1e3, 1)}
        print(f"{H}x{W}: {res['ms_per_frame']} ms per frame, workspace {res['workspace_bytes']} bytes", file=sys.stderr, flush=True)
        if trace:
            rows = trace_rows(lib, call)
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
        if parity or cpu:
            torch.set_num_threads(host_threads)
            x = f[:4].permute(0, 3, 1, 2).contiguous()
            got = out[0].cpu()
            del fd, out
            eng.release_workspace()      # the device is idle while the host computes
            stop = heartbeat(f"{H}x{W}: float32 restatement on the host ({host_threads} threads)")
            t0 = time.perf_counter()
            with torch.no_grad():
                want = flavr_restated.flavr_forward(sd, [x[i:i + 1] for i in range(4)])[0].permute(1, 2, 0)
            stop()
            res["cpu_restatement_s"] = round(time.perf_counter() - t0, 2)
            res["cpu_threads"] = host_threads
            if parity:
                d = (got - want).abs()
                res["parity_max_abs_vs_float32_restatement"] = float(d.max())
                res["parity_pixels_over_1e-3"] = int((d.amax(-1) > 1e-3).sum())
                print(f"{H}x{W}: parity max |d| {res['parity_max_abs_vs_float32_restatement']:.3e}, {res['parity_pixels_over_1e-3']} pixels over 1e-3",
                      file=sys.stderr, flush=True)
                if res["parity_max_abs_vs_float32_restatement"] > 1e-3:
                    over.append((f"{H}x{W}", res["parity_max_abs_vs_float32_restatement"]))
        eng.release_workspace()
        return res

    res = run_size(args.height, args.width, args.trace, args.parity, args.cpu)
    if args.uhd:
        u = run_size(2160, 3840, args.trace, not args.no_uhd_parity, False)
        u["ms_4x_first_size"] = round(4 * res["ms_per_frame"], 3)
        u["over_4x_first_size"] = round(u["ms_per_frame"] / (4 * res["ms_per_frame"]), 3)
        res["2160x3840"] = u
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res) + "\n")
    eng.close()
    assert not over, f"parity over the gate of 1e-3: {over}"


if __name__ == "__main__":
    main()
