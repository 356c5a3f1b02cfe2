"""Device-resident CAIN at 1080p, multiplier 2 (one model call per interpolated frame), seeded weights.

    python tools/cain_bench.py [--iters 10] [--pairs 1] [--trace]

Prints one JSON line: ms per interpolated frame (median of `iters` vfi_cain_forward calls of `pairs` pairs, timed with device events
around the call; frames already on the device), frames/s, executed and direct-form TFLOP/s, the time and fraction of peak of the
dominant kernel and of the channel-attention pass (from the library's per-kernel event trace, vfi_trace_*, with --trace), and the CPU
time of the torch restatement (tests/cain_restated.py) on the same tensors.  The committed outputs are profiles/cain_bench.json and
profiles/cain_kernel_stats.txt (a `rocprofv3 --kernel-trace --stats` run of this script).

FLOP model (per interpolated frame, feature map h x w = 144 x 240 at 1080p): 126 convolutions 192 -> 192 and one 384 -> 192, 3x3:
direct form 2 * 9 * Cin * 192 * h * w; executed (Winograd F(2x2,3x3): 16 MACs per 4 outputs instead of 36) 4/9 of it.
Peaks (MI355X_MICROARCH.md): fp32 MFMA 157.3 TFLOP/s, HBM 8.0 TB/s.  Channel-attention bytes per RCAB: t read twice, x read, out
written = 4 * h * w * 192 * 4."""
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
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=1)
    ap.add_argument("--trace", action="store_true", help="per-kernel event trace of one extra call (kernel split)")
    ap.add_argument("--cpu", action="store_true", help="also time the torch restatement on the host")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cain_bench needs the GPU"
    from pkgload import load_package

    load_package()
    import cain_restated
    from cfi_amd import _lib
    from cfi_amd.cain import CainEngine

    H, W, N = 1080, 1920, args.pairs
    sd = cain_restated.seeded_state_dict(1)
    eng = CainEngine(sd)
    g = torch.Generator().manual_seed(3)
    f = torch.rand(N + 1, H, W, 3, generator=g)
    fd = f.cuda()
    out = torch.empty((N, H, W, 3), device="cuda")
    call = lambda: eng.forward([fd[i] for i in range(N)], [fd[i + 1] for i in range(N)], out)   # noqa: E731
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
    ms = statistics.median(ts) / N
    h, w = 1152 // 8, 1920 // 8
    direct = 2 * 9 * 192 * h * w * (126 * 192 + 384)
    res = {"workload": "cain 1080p x2, device-resident", "pairs_per_call": N, "ms_per_frame": round(ms, 3), "fps": round(1000 / ms, 2),
           "ms_samples": [round(t, 3) for t in ts], "direct_tflops": round(direct / ms / 1e9, 2),
           "executed_tflops": round(direct * 4 / 9 / ms / 1e9, 2), "target_ms": 25.0}
    if args.trace:
        lib = _lib.load()
        lib.vfi_trace_reset()
        lib.vfi_trace_enable(1)
        call()
        torch.cuda.synchronize()
        lib.vfi_trace_enable(0)
        import ctypes as C

        buf = C.create_string_buffer(1 << 20)
        lib.vfi_trace_report(buf, len(buf))
        res["trace"] = buf.value.decode()
        rows = {}
        for line in res["trace"].splitlines():
            parts = line.split()
            if len(parts) >= 3:
                try:
                    rows[parts[0]] = (int(parts[1]), float(parts[2]))
                except ValueError:
                    pass
        res["trace_rows"] = rows
        # rows: name -> (calls, total ms) over this one call of N pairs
        if "conv3x3s1_192to192" in rows:
            cnt, tot = rows["conv3x3s1_192to192"]
            per_s = tot / cnt / 1e3
            executed = 2 * 9 * 192 * 192 * h * w * N * 4 / 9
            res["dominant_kernel"] = {"name": "conv3x3s1_192to192 (Winograd)", "calls": cnt, "ms_per_call": round(tot / cnt, 4),
                                      "share_of_call": round(tot / sum(v[1] for v in rows.values()), 3),
                                      "executed_mfma_frac": round(executed / per_s / MFMA_PEAK, 3)}
        ca = {k: v for k, v in rows.items() if k.startswith("cain_ca_")}
        if ca:
            tot = sum(v[1] for v in ca.values())
            nbytes = 60 * 4 * h * w * 192 * 4 * N
            res["channel_attention"] = {"ms_per_frame": round(tot / N, 3), "hbm_frac": round(nbytes / (tot / 1e3) / HBM_PEAK, 3),
                                        "kernels": {k: round(v[1] / v[0] * 1e3, 2) for k, v in ca.items()}}   # us per launch
        del res["trace"]
    if args.cpu:
        torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
        x = f[:2].permute(0, 3, 1, 2).contiguous()
        t0 = time.perf_counter()
        with torch.no_grad():
            cain_restated.cain_forward(sd, x[0:1], x[1:2])
        res["cpu_restatement_s"] = round(time.perf_counter() - t0, 2)
        res["cpu_threads"] = torch.get_num_threads()
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
