"""Kernel time and roofline fraction of each op of cfi_amd.ops at the shapes the upstream nodes use (1080p input).

    python tools/ops_bench.py [--iters 20]

One JSON line per op.  ``ms`` is the median of ``iters`` launches timed with events around the op's own kernel launches (no
permutes, no allocations: the buffers are made once; the NCHW softsplat row includes its wrapper's permutes).  The committed
profiles are profiles/ref_ops_bench.jsonl (this output) and profiles/ref_ops_kernel_stats.txt (a ``rocprofv3 --kernel-trace
--stats`` run of this script, per-kernel averages).
Roofline: sepconv and AdaCoF against the f32 VALU peak (157.3 TF, v_pk_fma_f32), the others against HBM (8.0 TB/s spec).
FLOP and byte models are in MODELS below.  softsplat reports the NHWC kernel alone and the NCHW wrapper (its permutes
included) separately."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_PEAK = 157.3e12
HBM_PEAK = 8.0e12
MODELS = {
    "sepconv": "2 * C * Ho * Wo * K^2 FLOP (the reference's count: one multiply-add per tap and channel)",
    "adacof": "C * Ho * Wo * F^2 * 10 FLOP (4 corner products of 2 FLOP + the weight FMA)",
    "correlation": "bytes = 2 * C * H * W * 4 (a, b) + 81 * H * W * 4 (out)",
    "softsplat": "bytes = (2 * C + 2) * H * W * 4 (in, out, flow)",
    "edt": "bytes = 4 * H * W * 4 (data, tmp written and read, out)",
}


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    from pkgload import load_package

    load_package()
    from cfi_amd import _lib, ops

    ops.init()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    s4 = lambda t: (C.c_longlong * 4)(*t.stride())
    lines = []

    def emit(op, shape, ms, work, peak, kind):
        rate = work / (ms * 1e-3)
        lines.append({"op": op, "shape": shape, "ms": round(ms, 4), kind: round(rate / (1e12 if kind == "tflops" else 1e9), 2),
                      "roofline": "valu" if peak == VALU_PEAK else "hbm", "fraction": round(rate / peak, 3), "model": MODELS[op.split(":")[0]]})
        print(json.dumps(lines[-1]), flush=True)

    # sepconv: SepConv++ at 1080p, N 1, C 4 (RGB + ones), K 51
    K, Ho, Wo, Cc = 51, 1080, 1920, 4
    x = torch.rand(1, Cc, Ho + K - 1, Wo + K - 1, device=dev, generator=g)
    ver = torch.rand(1, K, Ho, Wo, device=dev, generator=g) / K
    hor = torch.rand(1, K, Ho, Wo, device=dev, generator=g) / K
    out = torch.empty(1, Cc, Ho, Wo, device=dev)
    ms = _time(lambda: _lib.check(lib.vfi_sepconv(x.data_ptr(), s4(x), ver.data_ptr(), s4(ver), hor.data_ptr(), s4(hor), out.data_ptr(),
                                                  s4(out), 1, Cc, Ho + K - 1, Wo + K - 1, Ho, Wo, K, st()), "sepconv"), args.iters)
    emit("sepconv", [1, Cc, Ho, Wo, K], ms, 2.0 * Cc * Ho * Wo * K * K, VALU_PEAK, "tflops")
    del x, ver, hor, out

    # AdaCoF: STMFNet at 1080p, C 3, F 5, dilation 1
    Fs = 5
    xi = torch.rand(1, 3, Ho + Fs - 1, Wo + Fs - 1, device=dev, generator=g)
    w = torch.rand(1, Fs * Fs, Ho, Wo, device=dev, generator=g) / 25
    oi = torch.randn(1, Fs * Fs, Ho, Wo, device=dev, generator=g)
    oj = torch.randn(1, Fs * Fs, Ho, Wo, device=dev, generator=g)
    out = torch.empty(1, 3, Ho, Wo, device=dev)
    ms = _time(lambda: _lib.check(lib.vfi_adacof(xi.data_ptr(), w.data_ptr(), oi.data_ptr(), oj.data_ptr(), out.data_ptr(), 1, 3,
                                                 Ho + Fs - 1, Wo + Fs - 1, Fs, 1, Ho, Wo, st()), "adacof"), args.iters)
    emit("adacof", [1, 3, Ho, Wo, Fs], ms, 10.0 * 3 * Ho * Wo * Fs * Fs, VALU_PEAK, "tflops")
    hbm = (3 * 25 + 3 + 3) * Ho * Wo * 4
    print(json.dumps({"op": "adacof", "note": "HBM view", "fraction_hbm": round(hbm / (ms * 1e-3) / HBM_PEAK, 3)}), flush=True)
    del xi, w, oi, oj, out

    # correlation: STMFNet's PWC levels 2..6 for a 1080p input (resized to 1088 x 1920, multiples of 64)
    for lvl, Cc in ((2, 32), (3, 64), (4, 96), (5, 128), (6, 196)):
        H, W = 1088 >> lvl, 1920 >> lvl
        a = torch.randn(1, Cc, H, W, device=dev, generator=g)
        b = torch.randn(1, Cc, H, W, device=dev, generator=g)
        out = torch.empty(1, 81, H, W, device=dev)
        ms = _time(lambda: _lib.check(lib.vfi_correlation81(a.data_ptr(), s4(a), b.data_ptr(), s4(b), out.data_ptr(), 1, Cc, H, W, st()),
                                      "correlation"), args.iters)
        emit(f"correlation:L{lvl}", [1, Cc, H, W], ms, (2 * Cc + 81) * H * W * 4.0, HBM_PEAK, "gbps")

    # softsplat: SURVEY config 5's shape [1, 4, 1088, 1920] (the M2M splat), NHWC kernel alone and the NCHW wrapper
    H, W, Cc = 1088, 1920, 4
    xs = torch.rand(1, Cc, H, W, device=dev, generator=g)
    fl = (torch.rand(1, 2, H, W, device=dev, generator=g) - 0.5) * 16
    xn, fn_, on = xs.permute(0, 2, 3, 1).contiguous(), fl.permute(0, 2, 3, 1).contiguous(), torch.empty(1, H, W, Cc, device=dev)
    bytes_ = (2 * Cc + 2) * H * W * 4.0
    ms = _time(lambda: _lib.check(lib.vfi_softsplat_sum(xn.data_ptr(), fn_.data_ptr(), on.data_ptr(), 1, H, W, Cc, st()), "splat"), args.iters)
    emit("softsplat:nhwc_kernel", [1, Cc, H, W], ms, bytes_, HBM_PEAK, "gbps")
    ms = _time(lambda: ops.softsplat_func.apply(xs, fl), args.iters)
    emit("softsplat:nchw_wrapper", [1, Cc, H, W], ms, bytes_, HBM_PEAK, "gbps")

    # EDT at 1080p
    H, W = 1080, 1920
    m = (torch.rand(1, H, W, device=dev, generator=g) > 0.999).float()
    data = ((1 - m) * (H * H + W * W)).contiguous()
    tmp, out = torch.empty_like(data), torch.empty_like(data)
    ms = _time(lambda: _lib.check(lib.vfi_edt(data.data_ptr(), tmp.data_ptr(), out.data_ptr(), 1, H, W, float(H * H + W * W), st()), "edt"),
               args.iters)
    emit("edt", [1, H, W], ms, 4 * H * W * 4.0, HBM_PEAK, "gbps")


if __name__ == "__main__":
    main()
