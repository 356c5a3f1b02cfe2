"""Device-resident SepConv++ at 1080p, multiplier 2 (one model call per interpolated frame), seeded weights.

    python tools/sepconv_bench.py [--iters 10] [--pairs 1] [--trace] [--ab] [--uhd] [--parity]

Prints one JSON line: ms per interpolated frame (median of `iters` vfi_sepconvnet_forward calls of `pairs` pairs, timed with device
events around the call after 3 warm-up calls; frames already on the device), frames/s, direct-form TFLOP/s of the convolutions, the
workspace per pair, and with --trace the per-kernel split of one extra call from the library's event trace (vfi_trace_*), including
the fused output stage's time and fraction of the fp32 VALU peak.  The committed outputs are profiles/sepconv_bench.json and
profiles/sepconv_kernel_stats.txt (a `rocprofv3 --kernel-trace --stats` run of this script).  --ab (test library) also times the A/B forms:
the heads' first convs as four 64 -> 64 layers (option sepconv_split_heads) and the output stage reading the heads NHWC at their 208-float
pixel stride instead of planar (option sepconv_planar = 0).  --uhd (test library; config.yaml's sepconv_large_frames is turned on for this
process) adds a 2160x3840 pair through the banded head stage: ms per frame, workspace bytes, the ratio to four 1080p frames of the same run,
with --trace its kernel split, and the band-height sweep (option sepconv_band_rows: 16 ... the largest legal height).  --parity compares every
pixel of a 1080p frame and, with --uhd, of a 2160x3840 frame with the host fp32 restatement (tests/sepconv_restated.py: features on the
host, which takes minutes at 4K, then the float64 output stage on the device); the gate is 1e-3 per pixel.

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


def smooth_pair(H, W, seed):
    """two smooth frames [2,3,H,W] (a coarse random image up-sampled), as tests/test_gpu_sepconv.py's 1080p case"""
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(seed)
    lo = torch.rand(2, 3, H // 8 + 2, W // 8 + 2, generator=g)
    return F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False)


def parity(eng, H, W):
    """max |engine - restatement| over every pixel of one H x W frame: the network restated on the host in fp32, its output stage in float64
    on the device (as test_forward_1080p_vs_restatement)"""
    import time

    import sepconv_restated
    from cfi_amd.sepconv_spec import seeded_state_dict

    sd = seeded_state_dict(1)
    f = smooth_pair(H, W, 5)
    got = eng.forward([f[0].permute(1, 2, 0).contiguous().cuda()], [f[1].permute(1, 2, 0).contiguous().cuda()])[0].clone()
    print(f"parity {H}x{W}: host restatement running ...", file=sys.stderr, flush=True)
    t0 = time.time()
    with torch.no_grad():
        one, two, heads = sepconv_restated.features(sd, f[0:1], f[1:2])
        print(f"parity {H}x{W}: features after {time.time() - t0:.0f} s", file=sys.stderr, flush=True)
        want, _ = sepconv_restated.pair_out(one.cuda(), two.cuda(), *[h.cuda() for h in heads], H, W)
    d = (got - want[0].permute(1, 2, 0).float()).abs()
    res = {"max_abs_diff": float(d.max()), "mean_abs_diff": float(d.mean()), "gate": 1e-3, "within_gate": bool(d.max() <= 1e-3),
           "finite": bool(torch.isfinite(got).all()), "host_seconds": round(time.time() - t0, 1)}
    del want, d, got
    torch.cuda.empty_cache()
    return res


def timed_call(call, iters):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def uhd(eng, args, timed_fn, split, ms_1080):
    """a 2160x3840 pair with sepconv_large_frames on: time, workspace, ratio to four 1080p frames, kernel split, band-height sweep, parity"""
    from cfi_amd import _lib, ckpt

    real = ckpt.load_config
    ckpt.load_config = lambda: dict(real(), sepconv_large_frames=True)      # this process only
    lib = _lib.load()
    H, W = 2160, 3840
    eng.release_workspace()
    f = smooth_pair(H, W, 7).permute(0, 2, 3, 1).contiguous().cuda()
    out = torch.empty((1, H, W, 3), device="cuda")
    call = lambda: eng.forward([f[0]], [f[1]], out)      # noqa: E731
    ts = timed_fn(call)
    ms = statistics.median(ts)
    ref = out.clone()
    res = {"workload": "sepconv++ 2160x3840 x2, device-resident, banded head stage", "ms_per_frame": round(ms, 3), "ms_samples": [round(t, 3) for t in ts],
           "workspace_bytes_per_pair": eng.workspace_bytes(), "ms_per_1080p_frame_same_run": round(ms_1080, 3),
           "ratio_to_four_1080p_frames": round(ms / (4 * ms_1080), 3), "finite": bool(torch.isfinite(out).all()),
           "conv_direct_tflops": round(sum(conv_flop(H, W).values()) / ms / 1e9, 2)}
    if args.trace:
        res["trace_rows"] = split(call)
    sweep = {}
    top = (2097151 // W - 8) // 8 * 8      # csrc/sepconv_bands.h: max_band_rows
    for bh in (16, 32, 64, 128, 256, top):
        assert lib.vfi_test_set_option(b"sepconv_band_rows", bh) == 0
        try:
            t = timed_fn(call)
            sweep[str(bh)] = {"ms_per_frame": round(statistics.median(t), 3), "workspace_bytes_per_pair": eng.workspace_bytes(),
                              "bit_identical_to_default": bool(torch.equal(out, ref))}
        finally:
            lib.vfi_test_set_option(b"sepconv_band_rows", 0)
    res["band_sweep"] = sweep
    eng.release_workspace()
    del f, out, ref
    torch.cuda.empty_cache()
    if args.parity:
        res["parity"] = parity(eng, H, W)
    ckpt.load_config = real
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=1)
    ap.add_argument("--trace", action="store_true", help="per-kernel event trace of one extra call (kernel split)")
    ap.add_argument("--ab", action="store_true", help="also time the A/B forms (needs the test library)")
    ap.add_argument("--uhd", action="store_true", help="also a 2160x3840 pair behind sepconv_large_frames, with the band-height sweep (needs the test library)")
    ap.add_argument("--parity", action="store_true", help="every pixel against the host fp32 restatement at 1080p (and at 2160x3840 with --uhd)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sepconv_bench needs the GPU"
    from pkgload import load_package

    load_package()
    from cfi_amd import _lib

    if args.ab or args.uhd:
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
    if args.parity:
        res["parity_1080p"] = parity(eng, H, W)
    if args.uhd:
        del fd, out
        res["uhd"] = uhd(eng, args, timed_fn=lambda c: timed_call(c, args.iters), split=split, ms_1080=ms)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
