"""Device-resident AMT-S / AMT-L / AMT-G at 1080p (one vfi_amt_forward per frame pair with all of the pair's timesteps), seeded weights.

    python tools/amt_bench.py [--iters 5] [--variants S,L | --variant G [--large-frames]] [--trace]

Prints one JSON line.  Per variant: ms per NEW frame at multiplier 2 (one timestep per pair) and at multiplier 8 (seven timesteps per
pair), each the median of `iters` forward calls timed with device events around the call (frames already on the device, workspace
allocated by two warm-up calls); the per-pair and per-timestep parts those two figures imply (pair = what runs once per call: pad, mean,
feature encoder, pyramid encoders, pooled maps); the workspace size beside the bytes of the reference's correlation volumes at this size
(two directions, four levels) and of one level-0 volume; and with --trace the library's per-kernel event trace (vfi_trace_*) of one
extra 8x call: the share of the new kernels (amt_lookup, amt_pool2, conv7x7, amt_warps, amt_out, ...) and of the layer objects.
AMT-G (the tool turns the amt_g key on for its own process; every variant's output is asserted finite): with --trace also the kernel only
the two high blocks launch, amt_upsample, with the bytes it has to move in the 8x call — its 1/8-resolution input once per launch, its
1/4- and 1/2-resolution outputs once — over its traced time, as a fraction of the 8.0 TB/s HBM peak (the kernel is bandwidth-bound).

    python tools/amt_bench.py --uhd [--parity] [--out profiles/amt_bench.json]

--uhd is a run of its own: AMT-G at 1080x1920 and at 2160x3840 on ONE object, at multipliers 2 and 8, with config.yaml's amt_g and
amt_large_frames keys turned on for the tool's own process (the 1080p leg therefore runs with the key on).  Per size: ms per new frame
as above and the workspace; for 2160x3840 also its ratio to four 1080p frames of the same run, and the LARGE launches of one forward as
vfi_test_large_launches logs them (the tool loads the test build for that tap; the kernels are the product library's objects).  With
--parity: max |d| over every pixel of one 2160x3840 frame at t = 0.5 against the float32 restatement (tests/amt_g_restated.py) on the host,
minutes of CPU, and the 1080p figure of the same run beside it; the gate is 1e-3, checked after the JSON line is printed.  The result is
printed as one JSON line and, with --out, stored as that file's "uhd" entry (the rest of the file is kept)."""
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


def _time_calls(call, iters):
    samples = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        samples.append(a.elapsed_time(b))
    return samples


def run_uhd(args):
    from pkgload import load_package

    load_package()
    import amt_g_restated
    import cain_restated
    from cfi_amd import _lib, ckpt
    from cfi_amd.amt import AmtEngine, padded_size
    from cfi_amd.amt_spec import seeded_state_dict

    real_config = ckpt.load_config
    ckpt.load_config = lambda: dict(real_config(), amt_g=True, amt_large_frames=True)
    _lib.use_test_build()      # vfi_test_large_launches is a test tap (include/vfi_hip_test_large.h); the kernels are the product library's objects
    lib = _lib.load()
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    res = {"workload": "AMT-G, device-resident, ms per new frame; amt_g and amt_large_frames on", "iters": args.iters}
    over = []
    try:
        eng = AmtEngine(seeded_state_dict("G", amt_g_restated.SEED))
        for H, W in ((1080, 1920), (2160, 3840)):
            Hp, Wp = padded_size(H, W)
            frames = cain_restated.seeded_frames(2, H, W, 3, 31)
            f = frames.cuda()
            r = {"padded": [Hp, Wp]}
            for m in (2, 8):
                ts = [k / m for k in range(1, m)]
                out = torch.empty((len(ts), H, W, 3), device="cuda")
                call = lambda: eng.forward(f[0], f[1], ts, out)      # noqa: E731
                for _ in range(2):
                    call()
                torch.cuda.synchronize()
                assert torch.isfinite(out).all(), f"AMT-G at {H}x{W}, multiplier {m}: non-finite output"
                samples = _time_calls(call, args.iters)
                r[f"x{m}_ms_per_pair"] = round(statistics.median(samples), 3)
                r[f"x{m}_ms_per_frame"] = round(statistics.median(samples) / len(ts), 3)
                r[f"x{m}_ms_samples"] = [round(t, 3) for t in samples]
                del out
            r["workspace_bytes"] = eng.workspace_bytes()
            log = (C.c_int32 * (6 * 256))()
            lib.vfi_test_large_launches(log, 256)
            one = torch.empty((1, H, W, 3), device="cuda")
            eng.forward(f[0], f[1], [0.5], one)
            torch.cuda.synchronize()
            n = min(lib.vfi_test_large_launches(log, 256), 256)
            r["large_launches"] = [list(log[6 * i:6 * i + 6]) for i in range(n)]      # family (2 direct, 3 Winograd), Hin, Win, in_cs, Cin_p, Cout
            print(f"{H}x{W}: {r['x2_ms_per_frame']} / {r['x8_ms_per_frame']} ms per frame at 2x / 8x, workspace {r['workspace_bytes']} bytes, "
                  f"{n} LARGE launches", file=sys.stderr, flush=True)
            if args.parity:
                x = frames.permute(0, 3, 1, 2).contiguous()
                sd32 = {k: v.float() for k, v in amt_g_restated.state_dict64().items()}
                with torch.no_grad():
                    want = amt_g_restated.amt_g_forward(sd32, x[0:1], x[1:2], (0.5,))[0].permute(1, 2, 0)
                r["parity_max_abs_vs_float32_restatement"] = float((one[0].cpu() - want).abs().max())
                print(f"{H}x{W}: parity max |d| {r['parity_max_abs_vs_float32_restatement']:.3e}", file=sys.stderr, flush=True)
                if r["parity_max_abs_vs_float32_restatement"] > amt_g_restated.TOL:
                    over.append((f"{H}x{W}", r["parity_max_abs_vs_float32_restatement"]))
            else:
                r["parity_max_abs_vs_float32_restatement"] = None      # not measured in this run (--parity)
            del one, f
            eng.release_workspace()
            res[f"{H}x{W}"] = r
        eng.close()
    finally:
        ckpt.load_config = real_config
    for m in (2, 8):
        res[f"x{m}_2160x3840_over_four_1080p_frames"] = round(res["2160x3840"][f"x{m}_ms_per_frame"] / (4 * res["1080x1920"][f"x{m}_ms_per_frame"]), 3)
    print(json.dumps(res), flush=True)
    if args.out:
        doc = {}
        if os.path.exists(args.out):
            with open(args.out) as fh:
                doc = json.load(fh)
        doc["uhd"] = res
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc) + "\n")
    assert not over, f"parity over the gate of {amt_g_restated.TOL}: {over}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--variants", default="S,L")
    ap.add_argument("--variant", default=None, help="one variant (S, L or G); overrides --variants")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--trace", action="store_true", help="per-kernel event trace of one extra 8x call (kernel shares)")
    ap.add_argument("--large-frames", action="store_true", help="with --variant G: run with config.yaml's amt_large_frames on (the engine gives the object the switch)")
    ap.add_argument("--uhd", action="store_true", help="AMT-G at 1080p and 2160x3840 in one run (amt_g and amt_large_frames on); see the module text")
    ap.add_argument("--parity", action="store_true", help="with --uhd: compare one frame per size with the float32 restatement on the host")
    ap.add_argument("--out", default=None, help="with --uhd: store the result as this JSON file's \"uhd\" entry")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "amt_bench needs the GPU"
    if args.uhd:
        return run_uhd(args)
    from pkgload import load_package

    load_package()
    from cfi_amd import _lib
    from cfi_amd.amt import AmtEngine, padded_size
    from cfi_amd.amt_spec import seeded_state_dict

    H, W = args.height, args.width
    Hp, Wp = padded_size(H, W)
    h8, w8 = Hp // 8, Wp // 8
    g = torch.Generator().manual_seed(3)
    f = torch.rand(2, H, W, 3, generator=g).cuda()
    res = {"workload": f"amt {H}x{W} (padded {Hp}x{Wp}), device-resident, ms per new frame", "iters": args.iters,
           "reference_volume_bytes": 2 * 4 * h8 * w8 * sum((h8 >> l) * (w8 >> l) for l in range(4)), "reference_level0_volume_bytes": 4 * (h8 * w8) ** 2}
    variants = [args.variant] if args.variant else args.variants.split(",")
    from cfi_amd import ckpt

    real_config = ckpt.load_config
    if "G" in variants:      # AMT-G is opt-in (config.yaml's amt_g); this tool asks for it by name, and puts the real function back
        ckpt.load_config = lambda: dict(real_config(), amt_g=True, amt_large_frames=args.large_frames)
    try:
        for variant in variants:
            eng = AmtEngine(seeded_state_dict(variant, 1))
            r = {}
            for m in (2, 8):
                ts = [k / m for k in range(1, m)]
                out = torch.empty((len(ts), H, W, 3), device="cuda")
                call = lambda: eng.forward(f[0], f[1], ts, out)      # noqa: E731
                for _ in range(2):
                    call()
                torch.cuda.synchronize()
                assert torch.isfinite(out).all(), f"AMT-{variant} at {H}x{W}, multiplier {m}: non-finite output"
                samples = []
                for _ in range(args.iters):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    call()
                    b.record()
                    b.synchronize()
                    samples.append(a.elapsed_time(b))
                r[f"x{m}_ms_per_pair"] = round(statistics.median(samples), 3)
                r[f"x{m}_ms_per_frame"] = round(statistics.median(samples) / len(ts), 3)
                r[f"x{m}_ms_samples"] = [round(t, 3) for t in samples]
            per_t = (r["x8_ms_per_pair"] - r["x2_ms_per_pair"]) / 6
            r["per_timestep_ms"], r["per_pair_ms"] = round(per_t, 3), round(r["x2_ms_per_pair"] - per_t, 3)
            r["workspace_bytes"] = eng.workspace_bytes()
            if args.trace:
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
                high = rows.pop("amt_high_blocks", None)      # an outer scope around the high blocks' kernels, not a kernel: kept out of the sum
                total = sum(v[1] for v in rows.values()) or 1.0
                if high:
                    r["trace_x8_high_blocks"] = [high[0], round(high[1], 3), round(high[1] / total, 3)]
                new = ("amt_", "conv7x7")
                r["trace_x8_total_ms"] = round(total, 3)
                r["trace_x8_new_kernels"] = {k: [v[0], round(v[1], 3), round(v[1] / total, 3)] for k, v in rows.items() if k.startswith(new)}
                r["trace_x8_layer_objects_share"] = round(sum(v[1] for k, v in rows.items() if k.startswith(("conv", "deconv")) and not k.startswith("conv7x7")) / total, 3)
                if variant == "G" and "amt_upsample" in rows:
                    # vfi_amt_upsample_lrelu per timestep: convc1's 256 channels at 1/8 resolution read twice (x2 and x4), written at 1/4 and 1/2
                    px8 = h8 * w8
                    nbytes = 7 * 4 * 256 * (2 * px8 + 4 * px8 + 16 * px8)
                    ms = rows["amt_upsample"][1]
                    r["upsample_bytes_x8_call"], r["upsample_ms_x8_call"] = nbytes, round(ms, 3)
                    r["upsample_bytes_per_s"] = round(nbytes / (ms * 1e-3), 0)
                    r["upsample_share_of_hbm_peak_8TBps"] = round(nbytes / (ms * 1e-3) / 8.0e12, 3)
                r["trace_x8_rows"] = {k: [v[0], round(v[1], 3)] for k, v in sorted(rows.items(), key=lambda kv: -kv[1][1])[:12]}
            res["AMT-" + variant] = r
            eng.close()
    finally:
        ckpt.load_config = real_config
    print(json.dumps(res))


if __name__ == "__main__":
    main()
