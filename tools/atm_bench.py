"""Device-resident ATM-lite or ATM-base at 1080p (one vfi_atm_forward / vfi_atm_forward_ensemble per new frame), seeded weights.

    python tools/atm_bench.py [--variant lite|base] [--iters 5] [--height 1080 --width 1920] [--no-parity] [--no-ensemble] [--uhd [--uhd-parity On]] [--out profiles/atm_bench.json]

Prints one JSON line (and writes it to --out: lite's result is the file's top level, base's its "base" entry; the other one is kept).  Per global-motion mode ("On", "Off (fastest)" and, unless --no-ensemble, "On with Ensemble (slowest)" with the losses and the level it chose and
its time over the same run's "On" time): ms per new frame, the median of `iters`
forward calls timed with device events around the call (frames already on the device, workspace allocated by two warm-up calls); the
workspace size; the library's per-kernel event trace (vfi_trace_*) of one extra call: the share of the new kernels (atm_attn_cross,
atm_attn_self, atm_motion_mlp, atm_dwconv, atm_gather_taps, atm_depth_to_space, atm_blend, atm_out) and of the layer objects; and, unless
--no-parity, the in-run parity of the timed frame against the float32 restatement (tests/atm_restated.py, tests/atm_base_restated.py, tests/atm_ensemble_restated.py) on the
CPU: max |d| over every pixel, asserted <= 1e-3.

--uhd adds a 2160x3840 leg after the first one (the result's "2160x3840" entry, the same figures per mode): the tool turns config.yaml's
atm_large_frames key on for itself, as it does atm_base.  Its parity is a one-off per-pixel comparison with the same float32 restatement,
minutes of CPU per mode, for the modes --uhd-parity lists (comma-separated; default "On", "" for none); the gate is the same 1e-3, and the
first leg's figure of the same run stands beside it as the yardstick."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=("lite", "base"), default="lite")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--no-parity", action="store_true", help="skip the CPU restatement of the timed frame")
    ap.add_argument("--no-ensemble", action="store_true", help="skip the ensemble leg")
    ap.add_argument("--uhd", action="store_true", help="add a 2160x3840 leg (atm_large_frames on)")
    ap.add_argument("--uhd-parity", default="On", help="modes whose 2160x3840 frame is compared with the CPU restatement (comma-separated)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "atm_bench needs the GPU"
    from pkgload import load_package

    load_package()
    import atm_base_restated
    import atm_ensemble_restated
    import atm_restated
    import cain_restated
    from cfi_amd import _lib, ckpt
    from cfi_amd.atm import ENSEMBLE, AtmEngine, padded_size
    from cfi_amd.atm_spec import seeded_state_dict

    restated, keys = atm_restated, {}
    if args.variant == "base":      # opt-in: the tool turns the key on for itself
        restated, keys["atm_base"] = atm_base_restated, True
    if args.uhd:
        keys["atm_large_frames"] = True
    real_config = ckpt.load_config
    ckpt.load_config = lambda: dict(real_config(), **keys)
    if not args.no_ensemble:
        _lib.use_test_build()      # the ensemble's record is a test tap (include/vfi_hip_test_atm.h); the kernels are the product library's objects
    eng = AtmEngine(seeded_state_dict(atm_restated.SEED, args.variant), args.variant)
    lib = _lib.load()
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    modes = dict(atm_restated.MODES)
    if not args.no_ensemble:
        modes[atm_ensemble_restated.ENSEMBLE] = ENSEMBLE

    over = []      # parity figures over the gate: the JSON line is printed first, then the tool fails

    def run_size(H, W, parity_modes):
        """-> {"workload": ..., mode: figures}: every mode at one frame size; parity for the modes listed"""
        Hp, Wp = padded_size(H, W)
        frames = cain_restated.seeded_frames(2, H, W, 3, 31)
        f = frames.cuda()
        res = {"workload": f"atm-{args.variant} {H}x{W} (padded {Hp}x{Wp}), device-resident, ms per new frame", "iters": args.iters}
        for mode, gm in modes.items():
            out = torch.empty((H, W, 3), device="cuda")
            call = lambda: eng.forward(f[0], f[1], gm, out)      # noqa: E731
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            assert torch.isfinite(out).all(), f"ATM-{args.variant} at {H}x{W}, {mode}: non-finite output"
            samples = []
            for _ in range(args.iters):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
                b.synchronize()
                samples.append(a.elapsed_time(b))
            r = {"ms_per_frame": round(statistics.median(samples), 3), "ms_samples": [round(t, 3) for t in samples], "workspace_bytes": eng.workspace_bytes()}
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
            total = sum(v[1] for v in rows.values()) or 1.0
            r["trace_total_ms"] = round(total, 3)
            r["trace_new_kernels"] = {k: [v[0], round(v[1], 3), round(v[1] / total, 3)] for k, v in rows.items() if k.startswith("atm_")}
            r["trace_layer_objects_share"] = round(sum(v[1] for k, v in rows.items() if k.startswith(("conv", "deconv"))) / total, 3)
            r["trace_rows"] = {k: [v[0], round(v[1], 3)] for k, v in sorted(rows.items(), key=lambda kv: -kv[1][1])[:12]}
            print(f"{mode}: {r['ms_per_frame']} ms per frame, workspace {r['workspace_bytes']} bytes", file=sys.stderr, flush=True)
            if gm == ENSEMBLE:
                r["losses"], r["level"] = eng.ensemble_record()
                r["over_on"] = round(r["ms_per_frame"] / res["On"]["ms_per_frame"], 3)
            if mode in parity_modes:
                x = frames.permute(0, 3, 1, 2).contiguous()
                with torch.no_grad():
                    if gm == ENSEMBLE:
                        sd32 = atm_ensemble_restated.state_dict_as(args.variant, torch.float32)
                        want = atm_ensemble_restated.ensemble_frame(args.variant, sd32, x[0:1], x[1:2])[0].permute(1, 2, 0)
                    else:
                        want = restated.atm_frame(restated.state_dict_as(torch.float32), x[0:1], x[1:2], gm)[0].permute(1, 2, 0)
                r["parity_max_abs_vs_float32_restatement"] = float((out.cpu() - want).abs().max())
                print(f"{mode} {H}x{W}: parity max |d| {r['parity_max_abs_vs_float32_restatement']:.3e}", file=sys.stderr, flush=True)
                if r["parity_max_abs_vs_float32_restatement"] > atm_restated.TOL:
                    over.append((f"{H}x{W}", mode, r["parity_max_abs_vs_float32_restatement"]))
            res[mode] = r
        eng.release_workspace()
        return res

    res = run_size(args.height, args.width, () if args.no_parity else tuple(modes))
    if args.uhd:
        res["2160x3840"] = run_size(2160, 3840, tuple(m for m in args.uhd_parity.split(",") if m))
    eng.close()
    print(json.dumps(res), flush=True)
    if args.out:
        doc = {}
        if os.path.exists(args.out):
            with open(args.out) as fh:
                doc = json.load(fh)
        doc = dict(res, **({"base": doc["base"]} if "base" in doc else {})) if args.variant == "lite" else dict(doc, base=res)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc) + "\n")
    assert not over, f"parity over the gate of {atm_restated.TOL}: {over}"


if __name__ == "__main__":
    main()
