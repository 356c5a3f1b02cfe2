"""Write the goldens of ATM's multi-scale global-motion ensemble under tests/golden/ by running the REAL reference on this host (CPU),
through oracle/ref_import and the timm shim of tools/make_golden_atm.py:

  atm_ens_net.npz / atm_base_ens_net.npz     the reference's own network_lite / network_base Network with ensemble_global_motion = True on
                      the cases of atm_ensemble_restated.NET_CASES; per case also the three losses (captured around
                      global_alignmentness), the chosen level (the reference's own min / == chain over them), clamped_frac = the share
                      of output values at 0 or 1, and on_diff_max = the largest difference to the same model's "On" output
  atm_ens_node.npz / atm_base_ens_node.npz   the reference's own ATM_VFI node with "On with Ensemble (slowest)" on
                      atm_ensemble_restated.NODE_CASES

One model per case and mode: the shifted blocks keep their first mask (tools/make_golden_atm.py; what that does INSIDE an ensemble forward
is described in tests/atm_ensemble_restated.py).  Inputs are not stored (cain_restated.seeded_frames); outputs are stored compactly
(cain_restated.summary).  Weights: atm_spec.seeded_state_dict(SEED, variant).
Usage: python tools/make_golden_atm_ensemble.py [lite] [base] [probe]   (default: lite base; needs the reference checkout; nothing under oracle/
is changed).  probe: no file is written; the losses of every case, and of the frame seeds 1..8 at the smallest shapes, are printed (how the
cases were chosen: every level must win once per model, with the margin atm_ensemble_restated.MARGIN)."""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_atm as lite_tool  # noqa: E402  (puts the repository and tests/ on sys.path and loads the package)
import atm_ensemble_restated as E  # noqa: E402
import cain_restated  # noqa: E402
from cfi_amd import atm_spec  # noqa: E402
from oracle import ref_import  # noqa: E402

GOLDEN = lite_tool.GOLDEN


def run_case(net_mod, sd, f0, f1):
    """-> (ensemble I_t, "On" I_t, losses) of fresh reference models"""
    losses = []
    real = net_mod.Network.global_alignmentness

    def recording(self, x, im0, im1):
        loss = real(self, x, im0, im1)
        losses.append(loss[0].clone())
        return loss

    outs = []
    for ensemble in (True, False):
        model = net_mod.Network()
        model.load_state_dict(sd)
        model.eval()
        model.global_motion, model.ensemble_global_motion = True, ensemble
        net_mod.Network.global_alignmentness = recording
        try:
            with torch.no_grad():
                outs.append(model(f0, f1)["I_t"])
        finally:
            net_mod.Network.global_alignmentness = real
    assert len(losses) == 3
    return outs[0], outs[1], losses


def make_net(variant, net_mod):
    net, sd = {}, atm_spec.seeded_state_dict(E.SEED, variant)
    for case in E.NET_CASES[variant]:
        f0, f1 = E.frames_of(variant, case)
        out, on, losses = run_case(net_mod, sd, f0, f1)
        assert torch.isfinite(out).all()
        for k, v in cain_restated.summary(out[0].permute(1, 2, 0), E.NET_STRIDE).items():
            net[f"{case}_{k}"] = v
        net[f"{case}_losses"] = np.array([float(l) for l in losses], dtype=np.float32)
        net[f"{case}_level"] = np.array(E.select(losses))
        net[f"{case}_clamped_frac"] = np.array(float(((out <= 0) | (out >= 1)).float().mean()))
        net[f"{case}_on_diff_max"] = np.array(float((out - on).abs().max()))
        print(variant, case, "losses", net[f"{case}_losses"], "level", int(net[f"{case}_level"]), "clamped", float(net[f"{case}_clamped_frac"]),
              "vs On", float(net[f"{case}_on_diff_max"]))
    np.savez_compressed(os.path.join(GOLDEN, E.GOLDEN_PREFIX[variant] + "_net.npz"), seed=np.array(E.SEED), **net)


def make_node(variant):
    cupy = sys.modules.get("cupy")      # einops (vfi_utils.preprocess_frames) probes every importable array library
    if cupy is not None and not hasattr(cupy, "ndarray"):
        cupy.ndarray = type("ndarray", (), {})
    import vfi_models.atm as node_mod
    import vfi_utils

    node, ckpt = {}, E.CKPT[variant]
    with tempfile.TemporaryDirectory() as d:
        torch.save({"model_state_dict": atm_spec.seeded_state_dict(E.SEED, variant)}, os.path.join(d, ckpt))
        node_mod.load_file_from_github_release = lambda model_type, name: os.path.join(d, name)
        for name, (n, h, w, c, m, skip) in E.NODE_CASES.items():
            frames = cain_restated.seeded_frames(n, h, w, c, 9)
            states = vfi_utils.InterpolationStateList(skip, True) if skip else None
            with torch.no_grad():
                out = node_mod.ATM_VFI().vfi(ckpt, frames.clone(), 10, m, E.ENSEMBLE, optional_interpolation_states=states)[0]
            assert torch.isfinite(out).all()
            node[f"{name}_shape"] = np.array(out.shape)
            for k, v in cain_restated.summary(out, E.NODE_STRIDE).items():
                node[f"{name}_{k}"] = v
            print(variant, name, tuple(out.shape), float(out.min()), float(out.max()))
    np.savez_compressed(os.path.join(GOLDEN, E.GOLDEN_PREFIX[variant] + "_node.npz"), seed=np.array(E.SEED), **node)


def probe(variant, net_mod):
    sd = atm_spec.seeded_state_dict(E.SEED, variant)
    for h, w in ((64, 64), (64, 128), (128, 128), (128, 192)):
        for seed in range(1, 9):
            f = cain_restated.seeded_frames(2, h, w, 3, seed).permute(0, 3, 1, 2).contiguous()
            out, on, losses = run_case(net_mod, sd, f[0:1], f[1:2])
            ls = sorted(float(l) for l in losses)
            print(variant, f"{h}x{w} seed {seed}: losses", [round(float(l), 4) for l in losses], "level", E.select(losses), "gap",
                  round((ls[1] - ls[0]) / ls[1], 4), "clamped", round(float(((out <= 0) | (out >= 1)).float().mean()), 4), flush=True)


def main():
    which = set(sys.argv[1:]) or {"lite", "base"}
    lite_tool.install_timm_shim()
    ref_import.setup()
    import vfi_models.atm.network_base as net_base
    import vfi_models.atm.network_lite as net_lite

    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    for variant, net_mod in (("lite", net_lite), ("base", net_base)):
        if variant not in which:
            continue
        if "probe" in which:
            probe(variant, net_mod)
            continue
        make_net(variant, net_mod)
        make_node(variant)


if __name__ == "__main__":
    main()
