"""Write the ATM goldens under tests/golden/ by running the REAL reference on this host (CPU), through oracle/ref_import:

  atm_attn.npz   the reference's own ATMFormer / RefineBottleneck (vfi_models/atm/attention.py) on the cases of atm_restated.ATTN_CASES, both
                 kinds: every 7th channel of the block's output and, for the ATM blocks, the whole motion read-out
  atm_net.npz    the reference's own network_lite.Network forward at 64x64 (the minimum), 128x192 and 192x320 (a 12x20 global map), global
                 motion on and off; per shape and mode also the liveliness record of the seeded weights: motion_effect_mean = mean |frame -
                 frame with the ATM blocks' motion read-out zeroed|, max_flow = the largest final flow component, clamped_frac = share of
                 output values at 0 or 1; and the state dict's names and shapes
  atm_node.npz   the reference's own ATM_VFI node (vfi_models/atm/__init__.py) on atm_restated.NODE_CASES

The reference imports ``timm.models.layers`` (DropPath, to_2tuple, trunc_normal_), which is not installed: the tool puts a shim of those
three names into sys.modules first (DropPath -> nn.Identity: drop_path is 0 everywhere; trunc_normal_ -> torch's).  Inputs are not stored:
frames are cain_restated.seeded_frames.  Outputs are stored compactly (cain_restated.summary).  Weights: atm_spec.seeded_state_dict(SEED).
Usage: python tools/make_golden_atm.py [attn] [net] [node]   (default: all three; needs the reference checkout; nothing under oracle/ is changed)
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pkgload import load_package  # noqa: E402

load_package()
import atm_restated  # noqa: E402
import cain_restated  # noqa: E402
from cfi_amd import atm_spec  # noqa: E402
from oracle import golden_stats, ref_import  # noqa: E402

SEED = atm_restated.SEED
GOLDEN = os.path.join(ROOT, "tests", "golden")


def install_timm_shim():
    timm, models, layers = types.ModuleType("timm"), types.ModuleType("timm.models"), types.ModuleType("timm.models.layers")
    layers.DropPath = lambda *a, **k: torch.nn.Identity()
    layers.to_2tuple = lambda x: tuple(x) if isinstance(x, (tuple, list)) else (x, x)
    layers.trunc_normal_ = torch.nn.init.trunc_normal_
    timm.models, models.layers = models, layers
    sys.modules.update({"timm": timm, "timm.models": models, "timm.models.layers": layers})


def make_attn(att):
    out = {}
    for name, (h, w, win, shift) in atm_restated.ATTN_CASES.items():
        for cross in (True, False):
            p, x = atm_restated.attn_case(name, cross)
            C = x.shape[-1]
            cls = att.ATMFormer if cross else att.RefineBottleneck
            blk = cls(dim=C, window_size=win, shift_size=shift, patch_size=1, num_heads=8, mlp_ratio=2)
            blk.load_state_dict(p)
            blk.eval()
            with torch.no_grad():
                y = blk(x, h, w, 1) if cross else blk(x)
            kind = "cross" if cross else "self"
            y, mot = y if cross else (y, None)
            out[f"{name}_{kind}_x"] = y.reshape(2, h, w, C)[..., ::atm_restated.ATTN_CH_STRIDE].numpy()
            if cross:
                out[f"{name}_{kind}_motion"] = mot.reshape(2, h, w, 2).numpy()
            print(name, kind, float(y.abs().max()), None if mot is None else float(mot.abs().max()))
    np.savez_compressed(os.path.join(GOLDEN, "atm_attn.npz"), **out)


def make_net(att, net_mod):
    net = {}
    model = net_mod.Network()
    sd = atm_spec.seeded_state_dict(SEED)
    ref_sd = model.state_dict()
    assert list(ref_sd.keys()) == list(atm_spec.atm_shapes().keys())
    net["sd_names"] = np.array(list(ref_sd.keys()))
    net["sd_shapes"] = np.array([",".join(map(str, v.shape)) for v in ref_sd.values()])
    net["n_parameters"] = np.array(sum(p.numel() for p in model.parameters()))
    real = att.AttentionToMotion.forward

    def blind(self, *a, **k):
        x, motion = real(self, *a, **k)
        return x, torch.zeros_like(motion)

    for sname in atm_restated.NET_SHAPES:
        f0, f1 = atm_restated.frames_of(sname)
        # a model per shape, as the node builds one per call: a shifted block keeps its first mask for every later input with the same
        # padded H * W (attention.py:279-305), and the 4x4 and 8x12 global maps both pad to 12x12
        model = net_mod.Network()
        model.load_state_dict(sd)
        model.eval()
        for mode, gm in atm_restated.MODES.items():
            model.global_motion, model.ensemble_global_motion = gm, False
            key = f"{sname}_{'on' if gm else 'off'}"
            with torch.no_grad():
                res = model(f0, f1)
                att.AttentionToMotion.forward = blind
                try:
                    dark = model(f0, f1)["I_t"]
                finally:
                    att.AttentionToMotion.forward = real
            out = res["I_t"]
            assert torch.isfinite(out).all()
            for k, v in cain_restated.summary(out[0].permute(1, 2, 0), atm_restated.NET_STRIDE).items():
                net[f"{key}_{k}"] = v
            net[f"{key}_motion_effect_mean"] = np.array(float((out - dark).abs().mean()))
            net[f"{key}_max_flow"] = np.array(float(max(res["opt_flow_0"].abs().max(), res["opt_flow_1"].abs().max())))
            net[f"{key}_clamped_frac"] = np.array(float(((out <= 0) | (out >= 1)).float().mean()))
            print(key, tuple(out.shape), "motion effect", float(net[f"{key}_motion_effect_mean"]), "max flow", float(net[f"{key}_max_flow"]),
                  "clamped", float(net[f"{key}_clamped_frac"]))
    np.savez_compressed(os.path.join(GOLDEN, "atm_net.npz"), seed=np.array(SEED), **net)


def make_node():
    """the reference's own ATM_VFI on the seeded checkpoint in the real file's {"model_state_dict": ...} form"""
    cupy = sys.modules.get("cupy")      # einops (vfi_utils.preprocess_frames) probes every importable array library
    if cupy is not None and not hasattr(cupy, "ndarray"):
        cupy.ndarray = type("ndarray", (), {})
    import vfi_models.atm as node_mod
    import vfi_utils

    node = {}
    with tempfile.TemporaryDirectory() as d:
        torch.save({"model_state_dict": atm_spec.seeded_state_dict(SEED)}, os.path.join(d, atm_spec.LITE))
        node_mod.load_file_from_github_release = lambda model_type, ckpt: os.path.join(d, ckpt)
        for name, (n, h, w, c, m, skip, gm) in atm_restated.NODE_CASES.items():
            frames = cain_restated.seeded_frames(n, h, w, c, 9)
            states = vfi_utils.InterpolationStateList(skip, True) if skip else None
            with torch.no_grad():
                out = node_mod.ATM_VFI().vfi(atm_spec.LITE, frames.clone(), 10, m, gm, optional_interpolation_states=states)[0]
            assert torch.isfinite(out).all()
            node[f"{name}_shape"] = np.array(out.shape)
            for k, v in cain_restated.summary(out, atm_restated.NODE_STRIDE).items():
                node[f"{name}_{k}"] = v
            print(name, tuple(out.shape), float(out.min()), float(out.max()))
    np.savez_compressed(os.path.join(GOLDEN, "atm_node.npz"), seed=np.array(SEED), **node)


def main():
    which = set(sys.argv[1:]) or {"attn", "net", "node"}
    install_timm_shim()
    ref_import.setup()
    import vfi_models.atm.attention as att
    import vfi_models.atm.network_lite as net_mod

    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    if "attn" in which:
        make_attn(att)
    if "net" in which:
        make_net(att, net_mod)
    if "node" in which:
        make_node()
    golden_stats.write_host_signature(os.path.join(GOLDEN, "atm_host.json"))


if __name__ == "__main__":
    main()
