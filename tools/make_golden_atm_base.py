"""Write the ATM-base goldens under tests/golden/ by running the REAL reference on this host (CPU), through oracle/ref_import and the timm
shim of tools/make_golden_atm.py:

  atm_base_attn.npz   the reference's own ATMFormer (vfi_models/atm/attention.py, mlp_ratio at the class default 4, as network_base builds
                      it) on the cases of atm_base_restated.ATTN_CASES at C = 384 (window 8) / 672 (window 12): every 7th channel of the
                      block's output and the whole motion read-out
  atm_base_attn_self.npz   the same for RefineBottleneck (the self kind), in a file of its own: at base's widths the two kinds together
                      are 1.4 MB of incompressible floats, over the 1 MiB a committed file may have
  atm_base_net.npz    the reference's own network_base.Network forward at 64x64, 128x192 and 192x320, global motion on and off, with the
                      liveliness record of the seeded weights per shape and mode (motion_effect_mean, max_flow, clamped_frac: as in
                      atm_net.npz), and the state dict's names, shapes and parameter count (sd_names, sd_shapes, n_parameters)
  atm_base_node.npz   the reference's own ATM_VFI node on atm_base_restated.NODE_CASES under atm-vfi-base.pt

One model per shape, for the mask-caching reason tools/make_golden_atm.py documents.  Inputs are not stored (cain_restated.seeded_frames);
outputs are stored compactly (cain_restated.summary).  Weights: atm_spec.seeded_state_dict(SEED, "base").
Usage: python tools/make_golden_atm_base.py [attn] [net] [node]   (default: all three; needs the reference checkout; nothing under oracle/ is changed)
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_atm as lite_tool  # noqa: E402  (puts the repository and tests/ on sys.path and loads the package)
import atm_base_restated as B  # noqa: E402
import cain_restated  # noqa: E402
from cfi_amd import atm_spec  # noqa: E402
from oracle import ref_import  # noqa: E402

SEED = B.SEED
GOLDEN = lite_tool.GOLDEN


def make_attn(att):
    out = {True: {}, False: {}}
    for name, (h, w, win, shift) in B.ATTN_CASES.items():
        for cross in (True, False):
            p, x = B.attn_case(name, cross)
            C = x.shape[-1]
            cls = att.ATMFormer if cross else att.RefineBottleneck
            blk = cls(dim=C, window_size=win, shift_size=shift, patch_size=1, num_heads=8)
            blk.load_state_dict(p)
            blk.eval()
            with torch.no_grad():
                y = blk(x, h, w, 1) if cross else blk(x)
            kind = "cross" if cross else "self"
            y, mot = y if cross else (y, None)
            out[cross][f"{name}_{kind}_x"] = y.reshape(2, h, w, C)[..., ::B.ATTN_CH_STRIDE].numpy()
            if cross:
                out[cross][f"{name}_{kind}_motion"] = mot.reshape(2, h, w, 2).numpy()
            print(name, kind, C, float(y.abs().max()), None if mot is None else float(mot.abs().max()))
    for cross in (True, False):
        np.savez_compressed(os.path.join(GOLDEN, B.attn_golden_file(cross)), **out[cross])


def make_net(att, net_mod):
    net = {}
    model = net_mod.Network()
    sd = atm_spec.seeded_state_dict(SEED, "base")
    ref_sd = model.state_dict()
    assert list(ref_sd.keys()) == list(atm_spec.atm_shapes("base").keys())
    net["sd_names"] = np.array(list(ref_sd.keys()))
    net["sd_shapes"] = np.array([",".join(map(str, v.shape)) for v in ref_sd.values()])
    net["n_parameters"] = np.array(sum(p.numel() for p in model.parameters()))
    real = att.AttentionToMotion.forward

    def blind(self, *a, **k):
        x, motion = real(self, *a, **k)
        return x, torch.zeros_like(motion)

    for sname in B.NET_SHAPES:
        f0, f1 = B.frames_of(sname)
        model = net_mod.Network()      # a model per shape: a shifted block keeps its first mask (tools/make_golden_atm.py)
        model.load_state_dict(sd)
        model.eval()
        for mode, gm in B.MODES.items():
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
            for k, v in cain_restated.summary(out[0].permute(1, 2, 0), B.NET_STRIDE).items():
                net[f"{key}_{k}"] = v
            net[f"{key}_motion_effect_mean"] = np.array(float((out - dark).abs().mean()))
            net[f"{key}_max_flow"] = np.array(float(max(res["opt_flow_0"].abs().max(), res["opt_flow_1"].abs().max())))
            net[f"{key}_clamped_frac"] = np.array(float(((out <= 0) | (out >= 1)).float().mean()))
            print(key, tuple(out.shape), "motion effect", float(net[f"{key}_motion_effect_mean"]), "max flow", float(net[f"{key}_max_flow"]),
                  "clamped", float(net[f"{key}_clamped_frac"]))
    np.savez_compressed(os.path.join(GOLDEN, "atm_base_net.npz"), seed=np.array(SEED), **net)


def make_node():
    """the reference's own ATM_VFI on the seeded base checkpoint in the real file's {"model_state_dict": ...} form"""
    cupy = sys.modules.get("cupy")      # einops (vfi_utils.preprocess_frames) probes every importable array library
    if cupy is not None and not hasattr(cupy, "ndarray"):
        cupy.ndarray = type("ndarray", (), {})
    import vfi_models.atm as node_mod
    import vfi_utils

    node = {}
    with tempfile.TemporaryDirectory() as d:
        torch.save({"model_state_dict": atm_spec.seeded_state_dict(SEED, "base")}, os.path.join(d, B.CKPT))
        node_mod.load_file_from_github_release = lambda model_type, ckpt: os.path.join(d, ckpt)
        for name, (n, h, w, c, m, skip, gm) in B.NODE_CASES.items():
            frames = cain_restated.seeded_frames(n, h, w, c, 9)
            states = vfi_utils.InterpolationStateList(skip, True) if skip else None
            with torch.no_grad():
                out = node_mod.ATM_VFI().vfi(B.CKPT, frames.clone(), 10, m, gm, optional_interpolation_states=states)[0]
            assert torch.isfinite(out).all()
            node[f"{name}_shape"] = np.array(out.shape)
            for k, v in cain_restated.summary(out, B.NODE_STRIDE).items():
                node[f"{name}_{k}"] = v
            print(name, tuple(out.shape), float(out.min()), float(out.max()))
    np.savez_compressed(os.path.join(GOLDEN, "atm_base_node.npz"), seed=np.array(SEED), **node)


def main():
    which = set(sys.argv[1:]) or {"attn", "net", "node"}
    lite_tool.install_timm_shim()
    ref_import.setup()
    import vfi_models.atm.attention as att
    import vfi_models.atm.network_base as net_mod

    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    if "attn" in which:
        make_attn(att)
    if "net" in which:
        make_net(att, net_mod)
    if "node" in which:
        make_node()


if __name__ == "__main__":
    main()
