"""Write the XVFI goldens under tests/golden/ by running the REAL reference on this host (CPU), through oracle/ref_import:

  xvfi_net.npz    the reference's own XVFInet forward (is_training=False) on xvfi_restated.NET_CASES at t = 0.5 and 0.2: the output (compact:
                  cain_restated.summary), level 0's flow_l_tmp (every FLOW_STRIDE-th row / column), and the figures of xvfi_restated.NET_CONDITIONS measured on the reference alone
                  through hooks on VFInet.bwarp / z_fwarp.  The weight seed of a case is the first of SEED_ORDER at which the conditions hold
                  at both timesteps; it is recorded.
  xvfi_node.npz   the reference's own XVFI node (vfi_models/xvfi/__init__.py) on NODE_CASES and ORDER_CASES, the seed found the same way
                  (distance conditions only).  The ordering cases keep the reference's frames in the reference's own order, with their keys.

Inputs are not stored: frames are cain_restated.seeded_frames, weights cfi_amd.xvfi_spec.seeded_state_dict.
Usage: python tools/make_golden_xvfi.py [net] [node]   (default: both; needs the reference checkout; nothing under oracle/ is changed)
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pkgload import load_package  # noqa: E402

load_package()
import cain_restated  # noqa: E402
import xvfi_restated as xr  # noqa: E402
from cfi_amd.xvfi_spec import CKPT_CONFIGS, config_of, seeded_state_dict, xvfi_shapes  # noqa: E402
from oracle import ref_import  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


class Hooks:
    """Records, on the reference's own VFInet, every sampled bwarp mask before the gate and the level-0 splat's targets and norms"""

    def __init__(self, arch):
        self.arch, self.rec = arch, None
        self.real_bwarp, self.real_zf = arch.VFInet.bwarp, arch.VFInet.z_fwarp
        hooks = self

        def bwarp(self, x, flo):
            if hooks.rec is not None:
                hooks.rec.setdefault("masks", []).append(xr.bwarp_parts(x, flo)[1][:, 0])
            return hooks.real_bwarp(self, x, flo)

        def z_fwarp(self, img, flo, z):
            out = hooks.real_zf(self, img, flo, z)
            if hooks.rec is not None:
                hooks.rec.setdefault("tg", []).append(flo)
                hooks.rec.setdefault("nm", []).append(out[1][:, 0:1])
            return out

        arch.VFInet.bwarp, arch.VFInet.z_fwarp = bwarp, z_fwarp

    def start(self):
        self.rec = {}

    def figures(self):
        r = self.rec
        taps = {"targets": torch.cat(r["tg"][-2:], 1), "norms": torch.cat(r["nm"][-2:], 1), "masks": r["masks"]}
        self.rec = None
        return xr.conditions(taps, None)

    def figures_all_calls(self):
        """node runs: the worst distances over every model call"""
        r = self.rec
        self.rec = None
        tg = torch.cat([x.flatten() for x in r["tg"]]).double()
        return {"splat_dist": float((tg - torch.round(tg)).abs().min()), "mask_dist": min(float((m.double() - 0.999).abs().min()) for m in r["masks"])}


def holds(fig, gained, t=None):
    return all(fig[k] >= xr.NET_CONDITIONS[k] for k in xr.condition_keys(gained, t))


def make_net(arch, hooks):
    net = {}
    for name, (scale, S, h, w, gain) in xr.NET_CASES.items():
        args = argparse.Namespace(gpu=torch.device("cpu"), nf=64, module_scale_factor=scale, S_trn=S, S_tst=S, img_ch=3)
        model = arch.XVFInet(args).eval()
        assert list(model.state_dict().keys()) == list(xvfi_shapes(scale).keys())
        assert [tuple(v.shape) for v in model.state_dict().values()] == [tuple(s) for s in xvfi_shapes(scale).values()]
        # the reference module's own key order and shapes, for tests/test_xvfi_cpu.py
        net[f"keys_scale{scale}"] = np.array(list(model.state_dict().keys()))
        net[f"shapes_scale{scale}"] = np.array([",".join(map(str, v.shape)) for v in model.state_dict().values()])
        last = {}
        for mod in (model.vfinet.conv_flow2, model.vfinet.conv_flow_bottom):
            mod.register_forward_hook(lambda m, i, o: last.__setitem__("tmp", o))
        f = cain_restated.seeded_frames(2, h, w, 3, xr.FRAME_SEED).permute(0, 3, 1, 2).contiguous()
        x = torch.stack([f[0:1], f[1:2]], 2)      # [1,3,2,h,w]
        for seed in xr.SEED_ORDER:
            model.load_state_dict(seeded_state_dict((scale, S), seed, gain))
            outs, figs = {}, {}
            for t in xr.NET_TS:
                hooks.start()
                with torch.no_grad():
                    outs[t] = (model(x, torch.tensor([[t]]), is_training=False)[0], last["tmp"][0].permute(1, 2, 0).clone())
                figs[t] = hooks.figures()
                if not holds(figs[t], gain != 1.0, t):      # (the next timestep cannot mend it)
                    break
            ok = len(figs) == len(xr.NET_TS) and all(holds(figs[t], gain != 1.0, t) for t in xr.NET_TS)
            if ok or seed == xr.SEED_ORDER[0]:
                print(name, "seed", seed, "ok" if ok else "no", {t: {k: round(v, 6) for k, v in figs[t].items()} for t in figs}, flush=True)
            if ok:
                break
        else:
            raise RuntimeError(f"{name}: no seed of SEED_ORDER meets the conditions")
        net[f"{name}_seed"] = np.array(seed)
        for t in xr.NET_TS:
            out, tmp = outs[t]
            assert torch.isfinite(out).all()
            for k, v in cain_restated.summary(out.permute(1, 2, 0), xr.NET_STRIDE).items():
                net[f"{name}_t{t}_{k}"] = v
            for k, v in figs[t].items():
                net[f"{name}_t{t}_{k}"] = np.array(v)
        fs = xr.FLOW_STRIDE.get(name, 1)
        net[f"{name}_flow_l_tmp"] = outs[xr.NET_TS[0]][1][::fs, ::fs].numpy()
    np.savez_compressed(os.path.join(GOLDEN, "xvfi_net.npz"), **net)


def make_node(hooks):
    cupy = sys.modules.get("cupy")      # einops (vfi_utils.preprocess_frames) probes every importable array library
    if cupy is not None and not hasattr(cupy, "ndarray"):
        cupy.ndarray = type("ndarray", (), {})
    import vfi_models.xvfi as node_mod

    node = {}
    with tempfile.TemporaryDirectory() as d:
        node_mod.load_file_from_github_release = lambda model_type, ckpt: os.path.join(d, ckpt)
        for name, (ckpt, n, h, w, c, m, states) in {**xr.NODE_CASES, **xr.ORDER_CASES}.items():
            frames = cain_restated.seeded_frames(n, h, w, c, 9)
            assert not isinstance(states, tuple), "the reference raises on an InterpolationStateList"
            for seed in xr.SEED_ORDER:
                torch.save({"state_dict_Model": seeded_state_dict(ckpt, seed)}, os.path.join(d, ckpt))
                hooks.start()
                with torch.no_grad():
                    out = node_mod.XVFI().vfi(ckpt, frames.clone(), 1, m, optional_interpolation_states=states)[0]
                fig = hooks.figures_all_calls()
                ok = holds(fig, False)
                print(name, "seed", seed, "ok" if ok else "no", fig, tuple(out.shape), flush=True)
                if ok:
                    break
            else:
                raise RuntimeError(f"{name}: no seed of SEED_ORDER meets the conditions")
            assert torch.isfinite(out).all()
            node[f"{name}_seed"] = np.array(seed)
            node[f"{name}_shape"] = np.array(out.shape)
            for k, v in fig.items():
                node[f"{name}_{k}"] = np.array(v)
            if name in xr.ORDER_CASES:
                en = [i for i, s in enumerate(states if states is not None else [True] * (n - 1)) if s]
                keys = sorted([str(i) for i in range(n)] + [f"{i}.{k}" for i in en for k in range(1, m)])
                assert len(keys) == out.shape[0]
                node[f"{name}_keys"] = np.array(keys)
                node[f"{name}_frames"] = out.numpy()
            else:
                for k, v in cain_restated.summary(out, xr.NODE_STRIDE).items():
                    node[f"{name}_{k}"] = v
    np.savez_compressed(os.path.join(GOLDEN, "xvfi_node.npz"), **node)


def main():
    which = set(sys.argv[1:]) or {"net", "node"}
    ref_import.setup()
    import vfi_models.xvfi.xvfi_arch as arch

    assert set(CKPT_CONFIGS) == set(__import__("vfi_models.xvfi", fromlist=["CKPT_CONFIGS"]).CKPT_CONFIGS)
    assert config_of(xr.X) == (4, 5) and config_of(xr.V) == (2, 1)
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    hooks = Hooks(arch)
    if "net" in which:
        make_net(arch, hooks)
    if "node" in which:
        make_node(hooks)


if __name__ == "__main__":
    main()
