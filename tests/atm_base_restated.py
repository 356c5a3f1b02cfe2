"""TEST INFRASTRUCTURE: the torch restatement of ATM-base (vfi_models/atm/network_base.py), the float32 / float64 yardstick of
tests/test_atm_base_cpu.py and tests/test_gpu_atm_base.py, and the cases of the base goldens (tools/make_golden_atm_base.py).

network_base.Network and network_lite.Network share one forward and one module tree, so the layers, the windowed attention and the node loop
are tests/atm_restated.py's own, imported and left as they are.  Restated here is what that file ties to lite's widths: the Mlp (its
depthwise convolution has ``2 C`` groups written out there; base's mlp_ratio is 4, so the group count is read off the weights) and, because
the forward calls the Mlp through the block, the block and the forward that lead to it.  Everything else follows the state dict's shapes.
"""
import torch
import torch.nn.functional as F

import atm_restated as R
from atm_restated import (ATTN_CASES, ATTN_CH_STRIDE, HEADS, MODES, NET_SHAPES, NET_STRIDE, NODE_CASES, NODE_STRIDE, SEED, TOL,  # noqa: F401
                          check_node_case, frames_of)

VARIANT = "base"
CKPT = "atm-vfi-base.pt"
LOCAL_DIM, GLOBAL_DIM = 384, 672      # the attention cases' C: 384 for window 8, 672 for window 12


def attn_golden_file(cross):
    """the block goldens are one file per kind (each under the 1 MiB a committed file may have)"""
    return "atm_base_attn.npz" if cross else "atm_base_attn_self.npz"


def config_with(atm_base):
    """a stand-in for ckpt.load_config: the package's own config with the atm_base key set"""
    from cfi_amd import ckpt

    real = ckpt.load_config

    def load_config():
        return dict(real(), atm_base=atm_base)

    return load_config


_SD = {}


def state_dict_as(dtype):
    """the seeded base checkpoint, drawn once per dtype and shared (read-only) among the tests"""
    from cfi_amd import atm_spec

    if torch.float32 not in _SD:
        _SD[torch.float32] = atm_spec.seeded_state_dict(SEED, VARIANT)
    if dtype not in _SD:
        _SD[dtype] = {k: v.to(dtype) for k, v in _SD[torch.float32].items()}
    return _SD[dtype]


def attn_case(name, cross, dtype=torch.float32):
    """atm_restated.attn_case on the seeded BASE checkpoint: (block parameters, token map [2,h,w,C]), C = 384 (window 8) / 672 (window 12)"""
    h, w, win, shift = ATTN_CASES[name]
    prefix = "local_motion_atmformer.0." if win == 8 else "global_motion_atmformer.0."
    p = {k[len(prefix):]: v for k, v in state_dict_as(dtype).items() if k.startswith(prefix)}
    if not cross:
        p["attn.qkv.weight"] = torch.cat([p.pop("attn.q.weight"), p.pop("attn.kv.weight")])
        for k in [k for k in p if k.startswith("attn.mlp.") or k == "attn.relative_coord"]:
            del p[k]
    C = p["norm1.weight"].shape[0]
    assert C == (LOCAL_DIM if win == 8 else GLOBAL_DIM)
    g = torch.Generator().manual_seed(2000 + sorted(ATTN_CASES).index(name))
    x = torch.randn((2, h, w, C), generator=g, dtype=torch.float32) * 1.5
    return p, x.to(dtype)


def mlp_block(p, x):
    """x + fc2(gelu(dwconv3x3(fc1(norm2(x))))) on [n,h,w,C]; the hidden width (mlp_ratio C) is fc1's"""
    C = x.shape[-1]
    t = F.layer_norm(x, (C,), p["norm2.weight"], p["norm2.bias"])
    t = F.linear(t, p["mlp.fc1.weight"], p["mlp.fc1.bias"])
    t = R.nhwc(F.conv2d(R.nchw(t), p["mlp.dwconv.dwconv.weight"], p["mlp.dwconv.dwconv.bias"], padding=1, groups=t.shape[-1]))
    return x + F.linear(F.gelu(t), p["mlp.fc2.weight"], p["mlp.fc2.bias"])


def window_block(p, x, win, shift, cross, zero_motion=False):
    """ATMFormer (cross) / RefineBottleneck on x [2,h,w,C] -> (x', motion [2,h,w,2] or None)"""
    y, mot, _ = R.window_attention(p, x, win, shift, cross, zero_motion)
    return mlp_block(p, y), mot


def atm_forward(sd, im0, im1, global_motion, zero_motion=False, taps=None):
    """network_base.Network.forward_normal on padded frames [1,3,H,W] (H, W multiples of 64) -> I_t [1,3,H,W], clamped: the statements of
    atm_restated.atm_forward over this file's window_block.  zero_motion / taps: as there."""
    conv, conv_prelu, deconv_prelu, warp, nhwc, nchw, sub = R.conv, R.conv_prelu, R.deconv_prelu, R.warp, R.nhwc, R.nchw, R.sub
    pyr0, pyr1 = [im0], [im1]
    for _ in range(3):
        pyr0.append(R.half(pyr0[-1])), pyr1.append(R.half(pyr1[-1]))
    x, feats = torch.cat([im0, im1]), []
    for i in range(4):
        x = conv_prelu(sd, f"feat_extracts.{i}.1", conv_prelu(sd, f"feat_extracts.{i}.0", x, 1 if i == 0 else 2))
        feats.append(x)
    tok = R.fusion(sd, "cross_scale_feature_fusion", feats[1], feats[2], feats[3])
    if global_motion:
        g = conv_prelu(sd, "last_feat_extract.1", conv_prelu(sd, "last_feat_extract.0", feats[3], 2))
        gtok, mots = R.fusion(sd, "global_feature_fusion", feats[2], feats[3], g), []
        for k in range(2):
            gtok, mot = window_block(sub(sd, f"global_motion_atmformer.{k}."), gtok, 12, 6 * k, True, zero_motion)
            mots.append(mot)
        out = R.motion_head(sd, "global_motion_mlp", gtok, mots)
        fl0, fl1 = R.up_flow(out[:, 0:2]), R.up_flow(out[:, 2:4])
        tok = torch.cat([nhwc(warp(nchw(tok[0:1]).contiguous(), fl0)), nhwc(warp(nchw(tok[1:2]).contiguous(), fl1))])
        for i in (3, 2, 1, 0):
            pyr0[i], pyr1[i] = warp(pyr0[i], fl0), warp(pyr1[i], fl1)
            if i:
                fl0, fl1 = R.up_flow(fl0), R.up_flow(fl1)
    mots = []
    for k in range(2):
        tok, mot = window_block(sub(sd, f"local_motion_atmformer.{k}."), tok, 8, 4 * k, True, zero_motion)
        mots.append(mot)
    out = R.motion_head(sd, "local_motion_mlp", tok, mots)
    for k in range(2):
        tok, _ = window_block(sub(sd, f"feat_enhance_transformer.{k}."), tok, 8, 4 * k, False)
    feat = torch.cat([warp(nchw(tok[0:1]).contiguous(), out[:, 0:2]), warp(nchw(tok[1:2]).contiguous(), out[:, 2:4]), out], 1).contiguous()
    skips = []
    for i, scale in enumerate((2, 1, 0)):
        p = f"upsample_pyramid.{i}"
        j = 0
        if i:
            feat, j = F.prelu(feat, sd[p + ".0.weight"]), 1
        feat = conv(sd, f"{p}.{j + 2}", conv_prelu(sd, f"{p}.{j + 1}", deconv_prelu(sd, f"{p}.{j}", feat)))
        if scale:
            skips.append(feat[:, :-5])
    out = feat[:, -5:]
    m = torch.sigmoid(out[:, 4:5])
    w0, w1 = warp(pyr0[0], out[:, 0:2]), warp(pyr1[0], out[:, 2:4])
    it = m * w0 + (1 - m) * w1
    if taps is not None:
        taps["flow0"], taps["flow1"] = out[:, 0:2], out[:, 2:4]
    f0 = conv_prelu(sd, "proj", torch.cat([feat, im0, w0, im1, w1, it], 1))
    f1 = conv_prelu(sd, "down1.0", f0, 2)
    f2 = conv_prelu(sd, "down2.1", conv_prelu(sd, "down2.0", torch.cat([f1, skips[1]], 1), 2))
    f3 = conv_prelu(sd, "down3.0", torch.cat([f2, skips[0]], 1), 2)
    f3 = conv_prelu(sd, "down3.2", conv_prelu(sd, "down3.1", f3))
    u2 = conv_prelu(sd, "up1.1", deconv_prelu(sd, "up1.0", f3))
    u1 = conv_prelu(sd, "up2.1", deconv_prelu(sd, "up2.0", torch.cat([u2, f2], 1)))
    u0 = deconv_prelu(sd, "up3.0", torch.cat([u1, f1], 1))
    res = conv_prelu(sd, "refine_head.1", conv_prelu(sd, "refine_head.0", torch.cat([u0, f0], 1)))
    return (it + (2 * torch.sigmoid(res) - 1)).clamp(0, 1)


def atm_frame(sd, f0, f1, global_motion, zero_motion=False, taps=None):
    """One model call of the node: frames [1,3,H,W] -> clamp(unpad(model(pad(f0), pad(f1)))) [1,3,H,W]"""
    H, W = f0.shape[2:]
    t, b, l, r = R.pad64(H, W)
    a, c = F.pad(f0, (l, r, t, b), mode="replicate"), F.pad(f1, (l, r, t, b), mode="replicate")
    return atm_forward(sd, a, c, global_motion, zero_motion, taps)[:, :, t:t + H, l:l + W].clamp(0, 1)


_F32 = {}


def restated32(shape_name, mode):
    """the float32 restatement of a golden shape and mode, [h,w,3], computed once and shared (read-only)"""
    key = (shape_name, mode)
    if key not in _F32:
        f0, f1 = frames_of(shape_name)
        with torch.no_grad():
            _F32[key] = atm_forward(state_dict_as(torch.float32), f0, f1, MODES[mode])[0].permute(1, 2, 0).contiguous()
    return _F32[key]


class RestatedAtmBase:
    """AtmEngine.forward on the CPU: the restated base model, one call per new frame (test infrastructure only)."""

    variant = VARIANT

    def __init__(self):
        self.sd, self.device, self.calls = state_dict_as(torch.float32), torch.device("cpu"), 0

    def forward(self, frame0, frame1, global_motion=True):
        self.calls += 1
        one = lambda f: f[..., :3].permute(2, 0, 1)[None].contiguous()      # noqa: E731
        with torch.no_grad():
            return atm_frame(self.sd, one(frame0), one(frame1), global_motion)[0].permute(1, 2, 0)

    def release_workspace(self):
        pass

    def workspace_bytes(self):
        return 0


def run_node(case, monkeypatch, engine, ckpt_name=CKPT):
    """The node's vfi() on a case of NODE_CASES under a base checkpoint name, with the atm_base key on and the checkpoint lookup and the
    engine replaced"""
    import cain_restated
    import cfi_amd
    from cfi_amd import atm, ckpt
    from cfi_amd.schedule import InterpolationStateList

    n, h, w, c, m, skip, gm = NODE_CASES[case]
    monkeypatch.setattr(ckpt, "load_config", config_with(True))
    monkeypatch.setattr(atm, "load_file_from_github_release", lambda model_type, name: name)
    monkeypatch.setattr(atm, "cached_engine", lambda model_type, path, build: (engine, True))
    if engine.device.type == "cpu":
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    frames = cain_restated.seeded_frames(n, h, w, c, 9)
    states = InterpolationStateList(skip, True) if skip else None
    return cfi_amd.ATM_VFI().vfi(ckpt_name, frames, 10, m, gm, states)[0]
