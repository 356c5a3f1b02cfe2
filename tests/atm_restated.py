"""TEST INFRASTRUCTURE: a torch restatement of ATM-lite (vfi_models/atm/network_lite.py, attention.py) and of the reference node's loop
(vfi_models/atm/__init__.py), written from their semantics for the CPU tests and as the float32 / float64 yardstick of the GPU tests.
Generic in dtype: every tensor follows the frames'.  No timm, no einops.  Token maps are NHWC ([2, h, w, C]: frame 0, frame 1).

The windowed blocks are stated once (``window_block``) for both kinds: ``cross`` (ATMFormer: q of a frame against k, v of the other frame's
same window, plus the motion read-out) and self (RefineBottleneck).  The additive -100 mask is ``labels differ`` over ``region_labels``:
nine centre-pad regions and nine shift regions, BOTH taken at the position inside the layout the windows are cut from (the reference
builds its pad mask before the roll and applies it after, attention.py:28-62, :301-303: reproduced as it is).

The cases of the goldens (tools/make_golden_atm.py) live here, beside the restatement."""
import math

import torch
import torch.nn.functional as F

SEED = 1
TOL = 1e-3                      # the project's gate against the reference: per pixel, no pixel left out
HEADS = 8
MODES = {"On": True, "Off (fastest)": False}
NET_STRIDE = 4
NET_SHAPES = {"64x64": (64, 64, 500), "128x192": (128, 192, 501), "192x320": (192, 320, 502)}      # name -> (h, w, frame seed)
NODE_STRIDE = 4
# the node goldens' cases: name -> (frames, h, w, channels, multiplier, skip list, global_motion); frames cain_restated.seeded_frames(n, h, w, c, 9)
NODE_CASES = {"m2": (3, 64, 64, 3, 2, None, "On"), "list": (3, 64, 64, 3, [3, 2], None, "Off (fastest)"),
              "skip": (4, 64, 64, 3, 2, [1], "Off (fastest)"), "rgba": (2, 64, 64, 4, 2, None, "On"),
              "odd_on": (2, 100, 180, 3, 2, None, "On"), "odd_off": (2, 100, 180, 3, 2, None, "Off (fastest)")}
# the attention cases: name -> (h, w, window, shift) of the token map; C = 224 for window 8, 352 for window 12
ATTN_CASES = {"8x8_w8_s0": (8, 8, 8, 0), "8x8_w8_s4": (8, 8, 8, 4), "16x24_w8_s0": (16, 24, 8, 0), "16x24_w8_s4": (16, 24, 8, 4),
              "4x4_w12_s0": (4, 4, 12, 0), "8x12_w12_s0": (8, 12, 12, 0), "8x12_w12_s6": (8, 12, 12, 6), "12x20_w12_s6": (12, 20, 12, 6)}
ATTN_CH_STRIDE = 7              # the attention goldens keep every 7th channel of the block's output, and the motion whole


def attn_case(name, cross, dtype=torch.float32):
    """(block parameters, token map [2,h,w,C]) of an attention case: the parameters are the first ATM block's of the seeded checkpoint
    (local for window 8, global for window 12); the self kind takes qkv = (q | kv) of the same block."""
    from cfi_amd import atm_spec

    h, w, win, shift = ATTN_CASES[name]
    prefix = "local_motion_atmformer.0." if win == 8 else "global_motion_atmformer.0."
    sd = atm_spec.seeded_state_dict(SEED)
    p = {k[len(prefix):]: v.to(dtype) for k, v in sd.items() if k.startswith(prefix)}
    if not cross:
        p["attn.qkv.weight"] = torch.cat([p.pop("attn.q.weight"), p.pop("attn.kv.weight")])
        for k in [k for k in p if k.startswith("attn.mlp.") or k == "attn.relative_coord"]:
            del p[k]
    C = p["norm1.weight"].shape[0]
    g = torch.Generator().manual_seed(1000 + sorted(ATTN_CASES).index(name))
    x = torch.randn((2, h, w, C), generator=g, dtype=torch.float32) * 1.5
    return p, x.to(dtype)


def frames_of(shape_name):
    """the two frames of a forward golden, [1,3,h,w] each"""
    import cain_restated

    h, w, fseed = NET_SHAPES[shape_name]
    f = cain_restated.seeded_frames(2, h, w, 3, fseed).permute(0, 3, 1, 2).contiguous()
    return f[0:1], f[1:2]


def state_dict_as(dtype):
    from cfi_amd import atm_spec

    return {k: v.to(dtype) for k, v in atm_spec.seeded_state_dict(SEED).items()}


# ---- layers ------------------------------------------------------------------------------------------------------------------------

def conv_prelu(sd, name, x, stride=1):
    return F.prelu(F.conv2d(x, sd[name + ".0.weight"], sd[name + ".0.bias"], stride=stride, padding=1), sd[name + ".1.weight"])


def deconv_prelu(sd, name, x):
    return F.prelu(F.conv_transpose2d(x, sd[name + ".0.weight"], sd[name + ".0.bias"], stride=2), sd[name + ".1.weight"])


def conv(sd, name, x, stride=1, dilation=1):
    w = sd[name + ".weight"]
    return F.conv2d(x, w, sd[name + ".bias"], stride=stride, padding=dilation * (w.shape[-1] // 2), dilation=dilation)


def nhwc(x):
    return x.permute(0, 2, 3, 1)


def nchw(x):
    return x.permute(0, 3, 1, 2)


def half(x):
    return F.interpolate(x, scale_factor=0.5, mode="bilinear", align_corners=True)


def up_flow(f):
    return F.interpolate(f, scale_factor=2, mode="bilinear", align_corners=True) * 2


def warp(x, flow):
    """sample x [B,C,H,W] at pixel + flow [B,2,H,W] (x, y): bilinear, zeros outside, align_corners=True"""
    B, _, H, W = x.shape
    gy, gx = torch.meshgrid(torch.arange(H, dtype=x.dtype), torch.arange(W, dtype=x.dtype), indexing="ij")
    sx, sy = 2 * (gx + flow[:, 0]) / (W - 1) - 1, 2 * (gy + flow[:, 1]) / (H - 1) - 1
    return F.grid_sample(x, torch.stack([sx, sy], dim=-1), mode="bilinear", padding_mode="zeros", align_corners=True)


def fusion(sd, name, fine, mid, coarse):
    """CrossScaleFeatureFusion: plain strided / dilated convolutions (no activation), concat, 1x1, LayerNorm -> tokens [n,h,w,C]"""
    ys = [conv(sd, name + ".layers.0", mid, 2), conv(sd, name + ".layers.1", fine, 4), conv(sd, name + ".layers.2", fine, 4, 2), coarse]
    t = nhwc(conv(sd, name + ".proj", torch.cat(ys, 1)))
    return F.layer_norm(t, t.shape[-1:], sd[name + ".norm.weight"], sd[name + ".norm.bias"])


def region_labels(hp, wp, h, w, win, shift):
    """[hp, wp] region label of every position of the layout the windows are cut from: the pad regions (when hp x wp is larger than h x w)
    and the shift regions (when shift > 0) combined; two tokens of a window see each other when their labels are equal"""
    r, c = torch.arange(hp)[:, None], torch.arange(wp)[None, :]
    lab = torch.zeros((hp, wp), dtype=torch.long)
    if (hp, wp) != (h, w):
        top, left = (hp - h) // 2, (wp - w) // 2
        lab = lab + 3 * ((r >= top).long() + (r >= h + top).long()) + (c >= left).long() + (c >= w + left).long()
    if shift:
        lab = lab * 9 + 3 * ((r >= hp - win).long() + (r >= hp - shift).long()) + (c >= wp - win).long() + (c >= wp - shift).long()
    return lab


def mlp_block(p, x):
    """x + fc2(gelu(dwconv3x3(fc1(norm2(x))))) on [n,h,w,C]"""
    C = x.shape[-1]
    t = F.layer_norm(x, (C,), p["norm2.weight"], p["norm2.bias"])
    t = F.linear(t, p["mlp.fc1.weight"], p["mlp.fc1.bias"])
    t = nhwc(F.conv2d(nchw(t), p["mlp.dwconv.dwconv.weight"], p["mlp.dwconv.dwconv.bias"], padding=1, groups=2 * C))
    return x + F.linear(F.gelu(t), p["mlp.fc2.weight"], p["mlp.fc2.bias"])


def window_attention(p, x, win, shift, cross, zero_motion=False):
    """The attention half of a block on x [2,h,w,C]: -> (norm1(x) + proj(attention), motion [2,h,w,2] or None, per-head offsets [2,h,w,8,2]
    or None).  Pad tokens are zeros BEFORE norm1; rows of padding are dropped on the way out."""
    n, h, w, C = x.shape
    hp, wp = math.ceil(h / win) * win, math.ceil(w / win) * win
    top, left = (hp - h) // 2, (wp - w) // 2
    N, d = win * win, C // HEADS

    def cut(t):          # [n,hp,wp,c] -> [n, windows, N, c]
        return t.reshape(t.shape[0], hp // win, win, wp // win, win, -1).permute(0, 1, 3, 2, 4, 5).reshape(t.shape[0], -1, N, t.shape[-1])

    def paste(t):        # the inverse, then the roll back and the crop
        t = t.reshape(n, hp // win, wp // win, win, win, -1).permute(0, 1, 3, 2, 4, 5).reshape(n, hp, wp, -1)
        return torch.roll(t, (shift, shift), (1, 2))[:, top:top + h, left:left + w]

    xp = torch.roll(F.pad(x, (0, 0, left, wp - w - left, top, hp - h - top)), (-shift, -shift), (1, 2))
    t = F.layer_norm(cut(xp), (C,), p["norm1.weight"], p["norm1.bias"])
    lab = cut(region_labels(hp, wp, h, w, win, shift)[None, :, :, None])[0, :, :, 0]
    mask = (lab[:, :, None] != lab[:, None, :]).to(x.dtype) * -100.0

    def heads(z):
        return z.reshape(n, -1, N, HEADS, d).transpose(2, 3)

    if cross:
        kv = F.linear(t.flip(0), p["attn.kv.weight"])
        q, k, v = heads(F.linear(t, p["attn.q.weight"])), heads(kv[..., :C]), heads(kv[..., C:])
    else:
        qkv = F.linear(t, p["attn.qkv.weight"])
        q, k, v = heads(qkv[..., :C]), heads(qkv[..., C:2 * C]), heads(qkv[..., 2 * C:])
    a = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5 + mask[None, :, None], dim=-1)
    o = (a @ v).transpose(2, 3).reshape(n, -1, N, C)
    out = paste(t + F.linear(o, p["attn.proj.weight"], p["attn.proj.bias"]))
    if not cross:
        return out, None, None
    i = torch.arange(N)
    kx, ky = (i % win).to(x.dtype), (i // win).to(x.dtype)
    rel = torch.stack([kx[None, :] - kx[:, None], ky[None, :] - ky[:, None]])          # [2, query, key]
    off = (a[:, :, :, None] * rel).sum(-1)                                             # [n, windows, heads, 2, N]
    rows = off.flatten(0, 1).permute(2, 0, 3, 1).reshape(-1, N, HEADS)                 # (coordinate, frame and window) x N x heads
    mot = F.linear(F.gelu(F.linear(rows, p["attn.mlp.0.weight"], p["attn.mlp.0.bias"])), p["attn.mlp.2.weight"], p["attn.mlp.2.bias"])
    mot = mot.reshape(2, n, -1, N).permute(1, 2, 3, 0)                                 # [n, windows, N, 2]
    off = off.permute(0, 1, 4, 3, 2)                                                   # [n, windows, N, 2, heads]
    if zero_motion:
        mot = torch.zeros_like(mot)
    return out, paste(mot), paste(off.transpose(-1, -2).reshape(n, -1, N, 2 * HEADS)).reshape(n, h, w, HEADS, 2)


def window_block(p, x, win, shift, cross, zero_motion=False):
    """ATMFormer (cross) / RefineBottleneck on x [2,h,w,C] -> (x', motion [2,h,w,2] or None)"""
    y, mot, _ = window_attention(p, x, win, shift, cross, zero_motion)
    return mlp_block(p, y), mot


def sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def motion_head(sd, name, tok, mots):
    """channels (block 0: frame 0 x y, frame 1 x y | block 1: ... | frame 0 tokens | frame 1 tokens) -> the 5 motion channels [1,5,h,w]"""
    m = torch.cat([torch.cat([mo[0:1], mo[1:2]], -1) for mo in mots], -1)
    x = nchw(torch.cat([m, tok[0:1], tok[1:2]], -1)).contiguous()      # (NCHW in memory, as the reference's: torch's CPU convolutions pick their kernel by layout)
    return conv(sd, name + ".2", conv_prelu(sd, name + ".1", conv_prelu(sd, name + ".0", x)))


def atm_forward(sd, im0, im1, global_motion, zero_motion=False, taps=None):
    """network_lite.Network.forward_normal on padded frames [1,3,H,W] (H, W multiples of 64) -> I_t [1,3,H,W], clamped.  zero_motion: the ATM
    blocks' motion read-out replaced by zeros (the liveliness condition of the seeded weights).  taps (a dict): the final flows."""
    pyr0, pyr1 = [im0], [im1]
    for _ in range(3):
        pyr0.append(half(pyr0[-1])), pyr1.append(half(pyr1[-1]))
    x, feats = torch.cat([im0, im1]), []
    for i in range(4):
        x = conv_prelu(sd, f"feat_extracts.{i}.1", conv_prelu(sd, f"feat_extracts.{i}.0", x, 1 if i == 0 else 2))
        feats.append(x)
    tok = fusion(sd, "cross_scale_feature_fusion", feats[1], feats[2], feats[3])
    if global_motion:
        g = conv_prelu(sd, "last_feat_extract.1", conv_prelu(sd, "last_feat_extract.0", feats[3], 2))
        gtok, mots = fusion(sd, "global_feature_fusion", feats[2], feats[3], g), []
        for k in range(2):
            gtok, mot = window_block(sub(sd, f"global_motion_atmformer.{k}."), gtok, 12, 6 * k, True, zero_motion)
            mots.append(mot)
        out = motion_head(sd, "global_motion_mlp", gtok, mots)
        fl0, fl1 = up_flow(out[:, 0:2]), up_flow(out[:, 2:4])
        tok = torch.cat([nhwc(warp(nchw(tok[0:1]).contiguous(), fl0)), nhwc(warp(nchw(tok[1:2]).contiguous(), fl1))])
        for i in (3, 2, 1, 0):
            pyr0[i], pyr1[i] = warp(pyr0[i], fl0), warp(pyr1[i], fl1)
            if i:
                fl0, fl1 = up_flow(fl0), up_flow(fl1)
    mots = []
    for k in range(2):
        tok, mot = window_block(sub(sd, f"local_motion_atmformer.{k}."), tok, 8, 4 * k, True, zero_motion)
        mots.append(mot)
    out = motion_head(sd, "local_motion_mlp", tok, mots)
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
    # residual refinement
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


def pad64(H, W):
    """InputPadder(dims, 64): (top, bottom, left, right), centred"""
    ph, pw = (((H // 64) + 1) * 64 - H) % 64, (((W // 64) + 1) * 64 - W) % 64
    return ph // 2, ph - ph // 2, pw // 2, pw - pw // 2


def atm_frame(sd, f0, f1, global_motion, zero_motion=False, taps=None):
    """One model call of the node: frames [1,3,H,W] -> clamp(unpad(model(pad(f0), pad(f1)))) [1,3,H,W]"""
    H, W = f0.shape[2:]
    t, b, l, r = pad64(H, W)
    a, c = F.pad(f0, (l, r, t, b), mode="replicate"), F.pad(f1, (l, r, t, b), mode="replicate")
    return atm_forward(sd, a, c, global_motion, zero_motion, taps)[:, :, t:t + H, l:l + W].clamp(0, 1)


# ---- the node on a stand-in or a device engine (tests/test_atm_node_cpu.py, tests/test_gpu_atm.py) ----------------------------------

class RestatedAtm:
    """AtmEngine.forward on the CPU: the restated model, one call per new frame (test infrastructure only)."""

    def __init__(self):
        from cfi_amd import atm_spec

        self.sd, self.device, self.calls = atm_spec.seeded_state_dict(SEED), torch.device("cpu"), 0

    def forward(self, frame0, frame1, global_motion=True):
        self.calls += 1
        one = lambda f: f[..., :3].permute(2, 0, 1)[None].contiguous()      # noqa: E731
        with torch.no_grad():
            return atm_frame(self.sd, one(frame0), one(frame1), global_motion)[0].permute(1, 2, 0)

    def release_workspace(self):
        pass

    def workspace_bytes(self):
        return 0


def run_node(case, monkeypatch, engine):
    """The node's vfi() on a case of NODE_CASES with the checkpoint lookup and the engine replaced"""
    import cain_restated
    import cfi_amd
    from cfi_amd import atm
    from cfi_amd.schedule import InterpolationStateList

    n, h, w, c, m, skip, gm = NODE_CASES[case]
    monkeypatch.setattr(atm, "load_file_from_github_release", lambda model_type, ckpt: ckpt)
    monkeypatch.setattr(atm, "cached_engine", lambda model_type, path, build: (engine, True))
    if engine.device.type == "cpu":
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    frames = cain_restated.seeded_frames(n, h, w, c, 9)
    states = InterpolationStateList(skip, True) if skip else None
    return cfi_amd.ATM_VFI().vfi("atm-vfi-lite.pt", frames, 10, m, gm, states)[0]


def check_node_case(case, out, golden):
    """-> max |d| over the sampled pixels; asserts the shape, the gate (1e-3 per pixel) and the row / column sums"""
    import cain_restated

    assert tuple(out.shape) == tuple(golden[case + "_shape"]) and out.dtype == torch.float32 and out.device.type == "cpu"
    d, sums_ok = cain_restated.compare(out, golden, case + "_", NODE_STRIDE, TOL)
    print(f"ATM node {case}: max |d| vs the reference node {d:.3e}")
    assert d <= TOL and sums_ok, (case, d, sums_ok)
    return d
