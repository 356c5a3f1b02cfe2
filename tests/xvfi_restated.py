"""XVFI restated in plain torch (test infrastructure only; the product runs csrc/xvfi_net.hip): a float32 restatement of the inference
forward of vfi_models/xvfi/xvfi_arch.py (XVFInet.forward with is_training=False, VFInet.forward, RefineUNet) on a state dict in the
reference's own layout, float64 restatements of the new kernels, and the cases and seeds of the goldens, so that tools/make_golden_xvfi.py
and the tests cannot drift apart.

Both the warp gate (`mask < 0.999 -> 0`) and the splat (`floor(t flow)` with Gaussian corner weights that are no partition of unity) are
discontinuous in the flow, so a golden case is only a fair gate where no splat target sits next to an integer and no sampled mask next to
0.999: the tool measures those distances on the reference alone and the CPU test asserts them (NET_CONDITIONS).
"""
import math

import torch
import torch.nn.functional as F

TOL = 1e-3                  # per pixel, un-clamped output: the project's contract
NET_STRIDE, NODE_STRIDE = 3, 3
NET_TS = (0.5, 0.2)
FRAME_SEED = 3
# name: (module_scale_factor, S_tst, H, W, flow_gain); weight seeds are searched in SEED_ORDER until NET_CONDITIONS hold and recorded in the golden
NET_CASES = {
    "v16": (2, 1, 16, 16, 30.0),
    "v48x80": (2, 1, 48, 80, 30.0),
    "x64": (4, 2, 64, 64, 30.0),
    "x512": (4, 5, 512, 512, 1.0),
}
SEED_ORDER = tuple(range(7, 4000))
FLOW_STRIDE = {"x512": 2}      # rows / columns of level 0's flow_l_tmp kept in the golden (default: all)
# conditions on the reference's own run, every case: distances of splat targets from an integer and of sampled masks from 0.999; the
# flow_gain cases besides: mean |t flow| at the level-0 splat in pixels, the two directions' share of zero-norm cells summed, the smallest
# share of gated pixels over the bwarp calls
NET_CONDITIONS = {"splat_dist": 1e-4, "mask_dist": 1e-4, "mean_tflow": 0.8, "hole_share": 0.02, "masked_share": 0.05}


def condition_keys(gained, t):
    """Which of NET_CONDITIONS a run must meet: the two distances always; the flow_gain cases also the hole and gated shares at every
    timestep and the mean |t flow| at t = 0.5, where both directions carry half of the flow (at t = 0.2 the forward direction's target is a
    fifth of the flow by construction)"""
    if not gained:
        return ["splat_dist", "mask_dist"]
    return [k for k in NET_CONDITIONS if k != "mean_tflow" or t == 0.5]


NODE_SEED = 7
# name: (ckpt, n frames, h, w, c, multipler, states); states: None, a list of booleans, or ("skip", [pairs]) for an InterpolationStateList
V, X = "XVFInet_Vimeo_exp1_latest.pt", "XVFInet_X4K1000FPS_exp1_latest.pt"
NODE_CASES = {
    "vimeo_x2": (V, 3, 16, 16, 3, 2, None),
    "vimeo_x3": (V, 5, 16, 16, 3, 3, None),
    "rgba": (V, 2, 16, 16, 4, 2, None),
    "odd": (V, 2, 10, 18, 3, 2, None),
    "bools": (V, 4, 16, 16, 3, 2, [True, False, True]),
    "x4k": (X, 2, 20, 30, 3, 2, None),
}
# ordering cases: the reference's frames are stored by key, in the reference's own (string-sorted) order, with the keys beside them
ORDER_CASES = {"order_12x3": (V, 12, 16, 16, 3, 3, None), "order_3x11": (V, 3, 16, 16, 3, 11, None)}


def conv(sd, name, x, stride=1, pad=1):
    w = sd[name + ".weight"]
    if w.dim() == 5:
        w = w[:, :, 0]
    return F.conv2d(x, w.to(x.dtype), sd[name + ".bias"].to(x.dtype), stride=stride, padding=pad)


def bwarp_parts(x, flo):
    """VFInet.bwarp (:240-268) -> (sampled image, sampled all-ones mask before the gate)"""
    B, C, H, W = x.shape
    xx = torch.arange(0, W).view(1, 1, 1, W).expand(B, 1, H, W)
    yy = torch.arange(0, H).view(1, 1, H, 1).expand(B, 1, H, W)
    vgrid = torch.cat((xx, yy), 1).to(x.dtype) + flo
    gx = 2.0 * vgrid[:, 0] / max(W - 1, 1) - 1.0
    gy = 2.0 * vgrid[:, 1] / max(H - 1, 1) - 1.0
    g = torch.stack((gx, gy), -1)
    return F.grid_sample(x, g, align_corners=True), F.grid_sample(torch.ones_like(x), g, align_corners=True)


def bwarp(x, flo, taps=None):
    out, mask = bwarp_parts(x, flo)
    if taps is not None:
        taps.setdefault("masks", []).append(mask[:, 0])
    return out * (mask >= 0.999).to(x.dtype)


def z_fwarp(img, flo, z):
    """VFInet.z_fwarp (:320-415): img [N,C,H,W] splatted to floor(flo) + {0,1}^2 (flo[:,0] moves the column, flo[:,1] the row) with weights
    (z + 1e-5) exp(-d^2); returns (splatted image, splatted weights)"""
    N, C, H, W = img.shape
    y, x = flo[:, 0:1], flo[:, 1:2]
    x1, y1 = torch.floor(x), torch.floor(y)
    rows = torch.arange(H).view(1, 1, H, 1)
    cols = torch.arange(W).view(1, 1, 1, W)
    imgw = torch.zeros(N, C, H * W, dtype=img.dtype)
    o = torch.zeros(N, 1, H * W, dtype=img.dtype)
    for a in (0, 1):
        for b in (0, 1):
            wgt = (z + 1e-5) * torch.exp(-((x - (x1 + a)) ** 2 + (y - (y1 + b)) ** 2))
            # a target that is not finite or far away lands nowhere: decided on the floats
            ok = (x1 + a + rows >= 0) & (x1 + a + rows < H) & (y1 + b + cols >= 0) & (y1 + b + cols < W)
            r = torch.where(ok, x1 + a, torch.zeros_like(x1)).long() + rows
            c = torch.where(ok, y1 + b, torch.zeros_like(y1)).long() + cols
            idx = (r * W + c).clamp(0, H * W - 1).view(N, 1, H * W)
            wv = torch.where(ok, wgt, torch.zeros_like(wgt)).view(N, 1, H * W)
            iv = torch.where(ok, img * wgt, torch.zeros_like(img)).view(N, C, H * W)
            imgw.scatter_add_(2, idx.expand(N, C, H * W), iv)
            o.scatter_add_(2, idx, wv)
    return imgw.view(N, C, H, W), o.view(N, 1, H, W)


def cfr(flow, zlog, t, taps=None):
    """(:183-198) flow [N,4,h,w] = (flow_01, flow_10), zlog [N,2,h,w], t a 0-d tensor of flow's dtype -> [N,4,h,w] = (flow_t0, flow_t1)"""
    f01, f10 = flow[:, :2], flow[:, 2:]
    z01, z10 = torch.sigmoid(zlog[:, 0:1]), torch.sigmoid(zlog[:, 1:2])
    ff, n0 = z_fwarp(f01, t * f01, z01)
    fb, n1 = z_fwarp(f10, (1 - t) * f10, z10)
    ft0 = -(1 - t) * (t * ff) + t * (t * fb)
    ft1 = (1 - t) * ((1 - t) * ff) - t * ((1 - t) * fb)
    norm = (1 - t) * n0 + t * n1
    mask = (norm > 0).to(flow.dtype)
    ft0 = (1 - mask) * ft0 + mask * (ft0 / (norm + (1 - mask)))
    ft1 = (1 - mask) * ft1 + mask * (ft1 / (norm + (1 - mask)))
    if taps is not None:
        taps["targets"] = torch.cat([t * f01, (1 - t) * f10], 1)
        taps["norms"] = torch.cat([n0, n1], 1)
    return torch.cat([ft0, ft1], 1)


def tower(sd, name, first, x):
    r = torch.relu
    x = r(conv(sd, f"{name}.{first}", x, 2))
    x = r(conv(sd, f"{name}.{first + 2}", x, 2))
    x = r(conv(sd, f"{name}.{first + 5}", F.interpolate(x, scale_factor=2, mode="nearest")))
    x = r(conv(sd, f"{name}.{first + 8}", F.interpolate(x, scale_factor=2, mode="nearest")))
    return conv(sd, f"{name}.{first + 10}", x)


def features(sd, x, scale, S):
    """x [2,3,H,W] (both frames as a batch) -> [feat level 0, ..., level S], each [2,64,h,w]"""
    n = {2: 1, 4: 2}[scale]
    m = "rec_ext_ds_module."
    f = torch.relu(conv(sd, "channel_converter.0", x))
    for _ in range(n):
        f = torch.relu(conv(sd, "rec_ext_ds", f, 2))
    f = conv(sd, f"{m}{1 + 2 * n}", f)
    rr = f"{m}{2 + 2 * n}."
    y = f + conv(sd, rr + "resblock1.conv3x3_2", torch.relu(conv(sd, rr + "resblock1.conv3x3_1", f)))
    y = y + conv(sd, rr + "resblock2.conv3x3_2", torch.relu(conv(sd, rr + "resblock2.conv3x3_1", y)))
    feats = [y + f]
    for _ in range(S):
        feats.append(conv(sd, "rec_ctx_ds", feats[-1], 2))
    return feats


def level_flows(sd, feats, S, taps=None):
    """The recursion from level S down to 0 -> (flow_l_tmp of level 0 [1,6,h,w], flow_l of level 0 [1,4,h,w])"""
    flow = tmp = None
    for l in range(S, -1, -1):
        f0, f1 = feats[l][0:1], feats[l][1:2]
        if flow is None:
            tmp = tower(sd, "vfinet.conv_flow_bottom", 0, torch.cat([f0, f1], 1))
            flow = tmp[:, :4]
        else:
            up = 2.0 * F.interpolate(flow, scale_factor=(2, 2), mode="bilinear", align_corners=False)
            w1, w0 = bwarp(f1, up[:, :2], taps), bwarp(f0, up[:, 2:], taps)
            a = conv(sd, "vfinet.conv_flow1", torch.cat([f0, w1], 1))
            b = conv(sd, "vfinet.conv_flow1", torch.cat([f1, w0], 1))
            tmp = tower(sd, "vfinet.conv_flow2", 0, torch.cat([a, b, up], 1))
            flow = tmp[:, :4] + up
    return tmp, flow


def refine_unet(sd, x):
    u, r = "vfinet.refine_unet.", torch.relu
    up = lambda v: F.interpolate(v, scale_factor=2, mode="nearest")      # noqa: E731
    e1 = r(conv(sd, u + "enc1", x, 2))
    e2 = r(conv(sd, u + "enc2", e1, 2))
    o = r(conv(sd, u + "enc3", e2, 2))
    o = up(r(conv(sd, u + "dec0", o)))
    o = up(r(conv(sd, u + "dec1", torch.cat([o, e2], 1))))
    o = up(r(conv(sd, u + "dec2", torch.cat([o, e1], 1))))
    return conv(sd, u + "dec3", o)


def xvfi_forward(sd, x0, x1, t, scale, S, taps=None):
    """x0, x1 [1,3,Hp,Wp] padded frames, t a float -> [1,3,Hp,Wp], not clamped"""
    t = torch.tensor(t, dtype=torch.float32)
    feats = features(sd, torch.cat([x0, x1], 0), scale, S)
    tmp, flow = level_flows(sd, feats, S, taps)
    if taps is not None:
        taps["flow_l_tmp"] = tmp
    f0, f1 = feats[0][0:1], feats[0][1:2]
    ft = cfr(flow, tmp[:, 4:6], t, taps)
    w0, w1 = bwarp(f0, ft[:, :2], taps), bwarp(f1, ft[:, 2:], taps)
    x = torch.relu(conv(sd, "vfinet.conv_flow3.0", torch.cat([f0, w0, w1, f1, ft], 1), 1, 0))
    fr = tower(sd, "vfinet.conv_flow3", 2, x) + ft
    w0, w1 = bwarp(f0, fr[:, :2], taps), bwarp(f1, fr[:, 2:], taps)
    big = scale * F.interpolate(fr, scale_factor=(scale, scale), mode="bilinear", align_corners=False)
    i0, i1 = bwarp(x0, big[:, :2], taps), bwarp(x1, big[:, 2:], taps)
    ro = refine_unet(sd, torch.cat([F.pixel_shuffle(torch.cat([f0, f1, w0, w1], 1), scale), x0, x1, i0, i1, big], 1))
    occ0 = torch.sigmoid(ro[:, 0:1])
    occ1 = 1 - occ0
    out = (1 - t) * occ0 * i0 + t * occ1 * i1
    return out / ((1 - t) * occ0 + t * occ1) + ro[:, 1:4]


def xvfi_frame(sd, f0, f1, t, scale, S, taps=None):
    """One model call of the node: frames [1,3,H,W] -> crop(model(zero-pad to multiples of 2^S scale 4)) [1,3,H,W]"""
    H, W = f0.shape[2:]
    d = 2 ** S * scale * 4
    ph, pw = (d - H % d) % d, (d - W % d) % d
    a, b = F.pad(f0, (0, pw, 0, ph)), F.pad(f1, (0, pw, 0, ph))
    return xvfi_forward(sd, a, b, t, scale, S, taps)[:, :, :H, :W]


def conditions(taps, t):
    """The figures of NET_CONDITIONS from a run's taps (the tool computes the same from hooks on the reference)"""
    tg = taps["targets"].double()
    return {
        "splat_dist": float((tg - torch.round(tg)).abs().min()),
        "mask_dist": min(float((m.double() - 0.999).abs().min()) for m in taps["masks"]),
        "mean_tflow": min(float(tg[:, :2].abs().mean()), float(tg[:, 2:].abs().mean())),
        "hole_share": float((taps["norms"] == 0).double().mean((0, 2, 3)).sum()),
        "masked_share": min(float((m < 0.999).double().mean()) for m in taps["masks"]),
    }


# ---- float64 restatements of the kernels (tests/test_gpu_xvfi_ops.py) --------------------------------------------------------------------

BICUBIC_TAPS = (-3.0 / 32, 19.0 / 32, 19.0 / 32, -3.0 / 32)


def bicubic_down_f64(x, l):
    """x [N,H,W,C] -> [N,H/l,W/l,C] in float64: the fixed 4-tap filter over rows / columns l i + l/2 - 2 .. l i + l/2 + 1, clamped"""
    x = x.double()
    N, H, W, C = x.shape
    k = torch.tensor(BICUBIC_TAPS, dtype=torch.float64)
    iy = (torch.arange(H // l)[:, None] * l + l // 2 - 2 + torch.arange(4)[None]).clamp(0, H - 1)
    ix = (torch.arange(W // l)[:, None] * l + l // 2 - 2 + torch.arange(4)[None]).clamp(0, W - 1)
    rows = (x[:, iy] * k.view(1, 1, 4, 1, 1)).sum(2)                  # [N,Ho,W,C]
    return (rows[:, :, ix] * k.view(1, 1, 1, 4, 1)).sum(3)


def bwarp_f64(x, flo):
    """x [N,H,W,C], flo [N,H,W,2] (fp32 tensors) -> (out [N,H,W,C] float64, the sampled mask [N,H,W] float64).  The sampling position goes
    through the reference's normalise / un-normalise in fp32 (that is the function under test); taps and sums are float64."""
    N, H, W, C = x.shape
    xx = torch.arange(W, dtype=torch.float32).view(1, 1, W) + flo[..., 0]
    yy = torch.arange(H, dtype=torch.float32).view(1, H, 1) + flo[..., 1]
    gx = 2.0 * xx / max(W - 1, 1) - 1.0
    gy = 2.0 * yy / max(H - 1, 1) - 1.0
    ix = (((gx + 1.0) / 2.0) * (W - 1)).double()
    iy = (((gy + 1.0) / 2.0) * (H - 1)).double()
    bad = ~(torch.isfinite(ix) & torch.isfinite(iy))
    ix, iy = torch.where(bad, torch.full_like(ix, -10.0), ix).clamp(-10, W + 10), torch.where(bad, torch.full_like(iy, -10.0), iy).clamp(-10, H + 10)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    out = torch.zeros(N, H, W, C, dtype=torch.float64)
    mask = torch.zeros(N, H, W, dtype=torch.float64)
    xd = x.double()
    n_idx = torch.arange(N).view(N, 1, 1).expand(N, H, W)
    for dy in (0, 1):
        for dx in (0, 1):
            wx = (ix - x0) if dx else (x0 + 1 - ix)
            wy = (iy - y0) if dy else (y0 + 1 - iy)
            cx, cy = (x0 + dx).long(), (y0 + dy).long()
            ok = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
            wgt = torch.where(ok, wx * wy, torch.zeros_like(wx))
            out += xd[n_idx, cy.clamp(0, H - 1), cx.clamp(0, W - 1)] * wgt[..., None]
            mask += wgt
    return out * (mask >= 0.999).double()[..., None], mask


def cfr_f64(flow, zlog, t):
    """flow [h,w,4], zlog [h,w,2] (fp32 tensors), t float -> [h,w,4] float64; the splat targets are the fp32 products, as in the kernel and
    in torch, everything after them is float64.  Also returns (targets [h,w,4] float64, norms [h,w,2])"""
    t32 = torch.tensor(t, dtype=torch.float32)
    f = flow.permute(2, 0, 1)[None]
    tg = torch.cat([t32 * f[:, :2], (1 - t32) * f[:, 2:]], 1)
    td, omt = float(t32), float(1 - t32)
    fd, z = f.double(), torch.sigmoid(zlog.double()).permute(2, 0, 1)[None]
    ff, n0 = z_fwarp(fd[:, :2], tg[:, :2].double(), z[:, 0:1])
    fb, n1 = z_fwarp(fd[:, 2:], tg[:, 2:].double(), z[:, 1:2])
    ft0 = -omt * (td * ff) + td * (td * fb)
    ft1 = omt * (omt * ff) - td * (omt * fb)
    norm = omt * n0 + td * n1
    pos = norm > 0
    safe = torch.where(pos, norm, torch.ones_like(norm))
    out = torch.cat([torch.where(pos, ft0 / safe, ft0), torch.where(pos, ft1 / safe, ft1)], 1)
    return out[0].permute(1, 2, 0), tg[0].permute(1, 2, 0).double(), torch.cat([n0, n1], 1)[0].permute(1, 2, 0)


def splat_count(tg):
    """tg [1,2,h,w] targets -> [h,w] float64: how many sources reach each cell"""
    _, _, H, W = tg.shape
    x1, y1 = torch.floor(tg[:, 1:2]), torch.floor(tg[:, 0:1])
    rows, cols = torch.arange(H).view(1, 1, H, 1), torch.arange(W).view(1, 1, 1, W)
    cnt = torch.zeros(H * W, dtype=torch.float64)
    for a in (0, 1):
        for b in (0, 1):
            ok = (x1 + a + rows >= 0) & (x1 + a + rows < H) & (y1 + b + cols >= 0) & (y1 + b + cols < W)
            r = torch.where(ok, x1 + a, torch.zeros_like(x1)).long() + rows
            c = torch.where(ok, y1 + b, torch.zeros_like(y1)).long() + cols
            cnt.scatter_add_(0, (r * W + c).clamp(0, H * W - 1).flatten(), ok.double().flatten())
    return cnt.view(H, W)


def cfr_abs_sums(flow, zlog, tg, t):
    """For cfr_f64's rounding bound: (A [h,w] = the absolute sum of the terms of either numerator, an upper bound for both; K [h,w] = the
    larger number of sources that reach the cell in one direction), from finite flows and cfr_f64's own targets"""
    t32 = torch.tensor(t, dtype=torch.float32)
    td, omt = float(t32), float(1 - t32)
    f = flow.double().abs().permute(2, 0, 1)[None]
    z = torch.sigmoid(zlog.double()).permute(2, 0, 1)[None]
    tgn = tg.permute(2, 0, 1)[None]
    a0 = z_fwarp(f[:, :2], tgn[:, :2], z[:, 0:1])[0].amax(1)[0]
    a1 = z_fwarp(f[:, 2:], tgn[:, 2:], z[:, 1:2])[0].amax(1)[0]
    k0, k1 = splat_count(tgn[:, :2]), splat_count(tgn[:, 2:])
    return max(td, omt) * (a0 + a1), torch.maximum(k0, k1)


def conv4x4s2_f64(x, w, b):
    """x [N,H,W,Cin], w [Cout,Cin,4,4], b [Cout] -> Conv2d(4, 2, 1) as [N,H/2,W/2,Cout] float64"""
    return F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=2, padding=1).permute(0, 2, 3, 1)


# ---- the node on a stand-in or a device engine -----------------------------------------------------------------------------------------

class RestatedXvfi:
    """XvfiEngine.forward on the CPU: the restated model, one call per new frame (test infrastructure only)."""

    def __init__(self, ckpt, seed=NODE_SEED):
        from cfi_amd import xvfi_spec

        self.config = xvfi_spec.config_of(ckpt)
        self.sd, self.device, self.calls = xvfi_spec.seeded_state_dict(ckpt, seed), torch.device("cpu"), 0

    def forward(self, frame0, frame1, t, out=None):
        self.calls += 1
        one = lambda f: f[..., :3].permute(2, 0, 1)[None].contiguous()      # noqa: E731
        with torch.no_grad():
            return xvfi_frame(self.sd, one(frame0), one(frame1), t, *self.config)[0].permute(1, 2, 0)

    def release_workspace(self):
        pass

    def workspace_bytes(self):
        return 0


def node_states(states):
    from cfi_amd.schedule import InterpolationStateList

    if isinstance(states, tuple):
        return InterpolationStateList(states[1], states[0] == "skip")
    return states


def run_node(case, monkeypatch, engine_of, batch_size=1):
    """The node's vfi() on a case of NODE_CASES / ORDER_CASES with the checkpoint lookup and the engine replaced; engine_of(ckpt) -> engine"""
    import cain_restated
    import cfi_amd
    from cfi_amd import xvfi

    ckpt, n, h, w, c, m, states = {**NODE_CASES, **ORDER_CASES}[case] if isinstance(case, str) else case
    engine = engine_of(ckpt)
    monkeypatch.setattr(xvfi, "load_file_from_github_release", lambda model_type, name: name)
    monkeypatch.setattr(xvfi, "cached_engine", lambda model_type, path, build: (engine, True))
    if engine.device.type == "cpu":
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    frames = cain_restated.seeded_frames(n, h, w, c, 9)
    return cfi_amd.XVFI().vfi(ckpt, frames, batch_size, m, node_states(states))[0]


def numeric_order(keys):
    """The reference's frame keys ('3', '3.2', '10.11': input frame, or input frame '.' middle index) -> their indices in numeric order"""
    def k(s):
        a, _, b = s.partition(".")
        return int(a), int(b) if b else 0
    return sorted(range(len(keys)), key=lambda i: k(keys[i]))


def check_node_case(case, out, golden):
    import cain_restated

    assert tuple(out.shape) == tuple(golden[case + "_shape"]) and out.dtype == torch.float32 and out.device.type == "cpu"
    d, sums_ok = cain_restated.compare(out, golden, case + "_", NODE_STRIDE, TOL)
    print(f"XVFI node {case}: max |d| vs the reference node {d:.3e}")
    assert d <= TOL and sums_ok, (case, d, sums_ok)
    return d


assert math.isclose(sum(BICUBIC_TAPS), 1.0)
