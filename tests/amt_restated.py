"""Plain-torch restatement of the reference AMT-S / AMT-L forward (vfi_models/amt/amt_arch.py:1205-1285, :1349-1429) in the VOLUME-FREE
form, written from the state dict of cfi_amd.amt_spec.  It runs in the dtype and on the device of the tensors it is given, so the GPU
tests use it in float64 on the device; tests/test_amt_restated_cpu.py pins it to the reference's own outputs (tests/golden/amt_lookup.npz,
amt_net.npz; tools/make_golden_amt.py).

The lookup.  The reference builds corr[q][p] = <f0[q], f1[p]> / sqrt(D) for all pairs, average-pools it three times over p and samples
each level bilinearly (zero padding) at c(q) / 2^i + delta for the 49 deltas of a 7x7 window (:1076-1141).  Correlation is linear in the
target features, so avgpool(corr[q]) = <f0[q], avgpool(f1)>: here the FEATURES are pooled (floor sizes, as avg_pool2d), and per query
and level the 8x8 integer neighbourhood G of dot products around floor(c / 2^i) gives all 49 taps, which share one pair of fractions:

    out[lvl * 49 + a * 7 + b] = bilinear(G, x = cx + (a - 3), y = cy + (b - 3))

The FIRST window index moves x: the reference stacks delta as (dy, dx) and adds it to (x, y) coordinates (:1112-1120).

Error bound (tests/ref_ops_restated.py style, |got - want| <= gamma * 2^-24 * M, M = sum |term| of the element).  A term is
weight * fq[d] * ft_pooled[d] / sqrt(D) for one corner and one channel.  Roundings on the way of one term into the result: at most 3
per pooling level (three adds of the 2x2 mean, the division by 4 is exact) = 9 at level 3; one product and at most D - 1 additions of the
dot, in any order; the scale by 1 / sqrt(D) (one rounding of the constant, one of the product); two roundings for the corner weight
((1 - fy) and its product with fx or (1 - fx)) and one for weight * G; three additions of the four corners.  gamma_lookup(D) = D + 9 + 2
+ 3 + 3 + 2 spare = D + 19.  The fractions f = c - floor(c) are exact for c >= 0 but not for negative c (-0.3 + 1 has fewer bits than
-0.3): each may be off by U / 2 absolutely, however small the weight it forms, so each of the four weights is off by at most U (1 + U)
and the result by at most 2 U C, C = the four corners' sum |term| without their weights.  lookup_tolerance() = gamma U M + 2 U C holds
for a kernel that takes floor and fraction of c / 2^i directly.  The reference instead rounds c / 2^i + delta and takes the coordinate
through grid_sample's normalise / un-normalise round trip: its sampling position is off by up to coord_slack(...) pixels, which moves a
tap by at most that times the sum of the four corners' magnitudes; tests against the reference's fp32 output add this term."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
LEVELS, RADIUS = 4, 3
WIN = 2 * RADIUS + 1            # 7
NB = WIN + 1                    # 8: integer neighbourhood side


def gamma_lookup(D):
    return D + 19


def lookup_tolerance(D, M, Cn):
    return gamma_lookup(D) * U * M + 2 * U * Cn


def coord_slack(coord_abs, size):
    """Pixels by which the reference's fp32 sampling position may differ from the exact c / 2^i + delta: the rounding of the sum
    (|c| + 3) U, then 2 x / (size - 1) - 1 and ((g + 1) / 2) (size - 1) with five roundings of values up to max(|c| + 3, size)."""
    return 8 * U * (coord_abs + RADIUS + size)


def pool_pyramid(f):
    """[N,D,h,w] -> LEVELS maps, each avg_pool2d(2, 2) of the one before (odd sizes floored)"""
    out = [f]
    for _ in range(LEVELS - 1):
        out.append(F.avg_pool2d(out[-1], 2, stride=2))
    return out


def lookup(fq, ft, coords, bound=False):
    """One direction of BidirCorrBlock.__call__ without the volume.  fq, ft [D,h,w] query / target features, coords [2,h,w] = (x, y)
    in level-0 pixels of the target.  Returns out [196,h,w]; with bound=True also M (sum |term|), C (sum of the four corners' sum |term|,
    for the coordinate slack) and mn (the smallest non-zero |weight * one channel's product| of the element)."""
    D, h, w = fq.shape
    Q = h * w
    q = fq.reshape(D, Q)
    aq = q.abs()
    inv = 1.0 / math.sqrt(D)
    outs, Ms, Cs, mns = [], [], [], []
    for lvl, t in enumerate(pool_pyramid(ft[None])):
        t = t[0]
        hl, wl = t.shape[1:]
        tf = t.reshape(D, hl * wl)
        cx, cy = coords[0].reshape(Q) / 2 ** lvl, coords[1].reshape(Q) / 2 ** lvl
        x0, y0 = torch.floor(cx), torch.floor(cy)
        fx, fy = cx - x0, cy - y0
        x0, y0 = x0.clamp(-16, wl + 16).long(), y0.clamp(-16, hl + 16).long()
        G = q.new_zeros(NB, NB, Q)          # [gy][gx]
        A = q.new_zeros(NB, NB, Q)
        mt = q.new_full((NB, NB, Q), float("inf"))
        for gy in range(NB):
            for gx in range(NB):
                px, py = x0 - RADIUS + gx, y0 - RADIUS + gy
                ok = (px >= 0) & (px < wl) & (py >= 0) & (py < hl)
                v = tf[:, py.clamp(0, hl - 1) * wl + px.clamp(0, wl - 1)]        # [D,Q]
                G[gy, gx] = (q * v).sum(0) * inv * ok
                if bound:
                    prod = aq * v.abs() * inv
                    A[gy, gx] = prod.sum(0) * ok
                    mt[gy, gx] = torch.where(ok, prod.min(0).values, mt[gy, gx])
        w00, w01, w10, w11 = (1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx
        for a in range(WIN):                # x offset a - 3
            for b in range(WIN):            # y offset b - 3
                outs.append(w00 * G[b, a] + w01 * G[b, a + 1] + w10 * G[b + 1, a] + w11 * G[b + 1, a + 1])
                if bound:
                    Ms.append(w00 * A[b, a] + w01 * A[b, a + 1] + w10 * A[b + 1, a] + w11 * A[b + 1, a + 1])
                    Cs.append(A[b, a] + A[b, a + 1] + A[b + 1, a] + A[b + 1, a + 1])
                    m = torch.full_like(fx, float("inf"))
                    for wt, g in ((w00, mt[b, a]), (w01, mt[b, a + 1]), (w10, mt[b + 1, a]), (w11, mt[b + 1, a + 1])):
                        m = torch.where((wt > 0) & torch.isfinite(g), torch.minimum(m, wt * g), m)
                    mns.append(m)
    shape = (LEVELS * WIN * WIN, h, w)
    out = torch.stack(outs).reshape(shape)
    if not bound:
        return out
    return out, torch.stack(Ms).reshape(shape), torch.stack(Cs).reshape(shape), torch.stack(mns).reshape(shape)


# name -> (h, w, D, seed) of the lookup goldens: the minimum 16x16 map (2x2 coarsest level) and one whose pooled sizes are odd (18x26 ->
# 9x13 -> 4x6 -> 2x3)
LOOKUP_CASES = {"s_16x16": (16, 16, 84, 11), "l_18x26": (18, 26, 128, 12)}
LOOKUP_STRIDE = 2               # the goldens keep every second query row / column plus the last (cain_restated.sample_index)


def lookup_case(name):
    """fmap0, fmap1 [D,h,w] and the two coordinate maps [2,h,w] (fp32) of a golden lookup case, from its seed.  Coordinates are the grid
    plus a flow of about 6 pixels, so windows leave the map on every side; every fourth query sits exactly on an integer position, every
    seventh far outside the map (all taps zero)."""
    h, w, D, seed = LOOKUP_CASES[name]
    g = torch.Generator().manual_seed(seed)
    f0, f1 = torch.randn(D, h, w, generator=g), torch.randn(D, h, w, generator=g)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xs, ys])
    cs = []
    for _ in range(2):
        c = grid + torch.randn(2, h, w, generator=g) * 6.0
        k = torch.arange(h * w).reshape(h, w)
        c = torch.where((k % 4 == 0)[None], torch.round(c), c)
        c = torch.where((k % 7 == 3)[None], c + 40.0 * (1 - 2 * (k % 2))[None], c)
        cs.append(c)
    return f0, f1, cs[0], cs[1]


# ---- the forward goldens' cases (tools/make_golden_amt.py), shared by the CPU and GPU tests -----------------------------------------

SEED = 1
TOL = 1e-3                      # the project's gate against the reference: per-pixel, no pixel left out
NET_STRIDE = 4
NET_SHAPES = {"128x128": (128, 128, 400), "144x208": (144, 208, 401), "130x200": (130, 200, 402)}      # name -> (h, w, frame seed)
NET_TS = (0.5, 0.2)


NODE_STRIDE = 4
# the node goldens' cases: name -> (checkpoint, frames, h, w, channels, multiplier, skip list); frames cain_restated.seeded_frames(n, h, w, c, 9)
NODE_CASES = {"m2": ("amt-s.pth", 3, 128, 128, 3, 2, None), "m3": ("amt-s.pth", 2, 128, 128, 3, 3, None),
              "list": ("gopro_amt-s.pth", 3, 128, 128, 3, [3, 0], None), "skip": ("amt-s.pth", 3, 128, 128, 3, 3, [1]),
              "rgba": ("amt-l.pth", 2, 128, 128, 4, 2, None), "odd": ("amt-s.pth", 2, 130, 200, 3, 2, None)}


def frames_of(shape_name):
    """the two frames of a forward golden, [1,3,h,w] each"""
    import cain_restated

    h, w, fseed = NET_SHAPES[shape_name]
    f = cain_restated.seeded_frames(2, h, w, 3, fseed).permute(0, 3, 1, 2).contiguous()
    return f[0:1], f[1:2]


def state_dict64(variant):
    from cfi_amd import amt_spec

    return {k: v.double() for k, v in amt_spec.seeded_state_dict(variant, SEED).items()}


def pack7x7(w):
    """[Cout,Cin,7,7] -> vfi_conv7x7's [7][7][Cin4][CoutP] zero-padded pack (include/vfi_hip.h)"""
    cout, cin = w.shape[:2]
    cin4, co = (cin + 3) // 4 * 4, 4 if cout <= 4 else 16
    coutp = (cout + co - 1) // co * co
    wp = torch.zeros(7, 7, cin4, coutp, dtype=torch.float32)
    wp[:, :, :cin, :cout] = w.permute(2, 3, 1, 0)
    return wp.contiguous()


# ---- layers ------------------------------------------------------------------------------------------------------------------------

def _conv(sd, name, x, stride=1):
    w = sd[name + ".weight"]
    return F.conv2d(x, w, sd[name + ".bias"], stride=stride, padding=w.shape[-1] // 2)


def _convrelu(sd, name, x, stride=1):
    return F.prelu(_conv(sd, name + ".0", x, stride), sd[name + ".1.weight"])


def _norm_relu(x):
    return F.relu(F.instance_norm(x, eps=1e-5))          # InstanceNorm2d(affine=False): per sample and channel, biased variance


def feat_encoder(sd, variant, x):
    """SmallEncoder (bottleneck blocks) / BasicEncoder (residual blocks) with norm_fn='instance' over a batch of frames [N,3,H,W]"""
    p = "feat_encoder."
    x = _norm_relu(_conv(sd, p + "conv1", x, 2))
    for i in range(3):
        for b in range(2):
            q = f"{p}layer{i + 1}.{b}."
            s = 2 if (b == 0 and i > 0) else 1
            if variant == "S":
                y = _norm_relu(_conv(sd, q + "conv1", x))
                y = _norm_relu(_conv(sd, q + "conv2", y, s))
                y = _norm_relu(_conv(sd, q + "conv3", y))
            else:
                y = _norm_relu(_conv(sd, q + "conv1", x, s))
                y = _norm_relu(_conv(sd, q + "conv2", y))
            if s == 2:
                x = F.instance_norm(_conv(sd, q + "downsample.0", x, 2), eps=1e-5)
            x = F.relu(x + y)
    return _conv(sd, p + "conv2", x)


def pyramid_encoder(sd, x):
    fs = []
    for i in range(1, 5):
        x = _convrelu(sd, f"encoder.pyramid{i}.1", _convrelu(sd, f"encoder.pyramid{i}.0", x, 2))
        fs.append(x)
    return fs


def _resblock(sd, p, x, side):
    out = _convrelu(sd, p + "conv1", x)
    out = torch.cat([out[:, :-side], _convrelu(sd, p + "conv2", out[:, -side:])], 1)
    out = _convrelu(sd, p + "conv3", out)
    out = torch.cat([out[:, :-side], _convrelu(sd, p + "conv4", out[:, -side:])], 1)
    return F.prelu(x + _conv(sd, p + "conv5", out), sd[p + "prelu.weight"])


def _convblock(sd, name, x, side):
    p = name + ".convblock."
    x = _resblock(sd, p + "1.", _convrelu(sd, p + "0", x), side)
    return F.conv_transpose2d(x, sd[p + "2.weight"], sd[p + "2.bias"], stride=2, padding=1)


def resize(x, s):
    return F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=False)


def warp(img, flow):
    """border-padded, align_corners=True backward warp by a pixel flow (amt_arch.py:26-34)"""
    H, W = flow.shape[2:]
    xx = torch.linspace(-1.0, 1.0, W, dtype=img.dtype, device=img.device).view(1, 1, 1, W).expand(flow.shape[0], -1, H, -1)
    yy = torch.linspace(-1.0, 1.0, H, dtype=img.dtype, device=img.device).view(1, 1, H, 1).expand(flow.shape[0], -1, -1, W)
    grid = torch.cat([xx + flow[:, 0:1] / ((W - 1.0) / 2.0), yy + flow[:, 1:2] / ((H - 1.0) / 2.0)], 1).permute(0, 2, 3, 1)
    return F.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True)


def _conv7(sd, name, x, ops, act=0, slopes=None):
    """a 7x7 layer: through ops.conv7x7 (the kernel under test) where an ops object offers it, else torch"""
    if ops is not None and hasattr(ops, "conv7x7"):
        return ops.conv7x7(x, sd[name + ".weight"], sd[name + ".bias"], act, slopes)
    y = _conv(sd, name, x)
    return F.leaky_relu(y, 0.1) if act == 1 else (F.prelu(y, slopes) if act == 3 else y)


def _update(sd, name, variant, net, flow, corr, scale, ops=None):
    lr = lambda v: F.leaky_relu(v, 0.1)          # noqa: E731
    if scale:
        net = resize(net, 1 / scale)
    cor = lr(_conv(sd, name + ".convc1", corr))
    if variant == "L":
        cor = lr(_conv(sd, name + ".convc2", cor))
    flo = lr(_conv(sd, name + ".convf2", _conv7(sd, name + ".convf1", flow, ops, act=1)))
    inp = torch.cat([lr(_conv(sd, name + ".conv", torch.cat([cor, flo], 1))), flow, net], 1)
    out = _conv(sd, name + ".gru.2", lr(_conv(sd, name + ".gru.0", inp)))
    dnet = _conv(sd, name + ".feat_head.2", lr(_conv(sd, name + ".feat_head.0", out)))
    dflow = _conv(sd, name + ".flow_head.2", lr(_conv(sd, name + ".flow_head.0", out)))
    if scale:
        dnet, dflow = resize(dnet, scale), scale * resize(dflow, scale)
    return dnet, dflow


def pad16(H, W):
    """InputPadder(dims, 16)._pad (amt_arch.py:194-200): (left, right, top, bottom)"""
    ph, pw = (((H // 16) + 1) * 16 - H) % 16, (((W // 16) + 1) * 16 - W) % 16
    return pw // 2, pw - pw // 2, ph // 2, ph - ph // 2


def combine_warps(img0, img1, flow0, flow1, mask_logits, img_res, mean):
    """multi_flow_combine up to the input of comb_block (:883-900): [1, 3 n, h, w]"""
    n = flow0.shape[1] // 2
    h, w = flow0.shape[2:]
    f0, f1 = flow0.reshape(n, 2, h, w), flow1.reshape(n, 2, h, w)
    m = torch.sigmoid(mask_logits).reshape(n, 1, h, w)
    wr = m * warp(img0.expand(n, -1, -1, -1), f0) + (1 - m) * warp(img1.expand(n, -1, -1, -1), f1) + mean + img_res.reshape(n, 3, h, w)
    return wr.reshape(1, 3 * n, h, w)


def amt_forward(sd, variant, img0, img1, ts, zero_lookup=False, ops=None):
    """clamp(model(pad(img0), pad(img1), embt=t)) un-padded, for every t of ts: frames [1,3,H,W] -> [len(ts),3,H,W].  Everything that
    does not depend on t is computed once.  zero_lookup replaces the lookup's output by zeros (the goldens' corr_effect_mean).
    ops (tests/test_gpu_amt.py): an object whose methods lookup / conv7x7 / combine_warps / combine_out, where present, take the place of
    this file's torch code, so that a kernel is checked inside the forward it was written for."""
    from cfi_amd.amt_spec import CONFIG

    cfg = CONFIG[variant]
    skip, nf = cfg["skip"], cfg["num_flows"]
    H, W = img0.shape[2:]
    l, r, t_, b = pad16(H, W)
    img0, img1 = F.pad(img0, (l, r, t_, b), mode="replicate"), F.pad(img1, (l, r, t_, b), mode="replicate")
    Hp, Wp = img0.shape[2:]
    if min(Hp, Wp) < 128:
        raise ValueError(f"AMT needs padded sides of at least 128 pixels (the reference is all-NaN below): {Hp}x{Wp}")
    mean = torch.cat([img0, img1], 2).mean((1, 2, 3), keepdim=True)
    img0, img1 = img0 - mean, img1 - mean
    h8, w8 = Hp // 8, Wp // 8
    ys, xs = torch.meshgrid(torch.arange(h8, dtype=img0.dtype, device=img0.device), torch.arange(w8, dtype=img0.dtype, device=img0.device),
                            indexing="ij")
    coord = torch.stack([xs, ys])[None]
    fm = feat_encoder(sd, variant, torch.cat([img0, img1]))
    fmap0, fmap1 = fm[0], fm[1]
    p0, p1 = pyramid_encoder(sd, img0), pyramid_encoder(sd, img1)

    def corr_lookup(flow0, flow1, embt, down):
        if down != 1:
            flow0, flow1 = resize(flow0, 1 / down) / down, resize(flow1, 1 / down) / down
        s1, s0 = 1.0 / embt, 1.0 / (1.0 - embt)
        if zero_lookup:
            corr = flow0.new_zeros(1, 2 * LEVELS * WIN * WIN, h8, w8)
        elif ops is not None and hasattr(ops, "lookup"):
            corr = torch.cat([ops.lookup(fmap0, fmap1, flow1[0], float(s1)), ops.lookup(fmap1, fmap0, flow0[0], float(s0))])[None]
        else:
            corr = torch.cat([lookup(fmap0, fmap1, (coord + flow1 * s1)[0]), lookup(fmap1, fmap0, (coord + flow0 * s0)[0])])[None]
        return corr, torch.cat([flow0, flow1], 1)

    outs = []
    for t in ts:
        embt = torch.tensor(float(t), dtype=torch.float32).to(img0.device, img0.dtype)      # the node passes a FloatTensor
        out = _convblock(sd, "decoder4", torch.cat([p0[3], p1[3], embt.expand(1, 1, Hp // 16, Wp // 16)], 1), skip)
        fl0, fl1, ft = out[:, 0:2], out[:, 2:4], out[:, 4:]
        for dec, upd, lvl, down, scale in (("decoder3", "update4", 2, 1, None), ("decoder2", "update3", 1, 2, 2.0),
                                           ("decoder1", "update2", 0, 4, 4.0)):
            corr, flow = corr_lookup(fl0, fl1, embt, down)
            dft, dflow = _update(sd, upd, variant, ft, flow, corr, scale, ops)
            fl0, fl1, ft = fl0 + dflow[:, 0:2], fl1 + dflow[:, 2:4], ft + dft
            out = _convblock(sd, dec, torch.cat([ft, warp(p0[lvl], fl0), warp(p1[lvl], fl1), fl0, fl1], 1), skip)
            up0, up1 = 2.0 * resize(fl0, 2.0), 2.0 * resize(fl1, 2.0)
            if dec != "decoder1":
                fl0, fl1, ft = out[:, 0:2] + up0, out[:, 2:4] + up1, out[:, 4:]
        d0, d1, mask, res = torch.split(out, [2 * nf, 2 * nf, nf, 3 * nf], 1)
        d0, d1 = d0 + up0.repeat(1, nf, 1, 1), d1 + up1.repeat(1, nf, 1, 1)
        if ops is not None and hasattr(ops, "combine_warps"):
            wr = ops.combine_warps(img0, img1, torch.cat([d0, d1, mask, res], 1), mean, nf)
        else:
            wr = combine_warps(img0, img1, d0, d1, mask, res, mean)
        if cfg["comb_k"] == 7:
            comb = _conv7(sd, "comb_block.2", _conv7(sd, "comb_block.0", wr, ops, act=3, slopes=sd["comb_block.1.weight"]), ops)
        else:
            comb = _conv(sd, "comb_block.2", F.prelu(_conv(sd, "comb_block.0", wr), sd["comb_block.1.weight"]))
        if ops is not None and hasattr(ops, "combine_out"):
            outs.append(ops.combine_out(wr, comb, nf, t_, l, H, W))
        else:
            pred = (wr.reshape(1, nf, 3, Hp, Wp).mean(1) + comb).clamp(0, 1)
            outs.append(pred[:, :, t_:t_ + H, l:l + W])
    return torch.cat(outs)


# ---- the node on a stand-in or a device engine (tests/test_amt_node_cpu.py, tests/test_gpu_amt.py) ---------------------------------

class RestatedAmt:
    """AmtEngine.forward on the CPU: the restated model, one call per pair (test infrastructure only)."""

    def __init__(self, variant):
        from cfi_amd import amt_spec

        self.variant, self.sd, self.device, self.calls = variant, amt_spec.seeded_state_dict(variant, SEED), torch.device("cpu"), []

    def forward(self, frame0, frame1, ts):
        self.calls.append(list(ts))
        nchw = lambda f: f[..., :3].permute(2, 0, 1)[None].contiguous()      # noqa: E731
        with torch.no_grad():
            return amt_forward(self.sd, self.variant, nchw(frame0), nchw(frame1), ts).permute(0, 2, 3, 1)

    def release_workspace(self):
        pass

    def workspace_bytes(self):
        return 0


def run_node(case, monkeypatch, engine_of):
    """The node's vfi() on a case of NODE_CASES with the checkpoint lookup and the engine replaced: engine_of(variant) -> engine"""
    import cain_restated
    import cfi_amd
    from cfi_amd import amt, amt_spec
    from cfi_amd.schedule import InterpolationStateList

    ckpt, n, h, w, c, m, skip = NODE_CASES[case]
    monkeypatch.setattr(amt, "load_file_from_direct_url", lambda model_type, url: url.rsplit("/", 1)[-1])
    monkeypatch.setattr(amt, "cached_engine", lambda model_type, path, build: (engine_of(amt_spec.variant_of_ckpt(path)), True))
    if engine_of(amt_spec.variant_of_ckpt(ckpt)).device.type == "cpu":
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    frames = cain_restated.seeded_frames(n, h, w, c, 9)
    states = InterpolationStateList(skip, True) if skip else None
    return cfi_amd.AMT_VFI().vfi(ckpt, frames, 1, m, states)[0]


def check_node_case(case, out, golden):
    """-> max |d| over the sampled pixels; asserts the shape, the gate (1e-3 per pixel) and the row / column sums"""
    import cain_restated

    assert tuple(out.shape) == tuple(golden[case + "_shape"]) and out.dtype == torch.float32 and out.device.type == "cpu"
    d, sums_ok = cain_restated.compare(out, golden, case + "_", NODE_STRIDE, TOL)
    print(f"AMT node {case}: max |d| vs the reference node {d:.3e}")
    assert d <= TOL and sums_ok, (case, d, sums_ok)
    return d
