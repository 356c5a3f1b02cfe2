"""Plain-torch restatement of the reference AMT-G forward (vfi_models/amt/amt_arch.py:1441-1590) over the pieces of tests/amt_restated.py
(volume-free lookup, decoders, warps, multi_flow_combine), written from the state dict of cfi_amd.amt_spec.  It runs in the dtype and on
the device of the tensors it is given.  tests/test_amt_g_cpu.py pins it to the reference's own outputs (tests/golden/amt_g_net.npz,
amt_g_node.npz; tools/make_golden_amt_g.py).

AMT-G is AMT-L's forward with other tables (LargeEncoder: a fourth, stride-1 encoder stage; wider update blocks) plus two update blocks:
after ``update3_low`` / ``update2_low`` (AMT-L's update3 / update2: they run at 1/8 resolution on resized inputs), ``update3_high`` /
``update2_high`` run at 1/4 / 1/2 resolution on ft + dft, on cat(up_flow0, up_flow1) after the low block's deltas, and on the SAME lookup
output resized by 2 / 4 (:1537-1543, :1558-1564); they make no lookup of their own.

The order of the high blocks' first layer.  Here, as in the reference: resize the 392-channel lookup output, then convc1 (1x1), then
LeakyReLU.  The C object runs convc1 on the low-resolution lookup output and resizes its 256 channels (vfi_amt_upsample_lrelu): convc1 is
linear and per pixel and the bilinear weights sum to 1, so the two orders agree in exact arithmetic.  ``ops.upsample_lrelu`` (the kernel
under test), where an ops object offers it, switches this file to the commuted order, so that the kernel runs inside the forward it was
written for while the float64 evaluation of this file stays in the reference's order.  ``ops.convc1_upsample``, where offered instead, takes
the lookup output and convc1's weights and runs both steps (a 1x1 layer object, then the kernel).

Error bound of vfi_amt_upsample_lrelu (|got - want| <= gamma * 2^-24 * M, M = sum over the four taps of |weight * value|, against float64
on the same fp32 coordinates' exact values).  The source coordinate (dst + 0.5) / s - 0.5 is exact in fp32 for s = 2, 4 and dst < 2^22
(a dyadic rational with two fraction bits), so are its floor, the fraction l and 1 - l (multiples of 1/8): the weights carry no error.
Roundings on the way of one term into the result: the product with the x weight, the sum of the row's two terms, the product with the y
weight, the sum of the two rows, the product with the slope: gamma = 5, taken as 6 with one spare."""
import torch
import torch.nn.functional as F

import amt_restated
from amt_restated import (LEVELS, NET_SHAPES, NET_STRIDE, NET_TS, SEED, TOL, WIN, _conv, _conv7, _convblock, _norm_relu, combine_warps, lookup,
                          pad16, pyramid_encoder, resize, warp)

VARIANT = "G"
GAMMA_UPSAMPLE = 6
UPDATE_BLOCKS = ("update4", "update3_low", "update2_low", "update3_high", "update2_high")
# the goldens' frame seeds: amt_restated.NET_SHAPES' (400-402); the conditions on the seeded checkpoint hold with them
NODE_STRIDE = amt_restated.NODE_STRIDE
# name -> (checkpoint, frames, h, w, channels, multiplier, skip list); frames cain_restated.seeded_frames(n, h, w, c, 9)
NODE_CASES = {"g_m2": ("amt-g.pth", 3, 128, 128, 3, 2, None), "g_odd_m3": ("amt-g.pth", 2, 130, 200, 3, 3, None),
              "g_skip": ("amt-g.pth", 3, 128, 128, 3, 3, [1])}


def state_dict64():
    from cfi_amd import amt_spec

    return {k: v.double() for k, v in amt_spec.seeded_state_dict(VARIANT, SEED).items()}


def feat_encoder(sd, x, ops=None):
    """LargeEncoder (:665-741) with norm_fn='instance' over a batch of frames [N,3,H,W]: residual stages 64 / 112 (stride 2) / 160 (stride 2)
    / 160 (layer3_2, stride 1), then the 1x1 output convolution"""
    p = "feat_encoder."
    x = _norm_relu(_stem(sd, p + "conv1", x, ops, None))
    for lname, stride in (("layer1", 1), ("layer2", 2), ("layer3", 2), ("layer3_2", 1)):
        for b in range(2):
            q = f"{p}{lname}.{b}."
            s = stride if b == 0 else 1
            y = _norm_relu(_conv(sd, q + "conv1", x, s))
            y = _norm_relu(_conv(sd, q + "conv2", y))
            if s == 2:
                x = F.instance_norm(_conv(sd, q + "downsample.0", x, 2), eps=1e-5)
            x = F.relu(x + y)
    return _conv(sd, p + "conv2", x)


def _stem(sd, name, x, ops, slopes):
    """a 7x7 stride-2 layer over 3 channels [+ PReLU]: through ops.stem (vfi_conv7x7s2_prelu) where an ops object offers it"""
    if ops is not None and hasattr(ops, "stem"):
        return ops.stem(x, sd[name + ".weight"], sd[name + ".bias"], slopes)
    y = _conv(sd, name, x, 2)
    return y if slopes is None else F.prelu(y, slopes)


def pyramid_encoder_g(sd, x, ops=None):
    if ops is None or not hasattr(ops, "stem"):
        return pyramid_encoder(sd, x)
    fs = []
    for i in range(1, 5):
        n0 = f"encoder.pyramid{i}.0"
        y = _stem(sd, n0 + ".0", x, ops, sd[n0 + ".1.weight"]) if i == 1 else amt_restated._convrelu(sd, n0, x, 2)
        x = amt_restated._convrelu(sd, f"encoder.pyramid{i}.1", y)
        fs.append(x)
    return fs


def update(sd, name, net, flow, corr, scale, ops=None, corr_up=None):
    """BasicUpdateBlock.forward (:1055-1073).  scale: the low blocks' scale_factor (net is resized down, the deltas up).  corr_up: the high
    blocks' resize of the lookup output (2.0 / 4.0), applied here so that the order of resize and convc1 is this function's to choose."""
    lr = lambda v: F.leaky_relu(v, 0.1)          # noqa: E731
    if scale:
        net = resize(net, 1 / scale)
    if corr_up and ops is not None and hasattr(ops, "convc1_upsample"):     # the object's order: convc1 at low resolution, then resize + lrelu
        cor = ops.convc1_upsample(corr, sd[name + ".convc1.weight"], sd[name + ".convc1.bias"], int(corr_up), 0.1)
    elif corr_up and ops is not None and hasattr(ops, "upsample_lrelu"):
        cor = ops.upsample_lrelu(_conv(sd, name + ".convc1", corr), int(corr_up), 0.1)
    else:                                                                   # the reference's order
        cor = lr(_conv(sd, name + ".convc1", resize(corr, corr_up) if corr_up else corr))
    cor = lr(_conv(sd, name + ".convc2", cor))
    flo = lr(_conv(sd, name + ".convf2", _conv7(sd, name + ".convf1", flow, ops, act=1)))
    inp = torch.cat([lr(_conv(sd, name + ".conv", torch.cat([cor, flo], 1))), flow, net], 1)
    out = _conv(sd, name + ".gru.2", lr(_conv(sd, name + ".gru.0", inp)))
    dnet = _conv(sd, name + ".feat_head.2", lr(_conv(sd, name + ".feat_head.0", out)))
    dflow = _conv(sd, name + ".flow_head.2", lr(_conv(sd, name + ".flow_head.0", out)))
    if scale:
        dnet, dflow = resize(dnet, scale), scale * resize(dflow, scale)
    return dnet, dflow


def amt_g_forward(sd, img0, img1, ts, zero_lookup=False, zero_block=None, ops=None):
    """clamp(AMT_G(pad(img0), pad(img1), embt=t)) un-padded, for every t of ts: frames [1,3,H,W] -> [len(ts),3,H,W].  zero_lookup replaces
    the lookup's output by zeros, zero_block the two outputs of the named update block (the goldens' conditions on the seeded checkpoint).
    ops: as amt_restated.amt_forward's, plus stem (both 7x7 stride-2 layers) and convc1_upsample / upsample_lrelu (see the file's docstring)."""
    from cfi_amd.amt_spec import CONFIG

    cfg = CONFIG[VARIANT]
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
    fm = feat_encoder(sd, torch.cat([img0, img1]), ops)
    fmap0, fmap1 = fm[0], fm[1]
    p0, p1 = pyramid_encoder_g(sd, img0, ops), pyramid_encoder_g(sd, img1, ops)

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

    def upd(name, *a, **k):
        dft, dflow = update(sd, name, *a, ops=ops, **k)
        return (torch.zeros_like(dft), torch.zeros_like(dflow)) if name == zero_block else (dft, dflow)

    outs = []
    for t in ts:
        embt = torch.tensor(float(t), dtype=torch.float32).to(img0.device, img0.dtype)      # the node passes a FloatTensor
        out = _convblock(sd, "decoder4", torch.cat([p0[3], p1[3], embt.expand(1, 1, Hp // 16, Wp // 16)], 1), skip)
        fl0, fl1, ft = out[:, 0:2], out[:, 2:4], out[:, 4:]
        for dec, low, high, lvl, down in (("decoder3", "update4", None, 2, 1), ("decoder2", "update3_low", "update3_high", 1, 2),
                                          ("decoder1", "update2_low", "update2_high", 0, 4)):
            corr, flow = corr_lookup(fl0, fl1, embt, down)
            dft, dflow = upd(low, ft, flow, corr, float(down) if down != 1 else None)
            fl0, fl1, ft = fl0 + dflow[:, 0:2], fl1 + dflow[:, 2:4], ft + dft
            if high:
                dft, dflow = upd(high, ft, torch.cat([fl0, fl1], 1), corr, None, corr_up=float(down))
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
        comb = _conv7(sd, "comb_block.2", _conv7(sd, "comb_block.0", wr, ops, act=3, slopes=sd["comb_block.1.weight"]), ops)
        if ops is not None and hasattr(ops, "combine_out"):
            outs.append(ops.combine_out(wr, comb, nf, t_, l, H, W))
        else:
            pred = (wr.reshape(1, nf, 3, Hp, Wp).mean(1) + comb).clamp(0, 1)
            outs.append(pred[:, :, t_:t_ + H, l:l + W])
    return torch.cat(outs)


def upsample_lrelu(x, s, slope):
    """what vfi_amt_upsample_lrelu computes, [N,C,h,w] -> [N,C,s h,s w], and M = sum |weight * value| of each element's four taps"""
    return F.leaky_relu(resize(x, float(s)), slope), resize(x.abs(), float(s))


# ---- the node on a stand-in or a device engine ------------------------------------------------------------------------------------------

class RestatedAmtG:
    """AmtEngine.forward on the CPU: the restated model, one call per pair (test infrastructure only)."""

    def __init__(self):
        from cfi_amd import amt_spec

        self.variant, self.sd, self.device, self.calls = VARIANT, amt_spec.seeded_state_dict(VARIANT, SEED), torch.device("cpu"), []

    def forward(self, frame0, frame1, ts):
        self.calls.append(list(ts))
        nchw = lambda f: f[..., :3].permute(2, 0, 1)[None].contiguous()      # noqa: E731
        with torch.no_grad():
            return amt_g_forward(self.sd, nchw(frame0), nchw(frame1), ts).permute(0, 2, 3, 1)

    def release_workspace(self):
        pass

    def workspace_bytes(self):
        return 0


def config_with(amt_g):
    """a stand-in for ckpt.load_config: the package's own config with the amt_g key set"""
    from cfi_amd import ckpt

    real = ckpt.load_config

    def load_config():
        return dict(real(), amt_g=amt_g)

    return load_config


def run_node(case, monkeypatch, engine):
    """The node's vfi() on a case of NODE_CASES with amt_g on and the checkpoint lookup and the engine replaced"""
    import cain_restated
    import cfi_amd
    from cfi_amd import amt, ckpt
    from cfi_amd.schedule import InterpolationStateList

    name, n, h, w, c, m, skip = NODE_CASES[case]
    monkeypatch.setattr(ckpt, "load_config", config_with(True))
    monkeypatch.setattr(amt, "load_file_from_direct_url", lambda model_type, url: url.rsplit("/", 1)[-1])
    monkeypatch.setattr(amt, "cached_engine", lambda model_type, path, build: (engine, True))
    if engine.device.type == "cpu":
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    frames = cain_restated.seeded_frames(n, h, w, c, 9)
    states = InterpolationStateList(skip, True) if skip else None
    return cfi_amd.AMT_VFI().vfi(name, frames, 1, m, states)[0]


def check_node_case(case, out, golden):
    import cain_restated

    assert tuple(out.shape) == tuple(golden[case + "_shape"]) and out.dtype == torch.float32 and out.device.type == "cpu"
    d, sums_ok = cain_restated.compare(out, golden, case + "_", NODE_STRIDE, TOL)
    print(f"AMT-G node {case}: max |d| vs the reference node {d:.3e}")
    assert d <= TOL and sums_ok, (case, d, sums_ok)
    return d
