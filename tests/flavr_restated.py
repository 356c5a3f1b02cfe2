"""Torch CPU restatement of the reference FLAVR forward (vfi_models/flavr/flavr_arch.py UNet_3D_3D("unet_18", n_inputs=4,
joinType="concat", upmode="transpose", batchnorm=False), resnet_3D.py) together with the node's InputPadder(16), written from the state
dict of cfi_amd.flavr_spec: the GPU tests compare every pixel against it where the reference is not present, and
tests/test_flavr_spec_cpu.py pins it to the reference's own outputs in tests/golden/flavr_net.npz."""
import torch
import torch.nn.functional as F


def pad16(h, w):
    """InputPadder(dims, 16)._pad (flavr_arch.py:200-206): (left, right, top, bottom)"""
    ph, pw = (((h // 16) + 1) * 16 - h) % 16, (((w // 16) + 1) * 16 - w) % 16
    return (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2)


def _gate(sd, name, x):
    y = x.mean((2, 3, 4), keepdim=True)
    return x * torch.sigmoid(F.conv3d(y, sd[name + ".attn_layer.0.weight"], sd[name + ".attn_layer.0.bias"]))


def _block(sd, p, x, stride):
    out = F.relu(F.conv3d(x, sd[p + "conv1.0.weight"], sd.get(p + "conv1.0.bias"), stride=(1, stride, stride), padding=1))
    out = F.conv3d(out, sd[p + "conv2.0.weight"], sd.get(p + "conv2.0.bias"), padding=1)
    out = _gate(sd, p + "fg", out)
    if p + "downsample.0.weight" in sd:
        x = F.conv3d(x, sd[p + "downsample.0.weight"], None, stride=(1, stride, stride))
    return F.relu(out + x)


def flavr_forward(sd, frames):
    """model([pad(f) for f in frames])[0], un-padded: frames = four NCHW fp32 tensors [N,3,H,W] -> [N,3,H,W]; inputs are not modified."""
    H, W = frames[0].shape[2:]
    pad = pad16(H, W)
    x = torch.stack([F.pad(f, pad, mode="replicate") for f in frames], dim=2)      # [N,3,4,Hp,Wp]
    mean = x.mean((2, 3, 4), keepdim=True)
    x = x - mean
    lr = lambda t: F.leaky_relu(t, 0.2)
    x0 = F.relu(F.conv3d(x, sd["encoder.stem.0.weight"], sd.get("encoder.stem.0.bias"), stride=(1, 2, 2), padding=(1, 3, 3)))
    feats, t = [x0], x0
    for i, stride in enumerate((1, 2, 2, 1)):
        for b in range(2):
            t = _block(sd, f"encoder.layer{i + 1}.{b}.", t, stride if b == 0 else 1)
        feats.append(t)
    x0, x1, x2, x3, x4 = feats

    def conv_3d(i, t):
        return _gate(sd, f"decoder.{i}.conv.1", F.conv3d(t, sd[f"decoder.{i}.conv.0.weight"], sd[f"decoder.{i}.conv.0.bias"], padding=1))

    def up(i, t):
        t = F.conv_transpose3d(t, sd[f"decoder.{i}.upconv.0.weight"], sd[f"decoder.{i}.upconv.0.bias"], stride=(1, 2, 2), padding=1)
        return _gate(sd, f"decoder.{i}.upconv.1", t)

    d3 = torch.cat([lr(conv_3d(0, x4)), x3], 1)
    d2 = torch.cat([lr(up(1, d3)), x2], 1)
    d1 = torch.cat([lr(up(2, d2)), x1], 1)
    d0 = torch.cat([lr(conv_3d(3, d1)), x0], 1)
    dout = lr(up(4, d0))
    dout = torch.cat(torch.unbind(dout, 2), 1)
    out = lr(F.conv2d(dout, sd["feature_fuse.conv.0.weight"]))
    out = F.conv2d(F.pad(out, (3, 3, 3, 3), mode="reflect"), sd["outconv.1.weight"][:3], sd["outconv.1.bias"][:3])
    out = out + mean.squeeze(2)
    Hp, Wp = out.shape[2:]
    return out[:, :, pad[2]:Hp - pad[3], pad[0]:Wp - pad[1]]


def window_plan(n_frames, duplicate_first_last, skip=None):
    """The reference node's output assembly (vfi_models/flavr/__init__.py:72-97) as a list of ("src", frame index) / ("new", window
    index): window i (frames i..i+3) is skipped only when frames i and i + 1 are both in the skip list; a skipped first / last window
    also drops the leading / trailing source frames that only that window emits."""
    skip = set(skip or ())
    plan = []
    for i in range(n_frames - 3):
        if i in skip and i + 1 in skip:
            continue
        if i == 0:
            plan += [("src", 0)] + ([("src", 0)] if duplicate_first_last else []) + [("src", 1)]
        plan += [("new", i), ("src", i + 2)]
        if i == n_frames - 4:
            plan += [("src", i + 3)] + ([("src", i + 3)] if duplicate_first_last else [])
    return plan


def node_frames(sd, frames, duplicate_first_last=False, skip=None):
    """The reference node's frame list with this restatement as the model: frames [N,H,W,C] host -> [M,H,W,3]"""
    x = frames[..., :3].permute(0, 3, 1, 2).contiguous()
    out = []
    with torch.no_grad():
        for kind, i in window_plan(x.shape[0], duplicate_first_last, skip):
            out.append(x[i:i + 1] if kind == "src" else flavr_forward(sd, [x[i + j:i + j + 1] for j in range(4)]))
    return torch.cat(out).permute(0, 2, 3, 1)
