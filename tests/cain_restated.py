"""Torch CPU restatement of the reference CAIN forward (vfi_models/cain/cain_arch.py CAIN(depth=3), common.py), written from the
state dict of cfi_amd.cain_spec: the GPU tests compare against it where the reference is not present (1080p), and
tests/test_cain_spec_cpu.py pins it to the reference's own outputs in tests/golden/cain_net.npz."""
import torch
import torch.nn.functional as F

P = "encoder.interpolate."


def _conv(sd, name, x, reflect):
    if reflect:
        return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), sd[name + ".weight"], sd[name + ".bias"])
    return F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], padding=1)


def _unshuffle8(x):        # pixel_shuffle(x, 1/8), common.py:208-210
    n, c, h, w = x.shape
    return x.view(n, c, h // 8, 8, w // 8, 8).permute(0, 1, 3, 5, 2, 4).reshape(n, c * 64, h // 8, w // 8)


def _shuffle8(x):          # pixel_shuffle(x, 8), common.py:204-206
    n, c, h, w = x.shape
    return x.view(n, c // 64, 8, 8, h, w).permute(0, 1, 4, 2, 5, 3).reshape(n, c // 64, h * 8, w * 8)


def cain_forward(sd, x1, x2):
    """model(x1, x2)[0] for NCHW fp32 frames [N,3,H,W]; the inputs are not modified."""
    m1 = x1.mean(2, keepdim=True).mean(3, keepdim=True)
    m2 = x2.mean(2, keepdim=True).mean(3, keepdim=True)
    x1, x2 = x1 - m1, x2 - m2
    H, W = x1.shape[2:]
    pw = (W // 128 + 1) * 128 - W if W % 128 else 0
    ph = (H // 128 + 1) * 128 - H if H % 128 else 0
    pad = (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2)
    x1, x2 = F.pad(x1, pad, mode="reflect"), F.pad(x2, pad, mode="reflect")
    x = _conv(sd, P + "headConv", torch.cat([_unshuffle8(x1), _unshuffle8(x2)], 1), False)
    res = x
    for g in range(5):
        gin = res
        for b in range(12):
            q = f"{P}body.{g}.body.{b}.body."
            t = _conv(sd, q + "2.conv", F.leaky_relu(_conv(sd, q + "0.conv", res, True), 0.2), True)
            y = t.mean((2, 3), keepdim=True)
            y = F.relu(F.conv2d(y, sd[q + "3.conv_du.0.weight"], sd[q + "3.conv_du.0.bias"]))
            y = torch.sigmoid(F.conv2d(y, sd[q + "3.conv_du.2.weight"], sd[q + "3.conv_du.2.bias"]))
            res = t * y + res
        res = _conv(sd, f"{P}body.{g}.body.12.conv", res, True) + gin
    res = res + x
    out = _shuffle8(_conv(sd, P + "tailConv", res, False))
    out = out[:, :, pad[2]:pad[2] + H, pad[0]:pad[0] + W]
    return out + (m1 + m2) / 2


def seeded_state_dict(seed):
    """A stand-in for pretrained_cain.pth's weights: PyTorch's default initialisation of CAIN(depth=3)'s layers (kaiming-uniform,
    a = sqrt(5): U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weights and biases), drawn in state-dict order from one generator."""
    from cfi_amd.cain_spec import cain_shapes

    g = torch.Generator().manual_seed(seed)
    sd, fan = {}, None
    for k, shp in cain_shapes().items():
        if k.endswith(".weight"):
            fan = shp[1] * shp[2] * shp[3]
        bound = 1.0 / fan ** 0.5
        sd[k] = (torch.rand(shp, generator=g, dtype=torch.float32) * 2 - 1) * bound
    return sd


# ---- inputs and compact goldens ---------------------------------------------------------------------------------------------------
# The goldens under tests/golden/ keep no frames: inputs are recomputed from a seed (smooth sinusoid mixtures quantised to k / 255, so
# every host derives the same fp32 values), and outputs are kept as a strided sample of pixels (every `stride`-th row and column plus
# the last one) and as float64 sums over every row and every column of each channel.

def seeded_frames(n, h, w, c, seed):
    """[n,h,w,c] fp32 frames in [0, 1] on the k / 255 grid"""
    import numpy as np

    rng = np.random.default_rng(seed)
    y, x = np.arange(h, dtype=np.float64)[:, None], np.arange(w, dtype=np.float64)[None, :]
    out = np.empty((n, h, w, c))
    for i in range(n):
        for ch in range(c):
            a, b, q, r = rng.uniform(0.03, 0.25, 4)
            p, s = rng.uniform(0.0, 6.3, 2)
            out[i, :, :, ch] = 0.5 + 0.3 * np.sin(a * y + b * x + p) + 0.2 * np.cos(q * y - r * x + s)
    return torch.from_numpy((np.round(np.clip(out, 0.0, 1.0) * 255.0) / 255.0).astype(np.float32))


def sample_index(n, stride):
    import numpy as np

    return np.unique(np.concatenate([np.arange(0, n, stride), [n - 1]]))


def summary(img, stride):
    """img [..., H, W, 3] -> dict(sample, rows, cols): img[..., iy][:, ix] and float64 sums of every row / column per channel"""
    a = img.detach().cpu().double().numpy()
    iy, ix = sample_index(a.shape[-3], stride), sample_index(a.shape[-2], stride)
    return {"sample": a[..., iy, :, :][..., ix, :].astype("float32"), "rows": a.sum(-2), "cols": a.sum(-3)}


def compare(img, golden, prefix, stride, tol):
    """max |img - golden| over the sampled pixels, and whether every row / column sum is within tol * its pixel count"""
    got = summary(img, stride)
    d = float(abs(got["sample"].astype("float64") - golden[prefix + "sample"]).max())
    H, W = img.shape[-3], img.shape[-2]
    sums_ok = bool((abs(got["rows"] - golden[prefix + "rows"]) <= tol * W).all() and (abs(got["cols"] - golden[prefix + "cols"]) <= tol * H).all())
    return d, sums_ok


def node_frames(sd, frames, multiplier, skip=None):
    """The reference node's frame list (vfi_utils.generic_frame_loop, use_timestep=False) with this restatement as the model, for an int
    multiplier and an optional skip list of pair indices: frames [N,H,W,C] host -> [M,H,W,3]."""
    x = frames[..., :3].permute(0, 3, 1, 2).contiguous()

    def nti(f0, f1, n):        # non_timestep_inference, vfi_utils.py:161-170
        mid = cain_forward(sd, f0, f1)
        if n == 1:
            return [mid]
        first, second = nti(f0, mid, n // 2), nti(mid, f1, n // 2)
        return first + [mid] + second if n % 2 else first + second

    out = []
    with torch.no_grad():
        for i in range(x.shape[0] - 1):
            out.append(x[i:i + 1])
            if not (skip and i in skip):
                out += nti(x[i:i + 1], x[i + 1:i + 2], multiplier - 1)
        out.append(x[-1:])
    return torch.cat(out).permute(0, 2, 3, 1)
