"""Torch CPU restatement of the reference SepConv++ forward (vfi_models/sepconv/sepconv_enhanced.py:527-700), written from the state
dict of cfi_amd.sepconv_spec: the GPU tests compare against it where the reference is not present (1080p), and
tests/test_sepconv_spec_cpu.py pins it to the reference's own outputs in tests/golden/sepconv_net.npz.  The two separable convolutions
run in float64 through ref_ops_restated.sepconv, which also returns the magnitude M that bounds any fp32 summation order."""
import torch
import torch.nn.functional as F

import ref_ops_restated as ror

K = 51
ENC = "netEncode.0.netVer.{}.netMain."
HOR = "netDecode.0.netHor.{}.netMain."      # index i = row 4 - i
VER = "netDecode.0.netVer.{}.netMain."      # index i = row 4 - i, built from row 5 - i
HEADS = ("netVerone", "netVertwo", "netHorone", "netHortwo")


def _conv(sd, name, x, stride=1):
    return F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], stride=stride, padding=1)


def _prelu(sd, name, x):
    return F.prelu(x, sd[name + ".weight"])


def _up2(x):
    return F.interpolate(x, scale_factor=2.0, mode="bilinear", align_corners=False)


def even_pad(x):
    H, W = x.shape[2:]
    return F.pad(x, [0, W % 2, 0, H % 2], mode="replicate")


def features(sd, x1, x2):
    """(the even-padded frames, the four head outputs V1, V2, H1, H2 [N,51,Hp,Wp]) for NCHW fp32 frames [N,3,H,W]"""
    one, two = even_pad(x1), even_pad(x2)
    st = torch.stack([one, two], 1).reshape(one.shape[0], -1)
    mean = st.mean(1, True).view(-1, 1, 1, 1)
    std = st.std(1, True).view(-1, 1, 1, 1)
    rows = [torch.cat([_conv(sd, "netInput", (one - mean) / (std + 1e-7)), _conv(sd, "netInput", (two - mean) / (std + 1e-7))], 1)]
    for r in range(1, 5):
        p = ENC.format(r)
        t = _conv(sd, p + "1", _prelu(sd, p + "0", rows[r - 1]), stride=2)
        rows.append(_conv(sd, p + "3", _prelu(sd, p + "2", t)))
    for r in (4, 3, 2, 1):
        p = HOR.format(4 - r)
        rows[r] = rows[r] + _conv(sd, p + "3", _prelu(sd, p + "2", _conv(sd, p + "1", _prelu(sd, p + "0", rows[r]))))
    for r in (3, 2, 1):
        p = VER.format(4 - r)
        t = _conv(sd, p + "4", _prelu(sd, p + "3", _conv(sd, p + "2", _up2(_prelu(sd, p + "0", rows[r + 1])))))
        rows[r] = rows[r] + t[:, :, :rows[r].shape[2], :rows[r].shape[3]]     # crop after both convs
    u = _up2(rows[1])
    heads = [_conv(sd, h + ".netMain.3", _prelu(sd, h + ".netMain.2", _conv(sd, h + ".netMain.1", u))) for h in HEADS]
    return one, two, heads


def pair_out(f0, f1, v1, v2, h1, h2, H, W, threshold=0.01, min_norm=False, pad="replicate"):
    """The fused output stage in float64: f0 / f1 [N,C>=3,Hp,Wp] the even-padded frames, heads [N,51,Hp,Wp] -> (out [N,3,H,W],
    M [N,3,H,W]) with M the magnitude bound of the division's inputs carried through (|a/n| error <= (eps_a + |a/n| eps_n) / |n|).
    With min_norm the smallest |n| is returned too.  pad="constant" gives the zero-padded variant (for tests that must tell the two
    apart)."""
    acc, mag = 0, 0
    for f, v, h in ((f0, v1, h1), (f1, v2, h2)):
        x = F.pad(f[:, :3].double(), [K // 2] * 4, mode=pad)
        x = torch.cat([x, torch.ones_like(x[:, :1])], 1)
        o, m = ror.sepconv(x, v, h)
        acc, mag = acc + o, mag + m
    n = acc[:, 3:4].clone()
    small = n.abs() < threshold
    n[small] = 1.0
    out = acc[:, :3] / n
    bound = (mag[:, :3] + out.abs() * mag[:, 3:4]) / n.abs()
    bound = torch.where(small.expand_as(bound), mag[:, :3], bound)
    res = out[:, :, :H, :W], bound[:, :, :H, :W]
    if min_norm:
        return res + (float(acc[:, 3, :H, :W].abs().min()),)
    return res


def gamma_pair_out():
    """two K-tap sepconvs summed, then one division: 2 * (2K + 4) + 4 roundings on the longest chain"""
    return 2 * ror.gamma_sepconv(K) + 4


def sepconv_forward(sd, x1, x2, min_norm=False):
    """model(x1, x2) for NCHW fp32 frames [N,3,H,W] -> [N,3,H,W] fp32 (float64 output stage; the inputs are not modified)"""
    H, W = x1.shape[2:]
    with torch.no_grad():
        one, two, (v1, v2, h1, h2) = features(sd, x1, x2)
        r = pair_out(one, two, v1, v2, h1, h2, H, W, min_norm=min_norm)
    out = r[0].float()
    return (out, r[2]) if min_norm else out



def node_frames(sd, frames, multiplier, skip=None):
    """The reference node's frame list (vfi_utils.generic_frame_loop, use_timestep=False) with this restatement as the model, for an int
    multiplier and an optional skip list of pair indices: frames [N,H,W,C] host -> [M,H,W,3]."""
    x = frames[..., :3].permute(0, 3, 1, 2).contiguous()

    def nti(f0, f1, n):        # non_timestep_inference, vfi_utils.py:161-170
        mid = sepconv_forward(sd, f0, f1)
        if n == 1:
            return [mid]
        first, second = nti(f0, mid, n // 2), nti(mid, f1, n // 2)
        return first + [mid] + second if n % 2 else first + second

    out = []
    for i in range(x.shape[0] - 1):
        out.append(x[i:i + 1])
        if not (skip and i in skip):
            out += nti(x[i:i + 1], x[i + 1:i + 2], multiplier - 1)
    out.append(x[-1:])
    return torch.cat(out).permute(0, 2, 3, 1)
