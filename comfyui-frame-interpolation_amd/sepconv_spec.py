"""Checkpoint layout of SepConv++ (sepconv.pth: a plain ``Network().state_dict()``, no wrapper and no ``module.`` prefix; the node
does ``load_state_dict(torch.load(path))``, vfi_models/sepconv/__init__.py:40-42).

Key names / shapes follow vfi_models/sepconv/sepconv_enhanced.py:527-600 (Network with intChannels [32, 64, 128, 256, 512]); order =
torch state_dict order.  Every PReLU is ``num_parameters=1``: one scalar slope, a tensor of shape (1,).  Module indices do not follow
the row order: ``netDecode.0.netHor.i`` is row 4 - i, and ``netDecode.0.netVer.i`` builds row 4 - i from row 5 - i."""
from collections import OrderedDict

CHANNELS = (32, 64, 128, 256, 512)     # rows 0..4; row 0 = netInput of both frames (16 + 16 channels)
TAPS = 51                              # per-pixel separable filter size
HEADS = ("netVerone", "netVertwo", "netHorone", "netHortwo")


def sepconv_shapes():
    d = OrderedDict()
    d["netInput.weight"] = (16, 3, 3, 3)
    d["netInput.bias"] = (16,)
    for r in range(1, 5):     # encoder Ver: prelu - sconv(3) - prelu - conv(3)
        p, ci, co = f"netEncode.0.netVer.{r}.netMain.", CHANNELS[r - 1], CHANNELS[r]
        d[p + "0.weight"] = (1,)
        d[p + "1.weight"], d[p + "1.bias"] = (co, ci, 3, 3), (co,)
        d[p + "2.weight"] = (1,)
        d[p + "3.weight"], d[p + "3.bias"] = (co, co, 3, 3), (co,)
    for i in range(4):        # decoder Hor of row 4 - i: prelu - conv - prelu - conv + skip
        p, c = f"netDecode.0.netHor.{i}.netMain.", CHANNELS[4 - i]
        d[p + "0.weight"] = (1,)
        d[p + "1.weight"], d[p + "1.bias"] = (c, c, 3, 3), (c,)
        d[p + "2.weight"] = (1,)
        d[p + "3.weight"], d[p + "3.bias"] = (c, c, 3, 3), (c,)
    for i in range(1, 4):     # decoder Ver of row 4 - i from row 5 - i: prelu - up - conv - prelu - conv
        p, ci, co = f"netDecode.0.netVer.{i}.netMain.", CHANNELS[5 - i], CHANNELS[4 - i]
        d[p + "0.weight"] = (1,)
        d[p + "2.weight"], d[p + "2.bias"] = (co, ci, 3, 3), (co,)
        d[p + "3.weight"] = (1,)
        d[p + "4.weight"], d[p + "4.bias"] = (co, co, 3, 3), (co,)
    for h in HEADS:           # up - conv - prelu - conv
        p = h + ".netMain."
        d[p + "1.weight"], d[p + "1.bias"] = (64, 64, 3, 3), (64,)
        d[p + "2.weight"] = (1,)
        d[p + "3.weight"], d[p + "3.bias"] = (TAPS, 64, 3, 3), (TAPS,)
    return d


def check_state_dict(sd):
    """Strict, as ``Network.load_state_dict(sd)``: every key, no extra key, every shape."""
    want = sepconv_shapes()
    missing = [k for k in want if k not in sd]
    unexpected = [k for k in sd if k not in want]
    if missing or unexpected:
        raise RuntimeError(f"Error(s) in loading state_dict for Network: Missing key(s): {missing}. Unexpected key(s): {unexpected}.")
    for k, shp in want.items():
        if tuple(sd[k].shape) != tuple(shp):
            raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(sd[k].shape)} vs model {tuple(shp)}")


def load_file(path):
    """<ckpts_path>/sepconv/sepconv.pth -> the checked state dict"""
    import torch

    sd = torch.load(path, map_location="cpu", weights_only=False)
    check_state_dict(sd)
    return sd


def seeded_state_dict(seed):
    """A stand-in for sepconv.pth's weights, for the tests and goldens: PyTorch's default initialisation of the convolutions
    (U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weights and biases) drawn in state-dict order from one generator; every PReLU its own
    slope (0.10, 0.11, ... in key order, so a mis-wired slope changes the result); and the four heads' last biases at 1/51 plus a
    small spread, so each 51-tap filter sums to about 1 and the normaliser stays far from the 0.01 threshold."""
    import torch

    g = torch.Generator().manual_seed(seed)
    sd, fan, k_prelu = {}, None, 0
    for k, shp in sepconv_shapes().items():
        if shp == (1,):
            sd[k] = torch.tensor([0.10 + 0.01 * k_prelu], dtype=torch.float32)
            k_prelu += 1
            continue
        if k.endswith(".weight"):
            fan = shp[1] * shp[2] * shp[3]
        bound = 1.0 / fan ** 0.5
        sd[k] = (torch.rand(shp, generator=g, dtype=torch.float32) * 2 - 1) * bound
        if k.split(".")[0] in HEADS and k.endswith("3.bias"):
            sd[k] = 1.0 / TAPS + 0.1 * sd[k]
    return sd
