"""Checkpoint layout of CAIN (pretrained_cain.pth: ``{"state_dict": {"module.<key>": tensor}}`` of ``CAIN(depth=3)``,
vfi_models/cain/__init__.py:41-47).

Key names / shapes follow vfi_models/cain/cain_arch.py and common.py (Encoder -> Interpolation(5, 12, 192): headConv, 5
ResidualGroups of 12 RCABs + one ConvNorm, tailConv); order = torch state_dict order."""
from collections import OrderedDict

FEAT = 192      # 3 * 4^3 channels of a pixel_shuffle(1/8)-ed frame
RED = 12        # CALayer(192, reduction=16)
GROUPS, BLOCKS = 5, 12


def cain_shapes():
    d = OrderedDict()
    p = "encoder.interpolate."
    d[p + "headConv.weight"] = (FEAT, 2 * FEAT, 3, 3)
    d[p + "headConv.bias"] = (FEAT,)
    for g in range(GROUPS):
        for b in range(BLOCKS):
            q = f"{p}body.{g}.body.{b}.body."
            for i in (0, 2):
                d[f"{q}{i}.conv.weight"] = (FEAT, FEAT, 3, 3)
                d[f"{q}{i}.conv.bias"] = (FEAT,)
            d[q + "3.conv_du.0.weight"] = (RED, FEAT, 1, 1)
            d[q + "3.conv_du.0.bias"] = (RED,)
            d[q + "3.conv_du.2.weight"] = (FEAT, RED, 1, 1)
            d[q + "3.conv_du.2.bias"] = (FEAT,)
        d[f"{p}body.{g}.body.{BLOCKS}.conv.weight"] = (FEAT, FEAT, 3, 3)
        d[f"{p}body.{g}.body.{BLOCKS}.conv.bias"] = (FEAT,)
    d[p + "tailConv.weight"] = (FEAT, FEAT, 3, 3)
    d[p + "tailConv.bias"] = (FEAT,)
    return d


def check_state_dict(sd):
    """Strict, as ``CAIN.load_state_dict(sd)`` (vfi_models/cain/__init__.py:48): every key, no extra key, every shape."""
    want = cain_shapes()
    missing = [k for k in want if k not in sd]
    unexpected = [k for k in sd if k not in want]
    if missing or unexpected:
        raise RuntimeError(f"Error(s) in loading state_dict for CAIN: Missing key(s): {missing}. Unexpected key(s): {unexpected}.")
    for k, shp in want.items():
        if tuple(sd[k].shape) != tuple(shp):
            raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(sd[k].shape)} vs model {tuple(shp)}")


def unwrap(ckpt):
    """The checkpoint file's ``{"state_dict": ...}`` wrapper and DataParallel ``module.`` prefix, as the reference strips them
    (``key.replace('module.', '')``, vfi_models/cain/__init__.py:42-43)."""
    sd = ckpt["state_dict"]
    return {k.replace("module.", ""): v for k, v in sd.items()}


def load_file(path):
    import torch

    sd = unwrap(torch.load(path, map_location="cpu", weights_only=False))
    check_state_dict(sd)
    return sd
