"""Checkpoint layout of FLAVR (FLAVR_2x.pth / FLAVR_4x.pth / FLAVR_8x.pth: ``{"state_dict": ...}`` of a DataParallel model, every key
under ``module.``; the node strips the prefix with ``k.partition("module.")[-1]``, vfi_models/flavr/__init__.py:14-23).

Key names / shapes follow ``UNet_3D_3D("unet_18", n_inputs=4, n_outputs, joinType="concat", upmode="transpose")``
(vfi_models/flavr/flavr_arch.py:134-164, resnet_3D.py); order = torch state_dict order.  The encoder's convolutions (stem and the
BasicBlocks' 3x3x3 layers) carry a bias only when n_outputs > 1 (resnet_3D.useBias); the 1x1x1 downsample never does.  n_outputs is
read from the file: ``outconv.1.weight.shape[0] // 3`` — 1 for the 2x checkpoint, 3 for 4x, 7 for 8x."""
from collections import OrderedDict

N_INPUTS = 4
LAYERS = ((64, 64), (64, 128), (128, 256), (256, 512))      # layer1..layer4: (inplanes, planes), two BasicBlocks each


def flavr_shapes(n_outputs):
    bias = n_outputs > 1
    d = OrderedDict()

    def conv(name, shape, has_bias):
        d[name + ".weight"] = tuple(shape)
        if has_bias:
            d[name + ".bias"] = (shape[0],)

    def gate(name, c):
        conv(name + ".attn_layer.0", (c, c, 1, 1, 1), True)

    conv("encoder.stem.0", (64, 3, 3, 7, 7), bias)
    for i, (cin, c) in enumerate(LAYERS):
        for b in range(2):
            p = f"encoder.layer{i + 1}.{b}."
            conv(p + "conv1.0", (c, cin if b == 0 else c, 3, 3, 3), bias)
            conv(p + "conv2.0", (c, c, 3, 3, 3), bias)
            gate(p + "fg", c)
            if b == 0 and cin != c:
                conv(p + "downsample.0", (c, cin, 1, 1, 1), False)
    conv("decoder.0.conv.0", (256, 512, 3, 3, 3), True)
    gate("decoder.0.conv.1", 256)
    for i, (cin, c) in ((1, (512, 128)), (2, (256, 64))):
        d[f"decoder.{i}.upconv.0.weight"], d[f"decoder.{i}.upconv.0.bias"] = (cin, c, 3, 4, 4), (c,)      # ConvTranspose3d: [Cin, Cout, ...]
        gate(f"decoder.{i}.upconv.1", c)
    conv("decoder.3.conv.0", (64, 128, 3, 3, 3), True)
    gate("decoder.3.conv.1", 64)
    d["decoder.4.upconv.0.weight"], d["decoder.4.upconv.0.bias"] = (128, 64, 3, 4, 4), (64,)
    gate("decoder.4.upconv.1", 64)
    conv("feature_fuse.conv.0", (64, 64 * N_INPUTS, 1, 1), False)
    conv("outconv.1", (3 * n_outputs, 64, 7, 7), True)
    return d


def n_outputs_of(sd):
    return int(sd["outconv.1.weight"].shape[0]) // 3


def check_state_dict(sd):
    """Strict, as ``UNet_3D_3D.load_state_dict(sd)``: every key, no extra key, every shape."""
    if "outconv.1.weight" not in sd:
        raise RuntimeError("FLAVR state dict has no 'outconv.1.weight' (the node reads the number of outputs from it)")
    want = flavr_shapes(n_outputs_of(sd))
    missing = [k for k in want if k not in sd]
    unexpected = [k for k in sd if k not in want]
    if missing or unexpected:
        raise RuntimeError(f"Error(s) in loading state_dict for UNet_3D_3D: Missing key(s): {missing}. Unexpected key(s): {unexpected}.")
    for k, shp in want.items():
        if tuple(sd[k].shape) != tuple(shp):
            raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(sd[k].shape)} vs model {tuple(shp)}")


def strip_module_prefix(sd):
    """The reference's ``{k.partition("module.")[-1]: v}``: a key without ``module.`` becomes the empty string there (and the load fails
    on it as an unexpected key); here that case is named."""
    bare = [k for k in sd if "module." not in k]
    if bare:
        raise RuntimeError(f"FLAVR checkpoint keys without the 'module.' prefix (the file must be the DataParallel state dict): {bare[:4]}")
    return {k.partition("module.")[-1]: v for k, v in sd.items()}


def load_file(path):
    """<ckpts_path>/flavr/FLAVR_{2,4,8}x.pth -> the checked state dict"""
    import torch

    sd = strip_module_prefix(torch.load(path, map_location="cpu", weights_only=False)["state_dict"])
    check_state_dict(sd)
    return sd


def seeded_state_dict(seed, n_outputs):
    """A stand-in for the FLAVR checkpoints, for the tests and goldens.  PyTorch's default initialisation
    (U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weights and biases) leaves the network's contribution ``out - mean`` at a standard
    deviation of about 0.01, which a 1e-3 gate can hardly see; here every convolution weight is 2.4 times that draw and every gate bias
    is raised by 2 (gates mostly open), which brings it to about 0.15 (tests/test_flavr_spec_cpu.py asserts >= 0.05 at 64x96).  Drawn
    in state-dict order from one generator.  fan_in of a ConvTranspose3d weight [Cin, Cout, ...] is taken as torch does: shape[1] * k."""
    import torch

    g = torch.Generator().manual_seed(seed)
    sd, fan = {}, None
    for k, shp in flavr_shapes(n_outputs).items():
        if k.endswith(".weight"):
            fan = 1
            for s in shp[1:]:
                fan *= s
        bound = 1.0 / fan ** 0.5
        t = (torch.rand(shp, generator=g, dtype=torch.float32) * 2 - 1) * bound
        if k.endswith(".weight"):
            t = t * 2.4
        elif "attn_layer" in k:
            t = t + 2.0
        sd[k] = t
    return sd
