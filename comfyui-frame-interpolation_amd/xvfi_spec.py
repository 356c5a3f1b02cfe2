"""XVFI checkpoint layout (vfi_models/xvfi/xvfi_arch.py XVFInet with nf = 64, img_ch = 3; xvfi/__init__.py:12-37) — pure Python, no GPU.

The state dict has 72 tensors for ``module_scale_factor`` 2 (Vimeo) and 74 for 4 (X4K): ``XVFInet`` registers ``channel_converter`` and
``rec_ext_ds`` and then again inside the ``rec_ext_ds_module`` Sequential (``rec_ext_ds`` once per halving, i.e. log2(scale) times), so
their tensors appear under both names.  ``xvfi_shapes`` lists every key in the reference's order, aliases included; ``ALIASES`` says which
key each alias repeats, and ``check_state_dict`` refuses a state dict whose aliased tensors differ (a module cannot hold that).  Conv3d
weights have a temporal kernel of 1: [Cout, Cin, 1, 3, 3].  ``refine_unet.conv1`` / ``conv2`` are in the state dict and in no forward.
"""
from collections import OrderedDict

NF = 64
CKPT_CONFIGS = {
    "XVFInet_X4K1000FPS_exp1_latest.pt": {"module_scale_factor": 4, "S_trn": 3, "S_tst": 5},
    "XVFInet_Vimeo_exp1_latest.pt": {"module_scale_factor": 2, "S_trn": 1, "S_tst": 1},
}
# the two layers flow_gain multiplies in seeded_state_dict: the last layers of the towers that produce flow_l_tmp
FLOW_HEADS = ("vfinet.conv_flow_bottom.10", "vfinet.conv_flow2.10")


def config_of(config):
    """A checkpoint name or a (module_scale_factor, S_tst) pair -> (scale, S_tst)"""
    if isinstance(config, str):
        if config not in CKPT_CONFIGS:
            raise KeyError(f"unknown XVFI checkpoint {config!r} (known: {list(CKPT_CONFIGS)})")
        c = CKPT_CONFIGS[config]
        return c["module_scale_factor"], c["S_tst"]
    scale, s_tst = config
    if scale not in (2, 4) or not 0 <= int(s_tst) < 8:
        raise ValueError(f"XVFI: module_scale_factor {scale} (2 or 4), S_tst {s_tst} (0..7)")
    return int(scale), int(s_tst)


def divide_of(config):
    """The node pads the bottom / right with zeros to a multiple of this (xvfi/__init__.py:84-89): 16 for Vimeo, 512 for X4K"""
    scale, s_tst = config_of(config)
    return 2 ** s_tst * scale * 4


def padded_size(H, W, config):
    d = divide_of(config)
    return H + (d - H % d) % d, W + (d - W % d) % d


def _halvings(scale):
    return {2: 1, 4: 2}[scale]


def xvfi_shapes(scale):
    """Ordered {key: shape} = XVFInet(args).state_dict() for module_scale_factor ``scale``"""
    d = OrderedDict()

    def conv(name, cout, cin, k, three_d=False):
        d[name + ".weight"] = (cout, cin, 1, k, k) if three_d else (cout, cin, k, k)
        d[name + ".bias"] = (cout,)

    def tower(name, first, cin, cout):      # Conv(4,2,1) ReLU Conv(4,2,1) ReLU Up Conv3 ReLU Up Conv3 ReLU Conv3, numbered from `first`
        conv(f"{name}.{first}", 2 * NF, cin, 4)
        conv(f"{name}.{first + 2}", 4 * NF, 2 * NF, 4)
        conv(f"{name}.{first + 5}", 2 * NF, 4 * NF, 3)
        conv(f"{name}.{first + 8}", NF, 2 * NF, 3)
        conv(f"{name}.{first + 10}", cout, NF, 3)

    tower("vfinet.conv_flow_bottom", 0, 2 * NF, 6)
    conv("vfinet.conv_flow1", NF, 2 * NF, 3)
    tower("vfinet.conv_flow2", 0, 2 * NF + 4, 6)
    conv("vfinet.conv_flow3.0", NF, 4 * NF + 4, 1)
    tower("vfinet.conv_flow3", 2, NF, 4)
    u = "vfinet.refine_unet."
    conv(u + "conv1", NF, NF, 3)
    conv(u + "conv2", NF, NF, 3)
    conv(u + "enc1", NF, 4 * NF // scale // scale + 4 * 3 + 4, 4)
    conv(u + "enc2", 2 * NF, NF, 4)
    conv(u + "enc3", 4 * NF, 2 * NF, 4)
    conv(u + "dec0", 4 * NF, 4 * NF, 3)
    conv(u + "dec1", 2 * NF, 6 * NF, 3)
    conv(u + "dec2", NF, 3 * NF, 3)
    conv(u + "dec3", 4, NF, 3)
    conv("channel_converter.0", NF, 3, 3, True)
    conv("rec_ext_ds", NF, NF, 3, True)
    m = "rec_ext_ds_module."
    conv(m + "0.0", NF, 3, 3, True)
    n = _halvings(scale)
    for i in range(n):
        conv(f"{m}{1 + 2 * i}", NF, NF, 3, True)
    conv(f"{m}{1 + 2 * n}", NF, NF, 3, True)
    for rb in ("resblock1", "resblock2"):
        for c in ("conv3x3_1", "conv3x3_2"):
            conv(f"{m}{2 + 2 * n}.{rb}.{c}", NF, NF, 3, True)
    conv("rec_ctx_ds", NF, NF, 3, True)
    return d


def aliases(scale):
    """{alias key: the key it repeats}: one module registered twice"""
    a = {}
    for p in ("weight", "bias"):
        a[f"rec_ext_ds_module.0.0.{p}"] = f"channel_converter.0.{p}"
        for i in range(_halvings(scale)):
            a[f"rec_ext_ds_module.{1 + 2 * i}.{p}"] = f"rec_ext_ds.{p}"
    return a


def check_state_dict(sd, scale):
    """Strict, as ``load_state_dict(sd)``: every key, no extra key, every shape; and every aliased tensor equal to the one it repeats."""
    import torch

    want = xvfi_shapes(scale)
    missing = [k for k in want if k not in sd]
    unexpected = [k for k in sd if k not in want]
    if missing or unexpected:
        raise RuntimeError(f"Error(s) in loading state_dict for XVFInet: Missing key(s): {missing}. Unexpected key(s): {unexpected}.")
    for k, shp in want.items():
        if tuple(sd[k].shape) != tuple(shp):
            raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(sd[k].shape)} vs model {tuple(shp)}")
    for k, src in aliases(scale).items():
        if not torch.equal(sd[k], sd[src]):
            raise RuntimeError(f"XVFI state dict: {k} differs from {src}, which it repeats (one module registered twice): refused")


def load_file(path, ckpt_name=None):
    """<ckpts_path>/xvfi/<ckpt> -> checked state dict.  The real files are ``{"state_dict_Model": ...}`` (xvfi/__init__.py:37)."""
    import os

    import torch

    scale, _ = config_of(ckpt_name or os.path.basename(path))
    blob = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(blob, dict) or "state_dict_Model" not in blob:
        raise RuntimeError(f"{path}: an XVFI checkpoint is a dict with a 'state_dict_Model' entry")
    sd = blob["state_dict_Model"]
    check_state_dict(sd, scale)
    return sd


def seeded_state_dict(config, seed, flow_gain=1.0):
    """A stand-in for the XVFI checkpoints, for the tests and goldens: PyTorch's default initialisation magnitudes (weights and biases
    U(-1/sqrt(fan_in), 1/sqrt(fan_in))) drawn in state-dict order from one generator, aliases copied from the key they repeat.  With these
    magnitudes the flows are a small fraction of a pixel and the splat and the warps' gate do nothing; ``flow_gain`` multiplies weight and
    bias of ``conv_flow_bottom.10`` and ``conv_flow2.10`` only, the layers that emit flow_l_tmp."""
    import torch

    scale, _ = config_of(config)
    g = torch.Generator().manual_seed(seed)
    shapes = xvfi_shapes(scale)
    al = aliases(scale)
    sd = {}
    for k, shp in shapes.items():
        if k in al:
            sd[k] = sd[al[k]].clone()
            continue
        wshape = shapes[k.rsplit(".", 1)[0] + ".weight"]
        fan = 1
        for n in wshape[1:]:
            fan *= n
        v = (torch.rand(shp, generator=g, dtype=torch.float32) * 2 - 1) / fan ** 0.5
        if k.rsplit(".", 1)[0] in FLOW_HEADS:
            v = v * float(flow_gain)
        sd[k] = v
    return sd
