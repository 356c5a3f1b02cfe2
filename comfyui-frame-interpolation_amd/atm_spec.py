"""Checkpoint layout of ATM-lite (atm-vfi-lite.pt: ``{"model_state_dict": ...}``, loaded strictly by the node after the ``attn_mask`` / ``HW``
entries have been dropped, vfi_models/atm/__init__.py:128-142).

Key names / shapes follow ``network_lite.Network`` (vfi_models/atm/network_lite.py:88-273) with ``ATMFormer`` / ``RefineBottleneck``
(attention.py:216-237, :393-416); order = torch state_dict order (a module's own parameters, then its buffers, then its children): 236
entries, 11 975 523 parameters, plus the four ``relative_coord`` buffers of the ATM blocks.  Those buffers are not weights: they hold key
position minus query position inside the window (x, then y; attention.py:150-165), which the attention kernel computes itself, so a file
whose buffers say otherwise is refused (``load_file``).

ATM-base (atm-vfi-base.pt and its perceptual-loss fine-tune atm-vfi-base-pct.pt: ``network_base.Network``, network_base.py:88-260) has the same
module tree and forward, hence the same 236 names in the same order; only the widths differ (``CONFIG``): 51 564 259 parameters.  It is
served only when config.yaml's ``atm_base`` key is on (``atm_base_enabled()``); absent or off, both files and 24-channel state dicts are
refused as before.

The multi-scale global-motion ensemble ("On with Ensemble (slowest)", for both models) is served only when config.yaml's ``atm_ensemble`` key
is on (``atm_ensemble_enabled()``); absent or off, the choice is refused by name as before.

Frames beyond the 2 GiB-per-image limits (2160x3840 for both models) are served only when config.yaml's ``atm_large_frames`` key is on
(``atm_large_frames_enabled()``); absent or off, the limits and the refusal are what they were."""
from collections import OrderedDict

CKPT_NAMES = ("atm-vfi-base.pt", "atm-vfi-lite.pt", "atm-vfi-base-pct.pt")      # the reference's widget order
LITE = "atm-vfi-lite.pt"
HIDDEN = (16, 32, 64, 96)
HEADS = 8
LOCAL_DIM, LOCAL_WIN = 224, 8        # 96 + 64 + 2 * 32 on the H/8 map
GLOBAL_DIM, GLOBAL_WIN = 352, 12     # 128 + 96 + 2 * 64 on the H/16 map
MOTION_OUT = 5                       # flow 0 (x, y), flow 1 (x, y), mask logit
N_TENSORS, N_PARAMETERS = 236, 11975523
VARIANTS = ("lite", "base")          # the index is vfi_atm_create_variant's ``variant``
CKPT_VARIANT = {"atm-vfi-base.pt": "base", "atm-vfi-lite.pt": "lite", "atm-vfi-base-pct.pt": "base"}
# hidden: hidden_dims; last_extra: last_feat_extract's width over hidden[-1]; mlp_ratio: of all six windowed blocks (base passes none: the
# class default); local_head / global_head: the motion heads' hidden widths (lite 0.5 x 448 and 352, base int(0.75 x 768) and the constant
# 768); refine: the refinement net's hidden_dim
CONFIG = {"lite": dict(hidden=HIDDEN, last_extra=32, mlp_ratio=2, local_head=224, global_head=352, refine=32, n_parameters=N_PARAMETERS),
          "base": dict(hidden=(24, 48, 96, 192), last_extra=96, mlp_ratio=4, local_head=576, global_head=768, refine=64, n_parameters=51564259)}


def atm_shapes(variant="lite"):
    cfg = CONFIG[variant]
    HIDDEN = cfg["hidden"]
    LOCAL_DIM = HIDDEN[3] + HIDDEN[2] + 2 * HIDDEN[1]
    GLOBAL_DIM = 2 * HIDDEN[3] + cfg["last_extra"] + 2 * HIDDEN[2]
    d = OrderedDict()

    def conv(name, cout, cin, k=3):
        d[name + ".weight"], d[name + ".bias"] = (cout, cin, k, k), (cout,)

    def convprelu(name, cin, cout):
        conv(name + ".0", cout, cin)
        d[name + ".1.weight"] = (cout,)

    def deconv(name, cin, cout):      # ConvTranspose2d(cin, cout, 2, 2, 0) + PReLU
        d[name + ".0.weight"], d[name + ".0.bias"], d[name + ".1.weight"] = (cin, cout, 2, 2), (cout,), (cout,)

    def linear(name, cout, cin, bias=True):
        d[name + ".weight"] = (cout, cin)
        if bias:
            d[name + ".bias"] = (cout,)

    def norm(name, c):
        d[name + ".weight"], d[name + ".bias"] = (c,), (c,)

    def mlp(name, c, ratio=cfg["mlp_ratio"]):
        linear(name + ".fc1", ratio * c, c)
        d[name + ".dwconv.dwconv.weight"], d[name + ".dwconv.dwconv.bias"] = (ratio * c, 1, 3, 3), (ratio * c,)
        linear(name + ".fc2", c, ratio * c)

    def fusion(name, dims):      # CrossScaleFeatureFusion(in_dims = dims) (:34-56)
        conv(name + ".layers.0", dims[1], dims[1])
        conv(name + ".layers.1", dims[0], dims[0])
        conv(name + ".layers.2", dims[0], dims[0])
        c = 2 * dims[0] + dims[1] + dims[2]
        conv(name + ".proj", c, c, 1)
        norm(name + ".norm", c)

    def atmformer(name, c, win):
        norm(name + ".norm1", c)
        d[name + ".attn.relative_coord"] = (1, 1, 2, win * win, win * win)
        linear(name + ".attn.q", c, c, False)
        linear(name + ".attn.kv", 2 * c, c, False)
        linear(name + ".attn.proj", c, c)
        linear(name + ".attn.mlp.0", HEADS // 2, HEADS)
        linear(name + ".attn.mlp.2", 1, HEADS // 2)
        norm(name + ".norm2", c)
        mlp(name + ".mlp", c)

    def motion_mlp(name, c, hidden):
        convprelu(name + ".0", 2 * c + HEADS, hidden)
        convprelu(name + ".1", hidden, hidden)
        conv(name + ".2", MOTION_OUT, hidden, 1)

    prev = 3
    for i, c in enumerate(HIDDEN):
        convprelu(f"feat_extracts.{i}.0", prev, c)
        convprelu(f"feat_extracts.{i}.1", c, c)
        prev = c
    fusion("cross_scale_feature_fusion", HIDDEN[1:])
    for k in range(2):      # RefineBottleneck
        p = f"feat_enhance_transformer.{k}"
        norm(p + ".norm1", LOCAL_DIM)
        linear(p + ".attn.qkv", 3 * LOCAL_DIM, LOCAL_DIM, False)
        linear(p + ".attn.proj", LOCAL_DIM, LOCAL_DIM)
        norm(p + ".norm2", LOCAL_DIM)
        mlp(p + ".mlp", LOCAL_DIM)
    for k in range(2):
        atmformer(f"local_motion_atmformer.{k}", LOCAL_DIM, LOCAL_WIN)
    motion_mlp("local_motion_mlp", LOCAL_DIM, cfg["local_head"])
    last = HIDDEN[-1] + cfg["last_extra"]
    convprelu("last_feat_extract.0", HIDDEN[-1], last)
    convprelu("last_feat_extract.1", last, last)
    fusion("global_feature_fusion", (HIDDEN[-2], HIDDEN[-1], last))
    for k in range(2):
        atmformer(f"global_motion_atmformer.{k}", GLOBAL_DIM, GLOBAL_WIN)
    motion_mlp("global_motion_mlp", GLOBAL_DIM, cfg["global_head"])
    cin = 2 * LOCAL_DIM + MOTION_OUT
    for i, f in enumerate((LOCAL_DIM, LOCAL_DIM // 2, LOCAL_DIM // 4)):
        p, c = f"upsample_pyramid.{i}", f + MOTION_OUT
        j = 0
        if i > 0:
            d[p + ".0.weight"] = (cin,)
            j = 1
        deconv(f"{p}.{j}", cin, c)
        convprelu(f"{p}.{j + 1}", c, c)
        conv(f"{p}.{j + 2}", c, c)
        cin = c
    hid = cfg["refine"]
    convprelu("proj", LOCAL_DIM // 4 + MOTION_OUT + 15, hid)
    convprelu("down1.0", hid, hid)
    convprelu("down2.0", LOCAL_DIM // 2 + hid, 2 * hid)
    convprelu("down2.1", 2 * hid, 2 * hid)
    convprelu("down3.0", LOCAL_DIM + 2 * hid, 4 * hid)
    convprelu("down3.1", 4 * hid, 4 * hid)
    convprelu("down3.2", 4 * hid, 4 * hid)
    deconv("up1.0", 4 * hid, 2 * hid)
    convprelu("up1.1", 2 * hid, 2 * hid)
    deconv("up2.0", 4 * hid, 2 * hid)
    convprelu("up2.1", 2 * hid, hid)
    deconv("up3.0", 2 * hid, hid)
    convprelu("refine_head.0", 2 * hid, hid)
    convprelu("refine_head.1", hid, 3)
    return d


def weight_shapes(variant="lite"):
    """The tensors the C object takes (vfi_atm_create / vfi_atm_create_variant), in order: every entry but the ``relative_coord`` buffers."""
    return OrderedDict((k, v) for k, v in atm_shapes(variant).items() if not k.endswith(".relative_coord"))


def relative_coord(win):
    """[1,1,2,win^2,win^2]: [.., 0, q, k] = key x - query x, [.., 1, q, k] = key y - query y, tokens row-major in the window."""
    import torch

    i = torch.arange(win * win)
    x, y = (i % win).float(), (i // win).float()
    return torch.stack([x[None, :] - x[:, None], y[None, :] - y[:, None]])[None, None]


def atm_base_enabled():
    """config.yaml's ``atm_base`` key (absent = off), read at call time"""
    from . import ckpt

    return bool(ckpt.load_config().get("atm_base", False))


def atm_ensemble_enabled():
    """config.yaml's ``atm_ensemble`` key (absent = off), read at call time"""
    from . import ckpt

    return bool(ckpt.load_config().get("atm_ensemble", False))


def atm_large_frames_enabled():
    """config.yaml's ``atm_large_frames`` key (absent = off), read at call time"""
    from . import ckpt

    return bool(ckpt.load_config().get("atm_large_frames", False))


def check_ckpt_name(ckpt_name):
    """-> the variant the name stands for.  The two base files are "base" when config.yaml's ``atm_base`` key is on and raise
    NotImplementedError naming themselves otherwise, before anything is loaded."""
    if ckpt_name not in CKPT_NAMES:
        raise KeyError(f"unknown ATM checkpoint {ckpt_name!r} (known: {list(CKPT_NAMES)})")
    if ckpt_name != LITE and not atm_base_enabled():
        raise NotImplementedError(f"{ckpt_name}: ATM-base is not built yet; only {LITE} (ATM-lite) is served")
    return CKPT_VARIANT[ckpt_name]


def check_state_dict(sd, variant=None):
    """Strict, as ``load_state_dict(sd)``: every key, no extra key, every shape; and the ``relative_coord`` buffers equal the analytic table.
    variant None: told by the first convolution's width (16 = lite; 24 = base, with ``atm_base`` on); a dict of the other model than the
    variant asked for is a size mismatch, as it is for ``load_state_dict``.  Returns the variant."""
    import torch

    first = sd.get("feat_extracts.0.0.0.weight")
    width = None if first is None else int(first.shape[0])
    if not atm_base_enabled():
        if width is not None and width != HIDDEN[0]:
            raise NotImplementedError(f"an ATM state dict with {width} first feature channels: ATM-base is not built yet; only ATM-lite "
                                      f"({HIDDEN[0]}) is served")
        if variant == "base":
            raise NotImplementedError(f"ATM-base is not built yet; only {LITE} (ATM-lite) is served")
        variant = "lite"
    elif variant is None:
        variant = "base" if width == CONFIG["base"]["hidden"][0] else "lite"
    want = atm_shapes(variant)
    missing = [k for k in want if k not in sd]
    unexpected = [k for k in sd if k not in want]
    if missing or unexpected:
        raise RuntimeError(f"Error(s) in loading state_dict for Network: Missing key(s): {missing}. Unexpected key(s): {unexpected}.")
    for k, shp in want.items():
        if tuple(sd[k].shape) != tuple(shp):
            raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(sd[k].shape)} vs model {tuple(shp)}")
    for k, shp in want.items():
        if k.endswith(".relative_coord"):
            win = int(round(shp[3] ** 0.5))
            if not torch.equal(sd[k].detach().to("cpu", torch.float32), relative_coord(win)):
                raise RuntimeError(f"{k} is not key position minus query position inside the {win}x{win} window: the attention kernel computes "
                                   "these offsets itself and cannot serve a checkpoint trained with another table")
    return variant


def load_file(path, ckpt_name=None):
    """<ckpts_path>/atm/<ckpt> -> checked state dict.  The real file is ``{"model_state_dict": ...}``; keys containing ``attn_mask`` or ``HW``
    (masks a training run cached) are dropped, as the node does."""
    import os

    import torch

    variant = check_ckpt_name(ckpt_name or os.path.basename(path))
    blob = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(blob, dict) or "model_state_dict" not in blob:
        raise RuntimeError(f"{path}: an ATM checkpoint is a dict with a 'model_state_dict' entry")
    sd = OrderedDict((k, v) for k, v in blob["model_state_dict"].items() if "attn_mask" not in k and "HW" not in k)
    check_state_dict(sd, variant)
    return sd


# gains of seeded_state_dict over torch's default draws
GAIN_CONV, GAIN_QKV, GAIN_LINEAR, GAIN_GLOBAL_HEAD = 2.0, 4.0, 2.0, 1.0
# (conv, q / kv / qkv, other linears, global_motion_mlp.2) per variant
GAINS = {"lite": (GAIN_CONV, GAIN_QKV, GAIN_LINEAR, GAIN_GLOBAL_HEAD), "base": (2.0, 4.0, 3.0, 1.0)}


def seeded_state_dict(seed, variant="lite"):
    """A stand-in for atm-vfi-lite.pt, for the tests and goldens.  With the network's own initialisation (trunc_normal 0.02 linears, unit
    LayerNorms) the model is dead: final flows of 0.05 px, and the motion read-out of the ATM blocks moves the frame by 2e-8.  So the draws
    are torch's default ``reset_parameters`` ones, U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weights and biases, in state-dict order from one
    generator, with gains per group of layers: convolution and transposed-convolution weights x GAIN_CONV = 2.0, the q / kv / qkv weights x
    GAIN_QKV = 4 (peaked attention, so the read-out carries a signal), every other linear weight x GAIN_LINEAR = 2, the last layer of the
    global motion head (global_motion_mlp.2) x GAIN_GLOBAL_HEAD = 1 (its flows are multiplied by 16 on the way to full resolution: at x 2 a
    64x64 frame is warped out of itself and 17 % of the "On" output is clamped at 0), LayerNorm weights
    U(0.5, 1.5) and biases U(-0.2, 0.2) (the bias is what a pad token holds after norm1), PReLU slopes 0.25.  Biases keep gain 1.
    tests/test_atm_restated_cpu.py asserts what the gains are for, at every golden shape and in both global-motion modes: read-out effect >=
    1e-3, largest flow >= 0.5 px, <= 10 % of the output clamped, float32 within 1e-4 of float64 (at x 2.4 the "On" mode clamps half the
    frame).

    variant "base": a stand-in for atm-vfi-base.pt, drawn the same way over base's shapes with GAINS["base"] = (conv 2, q / kv / qkv 4, other
    linears 3, global_motion_mlp.2 1).  Lite's gains do not carry over: base's linears have 1.7 to 2 times the fan-in (384 / 672 / 1536 /
    2688 against 224 / 352 / 448 / 704), and at lite's linear gain of 2 the read-out effect with global motion off is 9.9e-4 at 128x192 and
    8.6e-4 at 192x320, below the 1e-3 the condition asks (q / kv / qkv at 6 instead also passes, with less margin).  With the gains above
    the reference's network_base.Network gives (tests/golden/atm_base_net.npz; On / Off over the three golden shapes): read-out effect
    2.5e-2 .. 5.7e-2 / 2.8e-3 .. 5.2e-3, largest flow 1.80 .. 2.10 / 1.60 .. 2.03 px, clamped <= 1.7 % / <= 1.5 %, and the float32
    restatement is within 3.1e-5 of the float64 one.  tests/test_atm_base_cpu.py asserts the four conditions."""
    import torch

    g = torch.Generator().manual_seed(seed)
    shapes = atm_shapes(variant)
    gain_conv, gain_qkv, gain_linear, gain_global_head = GAINS[variant]
    sd = OrderedDict()

    def uni(shp, lo, hi):
        return torch.rand(shp, generator=g, dtype=torch.float32) * (hi - lo) + lo

    for k, shp in shapes.items():
        if k.endswith(".relative_coord"):
            sd[k] = relative_coord(int(round(shp[3] ** 0.5)))
            continue
        stem, leaf = k.rsplit(".", 1)
        wshape = shapes.get(stem + ".weight", shp)
        if ".norm" in k and len(wshape) == 1:      # LayerNorm
            sd[k] = uni(shp, 0.5, 1.5) if leaf == "weight" else uni(shp, -0.2, 0.2)
        elif len(wshape) == 1:                     # PReLU
            sd[k] = torch.full(shp, 0.25)
        else:
            fan = wshape[1] * (wshape[2] * wshape[3] if len(wshape) == 4 else 1)
            gain = 1.0
            if leaf == "weight":
                gain = gain_global_head if k == "global_motion_mlp.2.weight" else gain_conv if len(wshape) == 4 else (gain_qkv if stem.rsplit(".", 1)[1] in ("q", "kv", "qkv") else gain_linear)
            sd[k] = uni(shp, -1.0, 1.0) * (gain / fan ** 0.5)
    return sd
