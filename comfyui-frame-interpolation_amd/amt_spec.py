"""Checkpoint layout of AMT-S and AMT-L (amt-s.pth / gopro_amt-s.pth / amt-l.pth: ``{"state_dict": ...}``, loaded strictly by the node,
vfi_models/amt/__init__.py:61-66).

Key names / shapes follow ``AMT_S`` (vfi_models/amt/amt_arch.py:1153-1188) and ``AMT_L`` (:1297-1332); order = torch state_dict order.
``InstanceNorm2d`` has no parameters and no buffers (affine=False, no running statistics), so the feature encoder contributes
convolutions only.  AMT-G (``amt-g.pth``, ``AMT_G`` :1441-1590: 84/96/112/128 pyramid channels, ``LargeEncoder``, five update blocks — the
``update*_high`` blocks re-read the ``_low`` blocks' lookup output, resized) is AMT-L's forward with other tables plus those two blocks.  It
is told apart by name and served only when config.yaml's ``amt_g`` key is on (``amt_g_enabled()``): its real checkpoint has not been run
here.  With the key off it is refused as before."""
from collections import OrderedDict

VARIANTS = ("S", "L")
# checkpoint -> variant, in the reference's CKPT_CONFIGS order (the node's widget list); None = listed but not served
CKPT_VARIANT = OrderedDict((("amt-s.pth", "S"), ("amt-l.pth", "L"), ("amt-g.pth", None), ("gopro_amt-s.pth", "S")))
CONFIG = {
    "S": dict(channels=(20, 32, 44, 56), skip=20, num_flows=3, feat_dim=84, comb_k=3, stem_k=3,
              hidden=76, flow_dim=20, corr_dim=64, corr_dim2=None, fc_dim=68),
    "L": dict(channels=(48, 64, 72, 128), skip=48, num_flows=5, feat_dim=128, comb_k=7, stem_k=7,
              hidden=128, flow_dim=48, corr_dim=256, corr_dim2=160, fc_dim=124),
    "G": dict(channels=(84, 96, 112, 128), skip=84, num_flows=5, feat_dim=128, comb_k=7, stem_k=7,
              hidden=192, flow_dim=64, corr_dim=256, corr_dim2=192, fc_dim=188),
}
# the update blocks in registration order (torch state-dict order) -> the pyramid level whose channel count is their cdim
UPDATE_BLOCKS = {"S": (("update4", 2), ("update3", 1), ("update2", 0)), "L": (("update4", 2), ("update3", 1), ("update2", 0)),
                 "G": (("update4", 2), ("update3_low", 1), ("update2_low", 0), ("update3_high", 1), ("update2_high", 0))}
G_BLOCK_PREFIXES = ("update3_high.", "update2_high.", "update3_low.", "update2_low.")
CORR_LEVELS, CORR_RADIUS = 4, 3
COR_PLANES = CORR_LEVELS * (2 * CORR_RADIUS + 1) ** 2       # 196 per direction


def amt_shapes(variant):
    cfg = CONFIG[variant]
    d = OrderedDict()

    def conv(name, cout, cin, k):
        d[name + ".weight"], d[name + ".bias"] = (cout, cin, k, k), (cout,)

    def convrelu(name, cin, cout, k=3):
        conv(name + ".0", cout, cin, k)
        d[name + ".1.weight"] = (cout,)

    # feature encoder (SmallEncoder :515-587 / BasicEncoder :589-663 / LargeEncoder :665-741)
    if variant == "S":
        conv("feat_encoder.conv1", 32, 3, 7)
        cin = 32
        for i, c in enumerate((32, 64, 96)):
            for b in range(2):
                p = f"feat_encoder.layer{i + 1}.{b}."
                conv(p + "conv1", c // 4, cin if b == 0 else c, 1)
                conv(p + "conv2", c // 4, c // 4, 3)
                conv(p + "conv3", c, c // 4, 1)
                if b == 0 and i > 0:
                    conv(p + "downsample.0", c, cin, 1)
            cin = c
        conv("feat_encoder.conv2", cfg["feat_dim"], 96, 1)
    else:
        conv("feat_encoder.conv1", 64, 3, 7)
        cin = 64
        # G: a fourth, stride-1 stage layer3_2 (no downsample)
        stages = (("layer1", 64, 1), ("layer2", 72, 2), ("layer3", 128, 2)) if variant == "L" else (
            ("layer1", 64, 1), ("layer2", 112, 2), ("layer3", 160, 2), ("layer3_2", 160, 1))
        for lname, c, stride in stages:
            for b in range(2):
                p = f"feat_encoder.{lname}.{b}."
                conv(p + "conv1", c, cin if b == 0 else c, 3)
                conv(p + "conv2", c, c, 3)
                if b == 0 and stride == 2:
                    conv(p + "downsample.0", c, cin, 1)
            cin = c
        conv("feat_encoder.conv2", cfg["feat_dim"], cin, 1)
    # pyramid encoder (:801-822)
    prev = 3
    for i, c in enumerate(cfg["channels"], 1):
        convrelu(f"encoder.pyramid{i}.0", prev, c, cfg["stem_k"] if i == 1 else 3)
        convrelu(f"encoder.pyramid{i}.1", c, c)
        prev = c
    # decoders (:824-857, :905-928): convrelu, ResBlock (:762-799), ConvTranspose2d [Cin, Cout, 4, 4]
    ch, skip, nf = cfg["channels"], cfg["skip"], cfg["num_flows"]
    for name, cin, c, cout in (("decoder4", ch[3] * 2 + 1, ch[3] * 2, ch[2] + 4), ("decoder3", ch[2] * 3 + 4, ch[2] * 3, ch[1] + 4),
                               ("decoder2", ch[1] * 3 + 4, ch[1] * 3, ch[0] + 4), ("decoder1", ch[0] * 3 + 4, ch[0] * 3, 8 * nf)):
        p = name + ".convblock."
        convrelu(p + "0", cin, c)
        for j, cc in ((1, c), (2, skip), (3, c), (4, skip)):
            convrelu(f"{p}1.conv{j}", cc, cc)
        conv(p + "1.conv5", c, c, 3)
        d[p + "1.prelu.weight"] = (c,)
        d[p + "2.weight"], d[p + "2.bias"] = (c, cout, 4, 4), (cout,)
    # update blocks (SmallUpdateBlock :969-1019 / BasicUpdateBlock :1022-1073)
    hid, fd, cd, cd2, fc = cfg["hidden"], cfg["flow_dim"], cfg["corr_dim"], cfg["corr_dim2"], cfg["fc_dim"]
    for name, lvl in UPDATE_BLOCKS[variant]:
        cdim = ch[lvl]
        conv(name + ".convc1", cd, 2 * COR_PLANES, 1)
        if cd2:
            conv(name + ".convc2", cd2, cd, 3)
        conv(name + ".convf1", fd * 2, 4, 7)
        conv(name + ".convf2", fd, fd * 2, 3)
        conv(name + ".conv", fc, (cd2 or cd) + fd, 3)
        conv(name + ".gru.0", hid, fc + 4 + cdim, 3)
        conv(name + ".gru.2", hid, hid, 3)
        conv(name + ".feat_head.0", hid, hid, 3)
        conv(name + ".feat_head.2", cdim, hid, 3)
        conv(name + ".flow_head.0", hid, hid, 3)
        conv(name + ".flow_head.2", 4, hid, 3)
    conv("comb_block.0", 6 * nf, 3 * nf, cfg["comb_k"])
    d["comb_block.1.weight"] = (6 * nf,)
    conv("comb_block.2", 3, 6 * nf, cfg["comb_k"])
    return d


def amt_g_enabled():
    """config.yaml's ``amt_g`` key (absent = off), read at call time"""
    from . import ckpt

    return bool(ckpt.load_config().get("amt_g", False))


def variant_of(sd):
    """"S" or "L" by name and shape, "G" by name when ``amt_g`` is on; AMT-G raises NotImplementedError otherwise, anything else
    RuntimeError."""
    if any(k.startswith(G_BLOCK_PREFIXES) for k in sd):
        if amt_g_enabled():
            return "G"
        raise NotImplementedError("this state dict is AMT-G's (update*_high / update*_low blocks): only AMT-S and AMT-L are served "
                                  "(AMT-G is opt-in: config.yaml's amt_g key)")
    w = sd.get("encoder.pyramid1.0.0.weight")
    if w is None or "comb_block.0.weight" not in sd or "feat_encoder.conv2.weight" not in sd:
        raise RuntimeError("not an AMT state dict: no 'encoder.pyramid1.0.0.weight' / 'comb_block.0.weight' / 'feat_encoder.conv2.weight'")
    for v in VARIANTS:
        if int(w.shape[0]) == CONFIG[v]["channels"][0]:
            return v
    raise RuntimeError(f"AMT state dict with {int(w.shape[0])} first pyramid channels: neither AMT-S (20) nor AMT-L (48)")


def check_state_dict(sd, variant=None):
    """Strict, as ``load_state_dict(sd)``: every key, no extra key, every shape.  Returns the variant."""
    found = variant_of(sd)
    if variant is not None and found != variant:
        raise RuntimeError(f"AMT-{found} state dict where AMT-{variant} is expected")
    want = amt_shapes(found)
    missing = [k for k in want if k not in sd]
    unexpected = [k for k in sd if k not in want]
    if missing or unexpected:
        raise RuntimeError(f"Error(s) in loading state_dict for AMT_{found}: Missing key(s): {missing}. Unexpected key(s): {unexpected}.")
    for k, shp in want.items():
        if tuple(sd[k].shape) != tuple(shp):
            raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(sd[k].shape)} vs model {tuple(shp)}")
    return found


def variant_of_ckpt(ckpt_name):
    """The variant a checkpoint name stands for; amt-g.pth is "G" when config.yaml's ``amt_g`` key is on and raises NotImplementedError
    naming it otherwise, before anything is loaded."""
    if ckpt_name not in CKPT_VARIANT:
        raise KeyError(f"unknown AMT checkpoint {ckpt_name!r} (known: {list(CKPT_VARIANT)})")
    v = CKPT_VARIANT[ckpt_name]
    if v is None:
        if amt_g_enabled():
            return "G"
        raise NotImplementedError(f"{ckpt_name}: AMT-G has a forward of its own (update*_high blocks) and is not served; use amt-s.pth, "
                                  "gopro_amt-s.pth or amt-l.pth (AMT-G is opt-in: config.yaml's amt_g key)")
    return v


def load_file(path, ckpt_name=None):
    """<ckpts_path>/amt/<ckpt> -> (checked state dict, variant).  The real files are ``{"state_dict": ...}``."""
    import os

    import torch

    want = variant_of_ckpt(ckpt_name or os.path.basename(path))
    blob = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(blob, dict) or "state_dict" not in blob:
        raise RuntimeError(f"{path}: an AMT checkpoint is a dict with a 'state_dict' entry")
    sd = blob["state_dict"]
    return sd, check_state_dict(sd, want)


def seeded_state_dict(variant, seed):
    """A stand-in for the AMT checkpoints, for the tests and goldens: PyTorch's default initialisation magnitudes, drawn in state-dict
    order from one generator.  Convolution weights and biases are U(-1/sqrt(fan_in), 1/sqrt(fan_in)) (fan_in of a ConvTranspose2d weight
    [Cin, Cout, 4, 4] as torch takes it: shape[1] * 16); the feature encoder's weights are N(0, 2 / fan_out) as its own kaiming_normal_
    (amt_arch.py:546-548, :621-623) leaves them; PReLU slopes are 0.25.  Nothing is scaled up: with these magnitudes the lookup moves
    the frame by more than 1e-2 on average and almost no output value is clamped (tests/test_amt_restated_cpu.py asserts both), while
    weights 1.5 times larger already saturate most of the frame."""
    import torch

    g = torch.Generator().manual_seed(seed)
    shapes = amt_shapes(variant)
    sd = {}
    for k, shp in shapes.items():
        if len(shp) == 1 and not k.endswith(".bias"):
            sd[k] = torch.full(shp, 0.25)
            continue
        # fan_in from the layer's OWN weight, looked up by name (a bias takes its layer's); torch's fan_in of a 4-d weight is
        # shape[1] * kh * kw for Conv2d [Cout, Cin, k, k] and for ConvTranspose2d [Cin, Cout, 4, 4] alike
        wshape = shapes[k.rsplit(".", 1)[0] + ".weight"]
        fan = wshape[1] * wshape[2] * wshape[3]
        if k.endswith(".weight") and k.startswith("feat_encoder."):
            sd[k] = torch.randn(shp, generator=g, dtype=torch.float32) * (2.0 / (shp[0] * shp[2] * shp[3])) ** 0.5
            continue
        sd[k] = (torch.rand(shp, generator=g, dtype=torch.float32) * 2 - 1) / fan ** 0.5
    return sd
