"""TEST INFRASTRUCTURE: the torch restatement of ATM's multi-scale global-motion ensemble ("On with Ensemble (slowest)":
vfi_models/atm/network_lite.py:540-704, network_base.py has the same code) on top of tests/atm_restated.py (lite) and
tests/atm_base_restated.py (base), both imported and left as they are; the float32 / float64 yardstick of tests/test_atm_ensemble_cpu.py and
tests/test_gpu_atm_ensemble.py, and the cases of the ensemble goldens (tools/make_golden_atm_ensemble.py).

``forward_global_ensemble`` is ``forward_normal``'s "On" path with the global motion head's flows replaced by the ensemble's choice, so the
restatement runs the variant's own ``atm_forward`` with ``motion_head`` wrapped for the one call that names ``global_motion_mlp``: the wrapper
computes level 0 as "On" does, runs the global branch again on the x0.5 and x0.25 frames, scores the three flow pairs
(``alignment_loss``), and hands back the winner resized to the 1/16 map.  The unused global-level mask logit is level 0's.

One property of the reference is reproduced as it is.  The SHIFTED block of the global branch keeps the additive mask it built at its first
call and re-uses it whenever the padded map has as many positions as then (attention.py:279-305).  Inside one ensemble forward that block
runs at three map sizes; where two consecutive levels pad to the same 12-multiple (a 4x4, a 2x2 and a 1x1 map all pad to 12x12), the later
level is masked with the EARLIER level's pad regions.  ``mask_level`` states the rule (it is stateless for a fixed frame size: the padded sizes
do not grow with the level, so equal position counts mean equal padded sizes), ``labels_of`` applies it: the shifted block of level k takes
its pad labels from the map of level ``mask_level(k)``.  The unshifted block always builds its own mask."""
import contextlib
import math

import torch
import torch.nn.functional as F

import atm_base_restated as B
import atm_restated as R

SEED, TOL, WIN = R.SEED, R.TOL, 12
ENSEMBLE = "On with Ensemble (slowest)"
NET_STRIDE, NODE_STRIDE = R.NET_STRIDE, R.NODE_STRIDE
MARGIN = 1e-2          # the smallest loss of a golden case is at least this far (relative) below the second smallest
LOSS_TOL = 1e-3        # relative, a tenth of the margin: a disagreement within it cannot flip a golden's choice
# the forward goldens' cases per model: name -> (h, w, frame seed); frames cain_restated.seeded_frames(2, h, w, 3, seed)
NET_CASES = {"lite": {"64x64": (64, 64, 9), "64x64_s7": (64, 64, 7), "64x128": (64, 128, 9), "128x128_s2": (128, 128, 2), "128x192_s4": (128, 192, 4),
                      "192x320_s2": (192, 320, 2), "256x448_s1": (256, 448, 1)},
             "base": {"64x64": (64, 64, 9), "64x128_s6": (64, 128, 6), "128x192_s1": (128, 192, 1), "192x320_s1": (192, 320, 1)}}
# the node goldens' cases: name -> (frames, h, w, channels, multiplier, skip list); frames cain_restated.seeded_frames(n, h, w, c, 9)
NODE_CASES = {"m2": (3, 64, 64, 3, 2, None), "skip": (4, 64, 64, 3, 2, [1]), "rgba": (2, 64, 64, 4, 2, None), "odd": (2, 100, 180, 3, 2, None)}
MODELS = {"lite": R, "base": B}
CKPT = {"lite": "atm-vfi-lite.pt", "base": B.CKPT}
GOLDEN_PREFIX = {"lite": "atm_ens", "base": "atm_base_ens"}      # + "_net.npz" / "_node.npz"


def config_with(atm_ensemble, atm_base=False):
    """a stand-in for ckpt.load_config: the package's own config with the two ATM keys set"""
    from cfi_amd import ckpt

    real = ckpt.load_config

    def load_config():
        return dict(real(), atm_ensemble=atm_ensemble, atm_base=atm_base)

    return load_config


_SD = {}


def state_dict_as(variant, dtype):
    """the seeded checkpoint of a model, drawn once per dtype and shared (read-only)"""
    if variant == "base":
        return B.state_dict_as(dtype)
    if dtype not in _SD:
        _SD[dtype] = R.state_dict_as(dtype)
    return _SD[dtype]


def frames_of(variant, case):
    """the two frames of a forward golden, [1,3,h,w] each"""
    import cain_restated

    h, w, fseed = NET_CASES[variant][case]
    f = cain_restated.seeded_frames(2, h, w, 3, fseed).permute(0, 3, 1, 2).contiguous()
    return f[0:1], f[1:2]


def padded(n):
    return math.ceil(n / WIN) * WIN


def mask_level(maps):
    """maps: the (h, w) of the three global maps -> per level the level whose pad regions its shifted block is masked with"""
    m = [0, 0, 0]
    for k in (1, 2):
        same = (padded(maps[k][0]), padded(maps[k][1])) == (padded(maps[k - 1][0]), padded(maps[k - 1][1]))
        m[k] = m[k - 1] if same else k
    return m


@contextlib.contextmanager
def labels_of(hw):
    """inside: atm_restated.window_attention takes its pad labels from an hw = (h, w) map centred in the padded layout (None: its own)"""
    real = R.region_labels
    if hw is not None:
        R.region_labels = lambda hp, wp, h, w, win, shift: real(hp, wp, hw[0], hw[1], win, shift)
    try:
        yield
    finally:
        R.region_labels = real


def features(sd, x):
    feats = []
    for i in range(4):
        x = R.conv_prelu(sd, f"feat_extracts.{i}.1", R.conv_prelu(sd, f"feat_extracts.{i}.0", x, 1 if i == 0 else 2))
        feats.append(x)
    return feats


def global_tokens(sd, feats):
    g = R.conv_prelu(sd, "last_feat_extract.1", R.conv_prelu(sd, "last_feat_extract.0", feats[3], 2))
    return R.fusion(sd, "global_feature_fusion", feats[2], feats[3], g)


def global_branch(M, sd, im, label_hw, head):
    """estimate_global_motion on the frame pair im [2,3,H,W] -> the 5 motion channels [1,5,H/16,W/16]"""
    gtok, mots = global_tokens(sd, features(sd, im)), []
    for k in range(2):
        with labels_of(label_hw if k else None):
            gtok, mot = M.window_block(R.sub(sd, f"global_motion_atmformer.{k}."), gtok, WIN, 6 * k, True)
        mots.append(mot)
    return head(sd, "global_motion_mlp", gtok, mots)


def resize_flow(flow, factor):
    return flow if factor == 1 else F.interpolate(flow, scale_factor=factor, mode="bilinear", align_corners=True) * factor


def alignment_loss(out, im0, im1):
    """global_alignmentness (:540-554): mean |warp(im0, flow0) - warp(im1, flow1)| over [3,H,W], flows at full resolution"""
    f = im0.shape[2] // out.shape[2]
    return (R.warp(im0, resize_flow(out[:, 0:2], f)) - R.warp(im1, resize_flow(out[:, 2:4], f))).abs().mean()


def select(losses):
    """min() and the == chain of :586-595: ties go to the lower level"""
    return 0 if losses[0] == min(losses) else 1 if losses[1] == min(losses) else 2


def ensemble_forward(variant, sd, im0, im1, taps=None):
    """Network.forward_global_ensemble on padded frames [1,3,H,W] (H, W multiples of 64) -> I_t [1,3,H,W], clamped.  taps (a dict):
    "losses" (three floats), "level", "maps" and the final flows."""
    M = MODELS[variant]
    head = R.motion_head
    maps = [(im0.shape[2] >> (4 + k), im0.shape[3] >> (4 + k)) for k in range(3)]
    ml = mask_level(maps)
    rec = {}

    def ensemble_head(sd_, name, tok, mots):
        out0 = head(sd_, name, tok, mots)
        if name != "global_motion_mlp":
            return out0
        outs, im = [out0], torch.cat([im0, im1])
        for k in (1, 2):
            im = R.half(im)
            outs.append(global_branch(M, sd, im, maps[ml[k]], head))
        assert [tuple(o.shape[2:]) for o in outs] == maps
        losses = [alignment_loss(o, im0, im1) for o in outs]
        level = select(losses)
        rec.update(losses=[float(l) for l in losses], level=level, maps=maps)
        return torch.cat([resize_flow(outs[level][:, 0:4], 1 << level), out0[:, 4:5]], 1)

    R.motion_head = ensemble_head
    try:
        out = M.atm_forward(sd, im0, im1, True, taps=taps)
    finally:
        R.motion_head = head
    if taps is not None:
        taps.update(rec)
    return out


def ensemble_frame(variant, sd, f0, f1, taps=None):
    """One model call of the node: frames [1,3,H,W] -> clamp(unpad(model(pad(f0), pad(f1)))) [1,3,H,W]"""
    H, W = f0.shape[2:]
    t, b, l, r = R.pad64(H, W)
    a, c = F.pad(f0, (l, r, t, b), mode="replicate"), F.pad(f1, (l, r, t, b), mode="replicate")
    return ensemble_forward(variant, sd, a, c, taps)[:, :, t:t + H, l:l + W].clamp(0, 1)


_RUNS = {}


def restated(variant, case, dtype=torch.float32):
    """(frame [h,w,3], taps) of a golden case through the restatement, computed once per dtype and shared (read-only); in float32 taps["on_diff"]
    is the largest difference to the "On" forward of the same frames"""
    key = (variant, case, dtype)
    if key not in _RUNS:
        f0, f1 = frames_of(variant, case)
        taps = {}
        with torch.no_grad():
            out = ensemble_forward(variant, state_dict_as(variant, dtype), f0.to(dtype), f1.to(dtype), taps)
            if dtype == torch.float32:
                taps["on_diff"] = float((out - MODELS[variant].atm_forward(state_dict_as(variant, dtype), f0, f1, True)).abs().max())
        _RUNS[key] = (out[0].permute(1, 2, 0).contiguous(), taps)
    return _RUNS[key]


class RestatedEnsemble:
    """AtmEngine.forward on the CPU for the ensemble mode: the restated model, one call per new frame (test infrastructure only)."""

    def __init__(self, variant):
        self.variant, self.sd, self.device, self.calls = variant, state_dict_as(variant, torch.float32), torch.device("cpu"), 0

    def forward(self, frame0, frame1, global_motion=True):
        from cfi_amd import atm

        assert global_motion == atm.ENSEMBLE and global_motion is not True, global_motion
        self.calls += 1
        one = lambda f: f[..., :3].permute(2, 0, 1)[None].contiguous()      # noqa: E731
        with torch.no_grad():
            return ensemble_frame(self.variant, self.sd, one(frame0), one(frame1))[0].permute(1, 2, 0)

    def release_workspace(self):
        pass

    def workspace_bytes(self):
        return 0


def run_node(variant, case, monkeypatch, engine):
    """The node's vfi() on a case of NODE_CASES in the ensemble mode, with the atm_ensemble key on (and atm_base for base), the checkpoint
    lookup and the engine replaced"""
    import cain_restated
    import cfi_amd
    from cfi_amd import atm, ckpt
    from cfi_amd.schedule import InterpolationStateList

    n, h, w, c, m, skip = NODE_CASES[case]
    monkeypatch.setattr(ckpt, "load_config", config_with(True, variant == "base"))
    monkeypatch.setattr(atm, "load_file_from_github_release", lambda model_type, name: name)
    monkeypatch.setattr(atm, "cached_engine", lambda model_type, path, build: (engine, True))
    if engine.device.type == "cpu":
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    frames = cain_restated.seeded_frames(n, h, w, c, 9)
    states = InterpolationStateList(skip, True) if skip else None
    return cfi_amd.ATM_VFI().vfi(CKPT[variant], frames, 10, m, ENSEMBLE, states)[0]
