"""MI355X-native drop-in for the RIFE / FILM / M2M / IFRNet nodes of ComfyUI-Frame-Interpolation.

ComfyUI imports this directory as a custom-node package and reads
``NODE_CLASS_MAPPINGS`` (reference: /root/reference/__init__.py:24-48).  The node
classes are imported lazily so that tooling which only needs the checkpoint spec or the
scheduler does not require the HIP library to be built.
"""

_LAZY = {
    "RIFE_VFI": ("rife", "RIFE_VFI"),
    "FILM_VFI": ("film", "FILM_VFI"),
    "M2M_VFI": ("m2m", "M2M_VFI"),
    "IFRNet_VFI": ("ifrnet", "IFRNet_VFI"),
    "GMFSS_Fortuna_VFI": ("gmfss", "GMFSS_Fortuna_VFI"),
    "IFUnet_VFI": ("ifunet", "IFUnet_VFI"),
    "CAIN_VFI": ("cain", "CAIN_VFI"),
    "SepconvVFI": ("sepconv", "SepconvVFI"),
    "FLAVR_VFI": ("flavr", "FLAVR_VFI"),
    "AMT_VFI": ("amt", "AMT_VFI"),
    "ATM_VFI": ("atm", "ATM_VFI"),
    "XVFI": ("xvfi", "XVFI"),
    "MakeInterpolationStateList": ("schedule", "MakeInterpolationStateList"),
    "InterpolationStateList": ("schedule", "InterpolationStateList"),
}


def __getattr__(name):
    if name in _LAZY:
        import importlib

        mod, attr = _LAZY[name]
        return getattr(importlib.import_module(f"{__name__}.{mod}"), attr)
    if name == "NODE_CLASS_MAPPINGS":
        return _node_class_mappings()
    if name == "NODE_DISPLAY_NAME_MAPPINGS":
        return dict(_DISPLAY_NAMES, **dict(EXTRA_NODES[n] for n in extra_nodes()))
    raise AttributeError(name)


def _node_class_mappings():
    from .film import FILM_VFI
    from .gmfss import GMFSS_Fortuna_VFI
    from .ifunet import IFUnet_VFI
    from .ifrnet import IFRNet_VFI
    from .m2m import M2M_VFI
    from .rife import RIFE_VFI
    from .schedule import MakeInterpolationStateList

    extra = {}
    if "cain" in extra_nodes():
        from .cain import CAIN_VFI

        extra["CAIN VFI"] = CAIN_VFI
    if "sepconv" in extra_nodes():
        from .sepconv import SepconvVFI

        extra["Sepconv VFI"] = SepconvVFI
    if "flavr_vfi" in extra_nodes():
        from .flavr import FLAVR_VFI

        extra["FLAVR VFI"] = FLAVR_VFI
    if "amt_vfi" in extra_nodes():
        from .amt import AMT_VFI

        extra["AMT VFI"] = AMT_VFI
    if "atm_vfi" in extra_nodes():
        from .atm import ATM_VFI

        extra["ATM VFI"] = ATM_VFI
    if "xvfi" in extra_nodes():
        from .xvfi import XVFI

        extra["XVFI VFI"] = XVFI
    return {
        "RIFE VFI": RIFE_VFI,
        "FILM VFI": FILM_VFI,
        "M2M VFI": M2M_VFI,
        "IFRNet VFI": IFRNet_VFI,
        "GMFSS Fortuna VFI": GMFSS_Fortuna_VFI,
        "IFUnet VFI": IFUnet_VFI,
        "Make Interpolation State List": MakeInterpolationStateList,
        **extra,
    }


# Nodes registered only on request (their real checkpoints have not been run yet): config.yaml's `extra_nodes`, a comma-separated
# list such as "cain, sepconv".  (No environment variable: the package's set of variables is kept small, _lib.SUPPORTED_ENV.)
# FLAVR's, AMT's and ATM's keys are the reference's class names lower-cased, "flavr_vfi" / "amt_vfi" / "atm_vfi"; a bare "flavr", "amt" or
# "atm" is not a key.  ATM VFI serves atm-vfi-lite.pt (ATM-lite) with global motion "On" or "Off (fastest)", and atm-vfi-base.pt /
# atm-vfi-base-pct.pt (ATM-base) only when config.yaml's atm_base key is on as well (atm_spec.atm_base_enabled).  Frames beyond 1088x1920
# (lite) / 1472x2560 (base), up to 2160x3840 with both, only when its atm_large_frames key is on (atm_spec.atm_large_frames_enabled).
# FLAVR VFI serves frames beyond 1088x1920, up to 2160x3840, only when config.yaml's flavr_large_frames key is on (flavr.large_frames_enabled).
# Sepconv VFI serves frames beyond 4 194 303 pixels, up to 2160x3840, only when config.yaml's sepconv_large_frames key is on (sepconv.large_frames_enabled).
# AMT VFI serves amt-g.pth (AMT-G) only when config.yaml's amt_g key is on as well (amt_spec.amt_g_enabled), and AMT-G frames beyond
# 6 100 805 padded pixels, up to 2160x3840, only when its amt_large_frames key is on (amt.large_frames_enabled).
# XVFI's key is "xvfi" (the reference's class is XVFI; upstream never registered it, so the node's name "XVFI VFI" follows the other nodes').
EXTRA_NODES = {"cain": ("CAIN VFI", "CAIN VFI (MI355X HIP)"), "sepconv": ("Sepconv VFI", "Sepconv VFI (MI355X HIP)"),
               "flavr_vfi": ("FLAVR VFI", "FLAVR VFI (MI355X HIP)"), "amt_vfi": ("AMT VFI", "AMT VFI (MI355X HIP)"),
               "atm_vfi": ("ATM VFI", "ATM VFI (MI355X HIP)"), "xvfi": ("XVFI VFI", "XVFI VFI (MI355X HIP)")}


def extra_nodes():
    from .ckpt import load_config

    spec = str(load_config().get("extra_nodes", "") or "")
    names = [s.strip().lower() for s in spec.split(",") if s.strip()]
    unknown = [n for n in names if n not in EXTRA_NODES]
    if unknown:
        raise ValueError(f"extra_nodes / VFI_EXTRA_NODES: unknown node(s) {unknown}; known: {sorted(EXTRA_NODES)}")
    return names


_DISPLAY_NAMES = {
    "RIFE VFI": "RIFE VFI (MI355X HIP; rife47 / rife49)",
    "FILM VFI": "FILM VFI (MI355X HIP)",
    "M2M VFI": "M2M VFI (MI355X HIP)",
    "IFRNet VFI": "IFRNet VFI (MI355X HIP)",
    "GMFSS Fortuna VFI": "GMFSS Fortuna VFI (MI355X HIP)",
    "IFUnet VFI": "IFUnet VFI (MI355X HIP)",
}
