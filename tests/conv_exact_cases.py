"""The case tables of tests/test_gpu_conv_exact.py (run on the GPU) and tests/test_conv_restated_cpu.py (certificates, no GPU).

A Job is one pytest case: one layer (fixed channels / kernel size / padding), a few calls of it at different sizes and epilogues, the
kernel form the calls must take — asserted through vfi_test_last_conv_launch — and other forms of the same call that must give the
same bits.  Sizes follow the tile of the variant under test: 1x1 pixel, exactly one tile, one tile + 1 in each direction on three
images (the tile decode across images), and 37x45 (ragged against 16x8, 16x16 and 32x16)."""
from dataclasses import dataclass, field, replace
from typing import Optional

from conv_restated import Case

GEN1, GEN2, WINO = 1, 2, 3
PLAIN, EXT, MASKED = 0, 1, 2

# id: (stride, taps, mt, nt, wm, wn, ck, grouped) — csrc/conv_mfma.hip kVariants, csrc/conv_mfma2.hip kVariants2 (+ 32).  Every entry is
# a (stride, taps, grouped) a layer object can issue.  tests/test_conv_restated_cpu.py compares this copy with the two source tables.
VARIANTS = {
    0: (1, 9, 2, 2, 4, 1, 16, 0), 1: (1, 9, 2, 3, 4, 1, 16, 0), 2: (1, 9, 1, 2, 4, 1, 16, 0), 3: (1, 9, 1, 3, 4, 1, 16, 0),
    4: (1, 9, 1, 1, 4, 1, 16, 0), 5: (1, 9, 2, 1, 4, 1, 16, 0), 6: (1, 9, 1, 1, 2, 2, 16, 0), 7: (1, 9, 2, 2, 2, 2, 16, 0),
    8: (2, 9, 1, 2, 4, 1, 8, 0), 9: (2, 9, 1, 3, 4, 1, 8, 0), 10: (2, 9, 1, 1, 4, 1, 8, 0), 11: (2, 9, 2, 2, 4, 1, 8, 0),
    12: (1, 4, 4, 1, 1, 4, 16, 1), 13: (1, 4, 2, 1, 1, 4, 16, 1),
    32: (1, 9, 2, 2, 4, 1, 8, 0), 33: (1, 9, 2, 3, 4, 1, 8, 0), 34: (1, 9, 1, 2, 4, 1, 8, 0), 35: (1, 9, 1, 3, 4, 1, 8, 0),
    36: (1, 9, 2, 2, 2, 2, 8, 0), 37: (1, 9, 4, 2, 2, 2, 8, 0), 38: (1, 9, 2, 2, 4, 1, 16, 0), 39: (2, 9, 1, 2, 4, 1, 8, 0),
    40: (2, 9, 2, 2, 4, 1, 8, 0), 41: (2, 9, 1, 3, 4, 1, 8, 0), 42: (2, 9, 2, 1, 4, 1, 8, 0), 43: (1, 4, 4, 1, 1, 4, 8, 1),
    44: (1, 4, 8, 1, 1, 4, 8, 1), 45: (1, 9, 2, 1, 4, 1, 8, 0), 46: (1, 4, 2, 2, 4, 1, 8, 0), 47: (1, 4, 1, 2, 4, 1, 8, 0),
    48: (1, 1, 2, 2, 4, 1, 8, 0), 49: (1, 1, 1, 2, 4, 1, 8, 0), 50: (1, 1, 2, 1, 4, 1, 8, 0), 51: (1, 4, 2, 1, 4, 1, 8, 0),
    52: (2, 4, 2, 1, 4, 1, 8, 0), 53: (2, 4, 1, 2, 4, 1, 8, 0), 54: (1, 9, 4, 2, 4, 1, 8, 0), 55: (1, 1, 1, 2, 4, 1, 32, 0),
    56: (1, 1, 2, 2, 2, 2, 32, 0), 57: (1, 4, 2, 2, 4, 1, 8, 0), 58: (1, 4, 1, 2, 4, 1, 8, 0), 59: (1, 4, 2, 2, 4, 1, 16, 0),
    60: (1, 4, 1, 2, 4, 1, 16, 0), 61: (1, 9, 1, 1, 4, 1, 8, 0),
}
MASKED_IDS = (57, 58, 59, 60)


def tile(vid):
    """(rows, columns) of the variant's output tile (grouped / masked: of one parity, i.e. in input pixels)."""
    _, _, mt, _, wm, _, _, _ = VARIANTS[vid]
    subs = wm * mt
    subx = (4 if subs >= 16 else 2 if subs >= 2 else 1) if vid >= 32 else (2 if subs >= 2 else 1)
    return subs // subx * 4, subx * 8


def n_tile(vid):
    _, _, _, nt, _, wn, _, grouped = VARIANTS[vid]
    return 32 if grouped else wn * nt * 32


def trace_name(c):
    """The trace name csrc/gen_ops.hip gives the call: what vfi_test_variant_override keys on."""
    if c.api == "up2":
        return "up2conv2x2"
    if c.api == "plain":
        return f"conv{c.k}x{c.k}"
    if c.kind == 1:
        return f"deconv4x4s2_{c.cphys}to{c.cout}"
    return f"conv{c.k}x{c.k}s{c.stride}_{c.cphys}to{c.cout}"


@dataclass
class Job:
    id: str
    cases: list                         # calls of ONE layer: they differ in size, batch, act / slope / residual / post affine only
    variant: Optional[int] = None       # forced through vfi_test_variant_override
    algo: int = 0                       # vfi_test_conv_algo
    opts: dict = field(default_factory=dict)
    expect: dict = field(default_factory=dict)      # family, variant, form, store, ks (int or ">1"), persistent
    same_bits: list = field(default_factory=list)   # other set-ups (dict: algo / opts / variant / expect) of the same calls: bit-equal


# ---- (a) every direct tile variant, plain and EXT ----------------------------------------------------------------------------------------
_CIN = {8: [8, 24, 40, 32], 16: [32, 16, 48], 32: [32, 64]}
_COUT = {32: [1, 9, 40, 96], 64: [40, 64, 128, 33], 96: [96, 70], 128: [128, 100]}
# EXT feature sets, cycled over the variants: (pad, act, slope, res, post)
_EXT = [(1, 1, 2.0, False, None), (2, 0, 0.0, True, None), (0, 3, 0.0, False, None), (0, 4, 0.0, False, (0.5, 3.0)), (0, 5, 0.0, False, None),
        (0, 3, 0.0, True, None), (0, 2, 0.0, False, (-2.0, 1.0))]


def _sizes(vid, pad):
    """Input sizes (n, h, w, odd) for a variant: per output tile (th, tw)."""
    st, taps, *_ = VARIANTS[vid]
    th, tw = tile(vid)
    outs = [(1, 1, 1), (1, th, tw), (3, th + 1, tw + 1), (1, 37, 45)]
    res = []
    for n, ho, wo in outs:
        if st == 1:
            h, w, odd = ho, wo, False
        elif taps == 9 and (ho, wo) != (th, tw):
            h, w, odd = 2 * ho - 1, 2 * wo - 1, True        # nn.Conv2d(3, 2, 1) on an odd size (vfi_conv_accept_odd)
        else:
            h, w, odd = 2 * ho, 2 * wo, False
        if pad == 2 and (h < 2 or w < 2):
            h, w = 2, 2                                       # ReflectionPad2d(1) needs two pixels
        res.append((n, h, w, odd))
    return res


def _variant_jobs():
    jobs = []
    e = 0
    for i, vid in enumerate(sorted(VARIANTS)):
        st, taps, mt, nt, wm, wn, ck, grouped = VARIANTS[vid]
        cphys = _CIN[ck][i % len(_CIN[ck])]
        cin = cphys - (3 if i % 2 else 0)
        cout = _COUT[n_tile(vid)][i % len(_COUT[n_tile(vid)])]
        fam = GEN2 if vid >= 32 else GEN1
        if vid in MASKED_IDS:      # nearest x2 + 2x2 'same' (vfi_conv_create_up2x2): act 0 / 1, all four parities, with and without chan_map
            for cm in (False, True):
                base = Case(api="up2", k=2, cin=cphys - 3, cphys=cphys, cout=64 if i % 2 else 128, cmap=cm)
                cs = [replace(base, n=n, h=h, w=w, act=j % 2, slope=0.25) for j, (n, h, w, _) in enumerate(_sizes(vid, 0))]
                jobs.append(Job(f"v{vid}-masked-{'cmap' if cm else 'id'}", cs, variant=vid, expect=dict(family=fam, variant=vid, form=MASKED, store=3, ks=1)))
            continue
        if grouped:                # ConvTranspose2d(4, 2, 1): the NHWC-2x interleaved store is EXT by itself; act 0 / 1 / 3
            base = Case(kind=1, k=4, stride=2, cin=cin, cphys=cphys, cout=cout, cmap=bool(i % 2), wino=True)
            cs = [replace(base, n=n, h=h, w=w, act=(0, 1, 3, 1)[j], slope=(0.0, 0.5, 0.0, -0.5)[j]) for j, (n, h, w, _) in enumerate(_sizes(vid, 0))]
            jobs.append(Job(f"v{vid}-grouped", cs, variant=vid, algo=1, expect=dict(family=fam, variant=vid, form=EXT, store=2, ks=1)))
            continue
        if taps == 4 and st == 1:  # FILM's 2x2 'same' layer (vfi_conv_create / vfi_conv_forward): no padding modes, slopes or post affine
            base = Case(api="plain", k=2, cin=cin, cphys=cphys, cout=cout, cmap=bool(i % 2))
            plain = [replace(base, n=n, h=h, w=w, act=j % 3, slope=2.0) for j, (n, h, w, _) in enumerate(_sizes(vid, 0))]
            ext = [replace(base, n=n, h=h, w=w, act=4 + j % 2) for j, (n, h, w, _) in enumerate(_sizes(vid, 0))]
        else:
            k = {9: 3, 4: 2, 1: 1}[taps]
            wino = taps == 9 and st == 1
            base = Case(k=k, stride=st, cin=cin, cphys=cphys, cout=cout, cmap=bool(i % 2), wino=wino)
            plain = [replace(base, n=n, h=h, w=w, odd=odd, act=j % 3, slope=(2.0, -0.5)[j % 2], res=j == 3)
                     for j, (n, h, w, odd) in enumerate(_sizes(vid, 0))]
            pad, act, slope, res, post = _EXT[e % len(_EXT)]
            if taps != 9 and pad:
                pad, act, slope = 1 if pad == 1 else 0, 3, 0.0       # reflect is 3x3 only; replicate elsewhere is legal and selects EXT
            e += 1
            eb = replace(base, pad=pad)
            ext = [replace(eb, n=n, h=h, w=w, odd=odd, act=act, slope=slope, res=res, post=post) for n, h, w, odd in _sizes(vid, pad)]
        algo = 1 if taps == 9 and st == 1 else 0
        jobs.append(Job(f"v{vid}-plain", plain, variant=vid, algo=algo, expect=dict(family=fam, variant=vid, form=PLAIN, store=0, ks=1)))
        jobs.append(Job(f"v{vid}-ext", ext, variant=vid, algo=algo, expect=dict(family=fam, variant=vid, form=EXT, store=0, ks=1)))
    return jobs


VARIANT_JOBS = _variant_jobs()

# a launch with so many tiles that the second-generation kernel runs persistent (grid.x < tiles: each workgroup walks several tiles, the
# DMA of the next tile's input in flight across the tile boundary).  The launcher goes persistent from 4 tiles per resident workgroup
# slot (csrc/conv_mfma2.hip: launch2_e): tiles x N blocks >= 4 x 256 CUs x occupancy.  2 x 272 x 480 -> 64 channels is 4080 workgroups
# of the 16x8x32 tile and stayed one workgroup per tile on the MI355X (the tap: grid.x 2040 = tiles; occupancy >= 4), so: 128 channels
# at 2 x 272 x 496 = 2108 tiles x 4 N blocks = 8432 >= 8192, persistent for any occupancy up to the hardware's 8 workgroups of 256
# threads per CU.  The first-generation launcher (launch_t) always starts one workgroup per tile: it has no persistent form to cover.
PERSISTENT_JOB = Job("persistent-v61", [Case(k=3, cin=8, cphys=8, cout=128, n=2, h=272, w=496, act=1, slope=0.25)], variant=61, algo=1,
                     expect=dict(family=GEN2, variant=61, form=PLAIN, store=0, ks=1, persistent=True))


# ---- (b) split-K: the epilogue runs in conv2_split_reduce_kernel -------------------------------------------------------------------------
# Sizes from the conditions in launch2_e on 256 CUs: one or two workgroups, and either TAPS * chunks >= 288 (long K) or >= 16 chunks
# with the chip 7/8 idle; ks <= chunks / 8 and <= TAPS * Cin_p / 576.  Cin_p = 264 / 584 / 1160 / 1184 give 33 / 73 / 145 / 37 chunks:
# ks = 4, 4, 2, 2 does not divide them, the last slice is shorter.  Cout = 40: lanes beyond Cout in the partial-sum launch.
def _epilogues(base, acts, h, w, odd=False):
    cs = []
    for act in acts:
        cs.append(replace(base, h=h, w=w, odd=odd, act=act, slope=2.0 if act == 1 else 0.0, res=act in (2, 3) and base.api == "ex" and base.kind == 0,
                          post=(0.5, 3.0) if act in (0, 4) and base.api == "ex" else None))
    return cs


def _split_jobs():
    jobs = []

    def add(name, base, h, w, variant, acts, odd=False):
        jobs.append(Job(f"split-{name}", _epilogues(base, acts, h, w, odd) + [replace(base, h=h, w=w, odd=odd, act=1, slope=-0.5)],
                        expect=dict(family=GEN2, variant=variant, ks=">1", store=0),
                        same_bits=[dict(opts={"splitk": 0}, expect=dict(family=GEN2, variant=variant, ks=1, store=0))]))

    for pad in (0, 1, 2):
        add(f"3x3s1-pad{pad}", Case(k=3, pad=pad, cin=261, cphys=264, cout=40, n=1), 8, 16, 61, (0, 1, 2, 3, 4, 5))
    for pad in (0, 1, 2):
        add(f"3x3s2-pad{pad}", Case(k=3, stride=2, pad=pad, cin=264, cphys=264, cout=40, n=1), 16, 32, 39, (0, 1, 2, 3, 4, 5))
        add(f"3x3s2-odd-pad{pad}", Case(k=3, stride=2, pad=pad, cin=264, cphys=264, cout=40, n=1), 15, 31, 39, (0, 3, 5), odd=True)
    add("2x2same", Case(api="plain", k=2, cin=580, cphys=584, cout=40, n=1), 8, 16, 47, (0, 1, 2, 4, 5))
    add("2x2s2", Case(k=2, stride=2, cin=584, cphys=584, cout=40, n=1), 16, 32, 53, (0, 1, 2, 3, 4, 5))
    add("1x1-k8", Case(k=1, cin=1155, cphys=1160, cout=40, n=1, cmap=True), 5, 7, 49, (0, 1, 2, 3, 4, 5))
    add("1x1-k32", Case(k=1, cin=1184, cphys=1184, cout=40, n=1), 5, 7, 55, (0, 1, 2, 3, 4, 5))
    return jobs


SPLIT_JOBS = _split_jobs()


# ---- (c) Winograd ------------------------------------------------------------------------------------------------------------------------
# epilogue MODE (csrc/conv_wino.hip: conv_wino_launch): 0 none / LeakyReLU with a slope in [0, 1]; 1 per-channel PReLU; 10 + act with a
# residual, a post affine, or an activation outside those two
_MODES = {0: dict(act=1, slope=0.25), 1: dict(act=3), 10: dict(act=0, res=True), 11: dict(act=1, slope=2.0), 12: dict(act=2, post=(-2.0, 1.0)),
          13: dict(act=3, res=True), 14: dict(act=4, post=(0.5, 3.0)), 15: dict(act=5, res=True)}
# region shape by the rule e16 > 1.15 e8 (covered-area efficiencies): 32x4 regions for 20x64, 12x96 and (partial regions) 19x62;
# 16x8 regions for 24x48 and (partial) 27x41
_WSHAPES = {16: [(1, 20, 64), (1, 12, 96), (3, 19, 62)], 8: [(1, 24, 48), (3, 27, 41)]}


def _wino_jobs():
    jobs = []
    i = 0
    for region in (8, 16):
        for mode, kw in _MODES.items():
            cphys = (8, 24, 32, 40)[i % 4]
            base = Case(k=3, pad=i % 3, cin=cphys - (3 if i % 2 else 0), cphys=cphys, cout=(9, 40, 96)[i % 3], cmap=bool(i % 2), wino=True, **kw)
            cs = [replace(base, n=n, h=h, w=w) for n, h, w in _WSHAPES[region]]
            jobs.append(Job(f"wino-r{region}-mode{mode}", cs, algo=2, expect=dict(family=WINO, variant=region, form=mode, store=0, ks=1),
                            same_bits=[dict(algo=1, expect=dict(store=0))]))
            i += 1
    # the transposed convolution as a 3x3 layer with 4 * Cout channels (SHUF 2), from 128 x 128 input pixels; against the grouped direct kernel
    for name, cphys, cm, kw, mode in (("act0", 8, False, dict(act=0), 0), ("lrelu", 16, True, dict(act=1, slope=0.5), 0), ("prelu", 16, False, dict(act=3), 1)):
        base = Case(kind=1, k=4, stride=2, cin=cphys - (2 if cm else 0), cphys=cphys, cout=24, cmap=cm, wino=True, **kw)
        cs = [replace(base, n=1, h=128, w=128), replace(base, n=1, h=131, w=133)]
        jobs.append(Job(f"wino-deconv-{name}", cs, expect=dict(family=WINO, variant=8, form=mode, store=2, ks=1),
                        same_bits=[dict(opts={"deconv_wino": 0}, expect=dict(form=EXT, store=2, variant=13 if cphys % 16 == 0 else 43))]))
    # FILM's 2x2 'same' layer with a long reduction, embedded in a 3x3 Winograd layer (vfi_conv_create: Cin_phys >= 1024)
    base = Case(api="plain", k=2, cin=1000, cphys=1024, cout=40, cmap=True, wino=True, act=1, slope=0.25)
    jobs.append(Job("wino-2x2-embedded", [replace(base, n=1, h=12, w=20), replace(base, n=2, h=27, w=41)], algo=2,
                    expect=dict(family=WINO, form=0, store=0, ks=1), same_bits=[dict(algo=1, expect=dict(family=GEN2, variant=47, ks=">1"))]))      # 128 chunks x 4 taps: the direct form splits K
    return jobs


WINO_JOBS = _wino_jobs()


# ---- (d) the default choice: one shape per return statement of conv_pick_variant (split_ok = 1) and per verdict of conv_wino_eligible ----
def _default_jobs():
    J = []

    def add(name, case, **expect):
        J.append(Job(f"default-{name}", [case], expect=expect))

    add("up2-k16", Case(api="up2", k=2, cin=16, cphys=16, cout=64, h=9, w=11), family=GEN2, variant=60, form=MASKED)
    add("up2-k8", Case(api="up2", k=2, cin=24, cphys=24, cout=64, h=9, w=11), family=GEN2, variant=58, form=MASKED)
    add("2x2s2-n64", Case(k=2, stride=2, cin=8, cphys=8, cout=64, h=18, w=22), family=GEN2, variant=53)
    add("2x2s2-n32", Case(k=2, stride=2, cin=8, cphys=8, cout=32, h=18, w=22), family=GEN2, variant=52)
    add("1x1-k32-wide", Case(k=1, cin=512, cphys=512, cout=128, h=9, w=11), family=GEN2, variant=56)
    add("1x1-k32", Case(k=1, cin=32, cphys=32, cout=64, h=9, w=11), family=GEN2, variant=55)
    add("2x2same-big", Case(api="plain", k=2, cin=8, cphys=8, cout=64, h=272, w=482), family=GEN2, variant=46)
    add("2x2same-small", Case(api="plain", k=2, cin=8, cphys=8, cout=64, h=9, w=11), family=GEN2, variant=47)
    add("1x1-big", Case(k=1, cin=8, cphys=8, cout=64, h=272, w=482), family=GEN2, variant=48)
    add("1x1-small", Case(k=1, cin=8, cphys=8, cout=64, h=9, w=11), family=GEN2, variant=49)
    add("2x2same-n32", Case(api="plain", k=2, cin=8, cphys=8, cout=32, h=9, w=11), family=GEN2, variant=51)
    add("1x1-n32", Case(k=1, cin=8, cphys=8, cout=32, h=9, w=11), family=GEN2, variant=50)
    add("deconv-k16", Case(kind=1, k=4, stride=2, cin=16, cphys=16, cout=24, h=9, w=11, wino=True), family=GEN1, variant=13, store=2)
    add("deconv-k8", Case(kind=1, k=4, stride=2, cin=24, cphys=24, cout=24, h=9, w=11, wino=True), family=GEN2, variant=43, store=2)
    add("3x3s2-n64", Case(k=3, stride=2, cin=8, cphys=8, cout=64, h=18, w=22), family=GEN2, variant=39)
    add("3x3s2-n96", Case(k=3, stride=2, cin=8, cphys=8, cout=96, h=18, w=22), family=GEN2, variant=41)
    add("3x3s2-n32", Case(k=3, stride=2, cin=8, cphys=8, cout=32, h=18, w=22), family=GEN1, variant=10)
    add("3x3-coarse", Case(k=3, cin=8, cphys=8, cout=64, h=17, w=30, wino=True), family=GEN2, variant=61)
    add("3x3-64", Case(k=3, cin=8, cphys=8, cout=64, h=80, w=80, wino=True), family=GEN2, variant=32)
    add("3x3-128", Case(k=3, cin=8, cphys=8, cout=128, h=80, w=80, wino=True), family=GEN2, variant=34)
    add("3x3-96-k16", Case(k=3, cin=16, cphys=16, cout=96, h=80, w=80, wino=True), family=GEN1, variant=4)
    add("3x3-96-k8", Case(k=3, cin=24, cphys=24, cout=96, h=80, w=80, wino=True), family=GEN2, variant=35)
    add("3x3-32-k16", Case(k=3, cin=16, cphys=16, cout=32, h=80, w=80, wino=True), family=GEN1, variant=4)
    add("3x3-32-k8", Case(k=3, cin=24, cphys=24, cout=32, h=80, w=80, wino=True), family=GEN2, variant=45)
    # conv_wino_eligible: 192 work items of a nominal two-image launch -> Winograd; 260 items = two rounds at 51 % -> direct (wino_quant)
    add("wino-yes", Case(k=3, cin=8, cphys=8, cout=128, h=96, w=128, wino=True), family=WINO, variant=8, form=0)
    add("wino-quantised-out", Case(k=3, cin=8, cphys=8, cout=128, h=104, w=160, wino=True), family=GEN2, variant=34)
    add("wino-too-few-items", Case(k=3, cin=8, cphys=8, cout=128, h=88, w=128, wino=True), family=GEN2, variant=34)
    return J


DEFAULT_JOBS = _default_jobs()

ALL_JOBS = VARIANT_JOBS + [PERSISTENT_JOB] + SPLIT_JOBS + WINO_JOBS + DEFAULT_JOBS
