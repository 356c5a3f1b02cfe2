"""-m gpu: RIFE's block transition 4 -> 2 fused into block 2's conv0.0 (csrc/rife_ops.hip: trans2_conv0a_kernel) against the two kernels it
replaces, bit for bit.

  1. Op level: the tap vfi_test_rife_trans2_conv0a (include/vfi_hip_test_rife.h) against vfi_test_rife_stage_trans (4 -> 2, the quad
     kernel) followed by vfi_conv3x3 (stride 2, slope 0.2, tile variant 62 = d2_m1n2_live4) on X permuted to NHWC on the host, on
     identical buffers: torch.equal on the new flow and on A0.  The fused kernel walks each accumulator through K in variant 62's order
     and restates the quad kernel's cell arithmetic statement for statement, so there is no tolerance; both reference kernels have
     float64 tests of their own (test_gpu_rife_stage.py, test_gpu_rife_live_k.py).
  2. Whole network: option fuse0a2 = 1 against 0, torch.equal, and against the oracle within the project's 1e-3 at the small sizes.
  3. Refusals: bad B, geometry or slope return an error and launch nothing.

Every buffer of (1) and (3) is a small_ops_restated.Buffers window between NaN guards; outputs start as NaN, so an unwritten element,
a stray write or a changed input fails the case."""
import ctypes as C

import pytest
import torch

import rife_stage_restated as rs
import small_ops_restated as so
from gpu_util import describe_diff, hptr, ptr

pytestmark = pytest.mark.gpu

LIVE4 = 62      # d2_m1n2_live4 in the common variant numbering: what conv0a_b2 runs
SLOPE = 0.2

# id, Hp, Wp, slot0, slot1, timesteps, flow family, T kind, gap behind a pack (floats)
CASES = [
    ("64x64-b1-a0", 64, 64, (0,), (1,), (0.3,), "a0", "pos", 0),                                      # 2 tiles, each touches a border
    ("64x192-b3-mixed", 64, 192, (2, 1, 2), (0, 1, 1), (0.0, 1.0, 0.3), "mixed", "noise", 8),         # task 1: slot0 == slot1; +-1e4 and +-1e30 flows
    ("128x320-b2-mixed", 128, 320, (0, 1), (1, 0), (0.25, 0.75), "mixed", "noise", 0),
    # 32 x 4 x 6 = 768 tiles: more than two per CU, so the persistent workgroups walk on to further tiles
    ("128x384-b32-rand", 128, 384, tuple(b % 4 for b in range(32)), tuple((b + 1 + b // 4) % 4 for b in range(32)), tuple(b / 31 for b in range(32)), "rand", "noise", 8),
]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _weights(seed):
    """OIHW [48][20][3][3] with |w| in [0.5, 1] and random signs, bias N(0, 1)"""
    g = so._g(seed)
    w = so._pos(g, 48, 20, 3, 3) * torch.where(torch.rand(48, 20, 3, 3, generator=g) < 0.5, -1.0, 1.0)
    return w.contiguous(), so._noise(g, 48).contiguous()


def _inputs(case):
    cid, Hp, Wp, s0, s1, ts, flow, tkind, gap = case
    g = so._g(sum(cid.encode()) * 7919 + Hp * Wp)
    nb, n = len(s0), max(s0 + s1) + 1
    pk = so._make(g, "noise", n, 2, Hp, Wp, 4)
    pack = 2 * Hp * Wp * 4
    body = torch.full((n, pack + gap), rs.NAN)
    body[:, :pack] = pk.reshape(n, -1)
    T = rs.to_planar(rs.make_T(g, tkind, nb, Hp // 4, Wp // 4, 2)).reshape(-1, 4)
    Fin = rs.flows(g, nb, Hp, Wp, flow).reshape(-1, 4)
    return dict(P=body, stride=pack + gap, T=T, F=Fin, nb=nb)


def _task_args(B, inp, case, nb=None):
    _, _, _, s0, s1, ts, _, _, _ = case
    k = len(s0)
    return [B.ptr("P"), inp["stride"], (C.c_int * k)(*s0), (C.c_int * k)(*s1), (C.c_float * k)(*ts), k if nb is None else nb]


def _fused_buffers(inp, Hp, Wp):
    nb = inp["nb"]
    B = so.Buffers("cuda")
    B.add("P", inp["P"])
    B.add("T", inp["T"])
    B.add("F", inp["F"])                                              # Fin: role "in", must come back unchanged
    B.add("Fout", None, nb * Hp * Wp, 4, role="out")
    B.add("A0", None, nb * (Hp // 4) * (Wp // 4), 48, role="out")
    return B


def _fused_args(B, inp, case, w, bias, **change):
    Hp, Wp = case[1], case[2]
    a = _task_args(B, inp, case, change.get("nb")) + [B.ptr("T"), B.ptr("F"), B.ptr("Fout"), w.data_ptr(), bias.data_ptr(), B.ptr("A0"),
                                                     change.get("Hp", Hp), change.get("Wp", Wp), C.c_float(change.get("slope", SLOPE))]
    return a


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_fused_matches_stage_trans_then_conv(hip_lib, case):
    from cfi_amd import _lib

    cid, Hp, Wp = case[:3]
    Hs, Ws = Hp // 2, Wp // 2
    inp = _inputs(case)
    nb = inp["nb"]
    w, bias = _weights(Hp + Wp + nb)
    fn = _lib.test_tap("vfi_test_rife_trans2_conv0a")

    # ---- the pair it replaces: stage_trans (in place on F, X planar4 with 24 channels), then the stride-2 convolution on NHWC X
    R = so.Buffers("cuda")
    R.add("P", inp["P"])
    R.add("T", inp["T"])
    R.add("F", inp["F"], role="inout")
    R.add("X", None, nb * 6 * Hs * Ws, 4, role="out")
    _lib.check(hip_lib.vfi_test_rife_stage_trans(*(_task_args(R, inp, case) + [R.ptr("T"), R.ptr("F"), R.ptr("X"), Hp, Wp, 4, 2, 1, 24, 1]), _stream()),
               "vfi_test_rife_stage_trans")
    torch.cuda.synchronize()
    ref = R.finish()
    X = ref["X"].view(nb, 6, Hs, Ws, 4).permute(0, 2, 3, 1, 4).reshape(nb, Hs, Ws, 24)
    assert not torch.isnan(X).any() and bool((X[..., 20:] == 0).all())
    R2 = so.Buffers("cuda")
    R2.add("X", X[..., :20].reshape(-1, 20))
    R2.add("A0", None, nb * (Hp // 4) * (Wp // 4), 48, role="out")
    rc = hip_lib.vfi_conv3x3(C.c_void_p(R2.ptr("X")), hptr(w), hptr(bias), None, C.c_void_p(R2.ptr("A0")), nb, Hs, Ws, 20, 48, 2, 1, SLOPE, LIVE4, None)
    _lib.check(rc, "vfi_conv3x3")
    torch.cuda.synchronize()
    rec = (C.c_int32 * 8)()
    assert hip_lib.vfi_test_last_conv_launch(rec, 8) == 8 and list(rec)[:2] == [2, LIVE4], list(rec)
    A0_ref = R2.finish()["A0"]
    F_ref = ref["F"]
    assert not torch.isnan(F_ref).any() and not torch.isnan(A0_ref).any(), "the reference pair left NaN: the case cannot see an unwritten output"

    # ---- the fused kernel
    B = _fused_buffers(inp, Hp, Wp)
    _lib.check(fn(*_fused_args(B, inp, case, w, bias), _stream()), "vfi_test_rife_trans2_conv0a")
    torch.cuda.synchronize()
    got = B.finish()                    # guards intact, P / T / Fin unchanged
    for name, want in (("Fout", F_ref), ("A0", A0_ref)):
        nan = torch.isnan(got[name])
        assert not nan.any(), f"{cid}: {int(nan.sum())} elements of {name} unwritten (or NaN); first at {nan.nonzero()[0].tolist()}"
        assert torch.equal(got[name], want), describe_diff(got[name], want, f"{cid}: {name}, fused vs stage_trans + conv (variant 62)")


def test_wrapper_refuses_bad_arguments(hip_lib):
    """B = 0, B = 33, Hp not a multiple of 32, Wp not a multiple of 64, slope outside [0, 1]: an error code and a message, no launch — every
    buffer, guards and outputs alike, is bit-identical afterwards"""
    from cfi_amd import _lib

    case = CASES[1]
    inp = _inputs(case)
    w, bias = _weights(1)
    B = _fused_buffers(inp, case[1], case[2])
    before = {k: b.dev.clone() for k, b in B.b.items()}
    fn = _lib.test_tap("vfi_test_rife_trans2_conv0a")
    for what, change in (("B = 0", dict(nb=0)), ("B = 33", dict(nb=33)), ("Hp % 32", dict(Hp=48)), ("Hp % 32", dict(Hp=80)), ("Wp % 64", dict(Wp=96)),
                         ("Wp % 64", dict(Wp=160)), ("slope < 0", dict(slope=-0.1)), ("slope > 1", dict(slope=1.5))):
        rc = fn(*_fused_args(B, inp, case, w, bias, **change), _stream())
        assert rc == -2 and _lib.last_error(), f"{what}: returned {rc}"
    torch.cuda.synchronize()
    for k, b in B.b.items():
        assert torch.equal(b.dev.view(torch.int32), before[k].view(torch.int32)), f"{k} changed: a refused call launched"


def _set(lib, value):
    assert lib.vfi_test_set_option(b"fuse0a2", value) == 0


def _traced(lib, f):
    from cfi_amd import _lib

    lib.vfi_trace_reset()
    lib.vfi_trace_enable(1)
    try:
        out = f()
        torch.cuda.synchronize()
    finally:
        lib.vfi_trace_enable(0)
    rep = _lib.trace_report()
    lib.vfi_trace_reset()
    return out, rep


@pytest.mark.parametrize("h,w,bs", [(64, 64, 1),        # 2 tiles of the fused kernel, every one touches a border
                                    (70, 90, 2),        # padded to 128 x 128, cropped
                                    (270, 480, 3)])     # padded to 320 x 512: 240 tiles, partial frame; the flow ping-pongs F -> F2 -> F
def test_network_fused_matches_two_kernels(hip_lib, h, w, bs):
    from cfi_amd import synth
    from cfi_amd.rife import RifeEngine, run_tasks
    from oracle import rife_oracle

    torch.cuda.set_device(0)
    sd = synth.rife47_synth_state_dict(1234)
    eng = RifeEngine(sd, "4.7")
    try:
        frames = synth.smooth_frames(bs + 1, h, w, seed=h + bs, shift=3.0)
        tasks = [(p, 0.5 if p % 2 == 0 else 0.3) for p in range(bs)]
        run = lambda: run_tasks(eng, frames, tasks, batch_size=bs)
        fused, rep1 = _traced(hip_lib, run)
        try:
            _set(hip_lib, 0)
            pair, rep0 = _traced(hip_lib, run)
        finally:
            _set(hip_lib, 1)
        again = run()
    finally:
        _set(hip_lib, 1)
        eng.close()
    assert "stage_trans2" in rep1 and "conv0a_b2" not in rep1, f"the fused path did not run: {sorted(rep1)}"
    assert "stage_trans2" in rep0 and "conv0a_b2" in rep0, f"option 0 did not select the two kernels: {sorted(rep0)}"
    assert torch.equal(fused, again), "not deterministic / state left behind by the un-fused form"
    assert torch.equal(fused, pair), describe_diff(fused, pair, "fuse0a2 = 1 vs 0")
    if h <= 70:
        x = frames.permute(0, 3, 1, 2)
        with torch.inference_mode():
            want = torch.cat([rife_oracle.ifnet47_forward(sd, x[p:p + 1], x[p + 1:p + 2], torch.tensor([t]).view(1, 1, 1, 1)) for p, t in tasks])
        want = want.permute(0, 2, 3, 1).clamp(0, 1)
        assert (fused - want).abs().max().item() <= 1e-3, describe_diff(fused, want, "fused transition vs oracle")
