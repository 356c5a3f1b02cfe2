"""ORACLE — test infrastructure only: run the PREBUILT host builds of the reference's own CUDA kernel text
(oracle/_ref/*.so, made in the build container by oracle/build_ref.py from /root/reference/vfi_models/ops/cupy_ops via the
reference's own ``cuda_kernel`` specialiser) without needing /root/reference — so the GPU box can compare the HIP
kernels with an execution of the reference kernels.  Shapes are fixed at build time (the reference specialises per shape);
oracle/_ref/manifest.json lists them.  Launch geometry and zero-initialisation restate the reference's launch sites:
softsplat.py:201-224 (out = zeros; grid = ceil(nelement/512), block = 512; args n, in, flow, out) and costvol.py:139-179
(out = empty [N,81,H,W]; n = N*H*W)."""
import ctypes as C
import json
import os

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_ref")
_libs = {}


def manifest():
    p = os.path.join(_DIR, "manifest.json")
    if not os.path.exists(p):
        return {}
    with open(p) as f:
        return json.load(f)


def available():
    m = manifest()
    return bool(m) and all(os.path.exists(os.path.join(_DIR, v)) for v in m.values())


def shapes(op):
    return [tuple(int(x) for x in k.split("|")[1].split(",")) for k in manifest() if k.startswith(op + "|")]


def _launch(op, shape, n, ptrs):
    so = manifest()[op + "|" + ",".join(str(s) for s in shape)]
    if so not in _libs:
        _libs[so] = C.CDLL(os.path.join(_DIR, so))
    fn = getattr(_libs[so], op + "__host")
    fn.restype = None
    keep = [C.c_int(n)] + [C.c_void_p(p) for p in ptrs]
    arr = (C.c_void_p * len(keep))(*[C.cast(C.pointer(k), C.c_void_p) for k in keep])
    fn(C.c_int((n + 511) // 512), C.c_int(1), C.c_int(1), C.c_int(512), C.c_int(1), C.c_int(1), arr)


def softsplat_out(ten_in, ten_flow):
    a = np.ascontiguousarray(ten_in, np.float32)
    f = np.ascontiguousarray(ten_flow, np.float32)
    out = np.zeros_like(a)
    _launch("softsplat_out", a.shape, out.size, [a.ctypes.data, f.ctypes.data, out.ctypes.data])
    return out


def costvol_out(one, two):
    a = np.ascontiguousarray(one, np.float32)
    b = np.ascontiguousarray(two, np.float32)
    n, c, h, w = a.shape
    out = np.empty((n, 81, h, w), np.float32)
    _launch("costvol_out", a.shape, n * h * w, [a.ctypes.data, b.ctypes.data, out.ctypes.data])
    return out


# ---- stored digests: the prebuilt kernels' outputs on seeded inputs, so that the C oracle is pinned to them where oracle/_ref is absent
DIGESTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ref_kernels_digests.json")


def digest(arr):
    """SHA-256 of a float32 array's shape and bytes: equal digests <=> np.array_equal (bit for bit)."""
    import hashlib

    a = np.ascontiguousarray(arr, np.float32)
    return hashlib.sha256(repr(a.shape).encode() + a.tobytes()).hexdigest()


def seeded_cases(softsplat_shapes, costvol_shapes):
    """(op, shape, inputs) of tests/test_oracle_m2m_ops.py's comparison with the prebuilt kernels: one numpy generator (seed 5) drawn
    in this order — softsplat shapes with N*H*W <= 200000 (flow N(0, 9 px), one NaN source), costvol shapes with N*H*W <= 5000."""
    rng = np.random.default_rng(5)
    for shp in softsplat_shapes:
        if shp[0] * shp[2] * shp[3] > 200000:
            continue
        a = rng.random(shp, dtype=np.float32)
        f = (rng.standard_normal((shp[0], 2, shp[2], shp[3])) * 9).astype(np.float32)
        f[0, 0, 1, 1] = np.nan
        yield "softsplat_out", shp, (a, f)
    for shp in costvol_shapes:
        if shp[0] * shp[2] * shp[3] > 5000:
            continue
        yield "costvol_out", shp, (rng.standard_normal(shp).astype(np.float32), rng.standard_normal(shp).astype(np.float32))


def write_digests():
    """python oracle/ref_kernels.py — needs the prebuilt oracle/_ref (build() where the reference checkout exists)."""
    assert available(), "oracle/_ref is not built"
    ss, cv = shapes("softsplat_out"), shapes("costvol_out")
    cases = [[op, list(shp), digest(globals()[op](*inputs))] for op, shp, inputs in seeded_cases(ss, cv)]
    with open(DIGESTS, "w") as f:
        json.dump({"softsplat_out_shapes": [list(s) for s in ss], "costvol_out_shapes": [list(s) for s in cv], "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    write_digests()
