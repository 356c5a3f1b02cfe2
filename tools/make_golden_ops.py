"""Writes tests/golden/ref_ops_golden.npz: the reference's own kernel text for sepconv_out, kernel_AdaCoF_updateOutput and
kernel_dt, executed on the host on seeded inputs, for tests/test_gpu_ref_ops.py.

    python tools/make_golden_ops.py

Runs on a build host where the reference tree is present, never on the GPU machine: it imports the reference's
``vfi_models.ops`` (cupy backend) through oracle/ref_import.reference_ops(), whose CuPy stand-in (oracle/stubs/cupy) compiles
the kernel text that the reference's ``cuda_kernel`` specialises with g++ and runs it serially; both are used read-only.

The stand-in refuses kernels that use shared memory, so the correlation golden does NOT come from the reference's kernel text
but from ``correlation_restated`` below, a torch restatement checked against the reference's kernels line by line in its
docstring.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "ref_ops_golden.npz")


def correlation_restated(first, second):
    """The reference's _FunctionCorrelation.forward (vfi_models/ops/cupy_ops/correlation.py:232-296), restated:

    * kernel_Correlation_rearrange (:4-28) copies each input into rbot[n, y+4, x+4, c] of a [N, H+8, W+8, C] tensor created
      by ``new_zeros`` (:234-239): a zero border of 4 pixels, channels last.  Here: F.pad(second, (4, 4, 4, 4)), zeros.
    * kernel_Correlation_updateOutput (:30-102) runs one block per output pixel (blockIdx.x = x, blockIdx.y = y, blockIdx.z = n);
      x1 = x + 4, y1 = y + 4 is the pixel in padded coordinates (:43-44); the patch loop is 1x1 (:49-58), so patch_data is
      rbot0[n, y1, x1, :] = first[n, :, y, x].
    * for top_channel in 0..80 (:66): s2o = top_channel % 9 - 4 (x displacement), s2p = top_channel / 9 - 4 (y displacement)
      (:69-70); x2 = x1 + s2o, y2 = y1 + s2p (:76-77) index rbot1, i.e. second[n, :, y + s2p, x + s2o], zero outside the image.
    * sum over channels of patch_data[c] * rbot1[..., c] (:82), 32 interleaved partial sums reduced in lane order (:88-93),
      then / (float)SIZE_3(rbot0) = / C (:94-96), written to top[n, top_channel, y, x] (:95-96).
    Here: out[:, 9 * (dy + 4) + (dx + 4)] = (first * padded[:, :, 4+dy : 4+dy+H, 4+dx : 4+dx+W]).sum(1) / C, in float64 and
    rounded once (the reference's fp32 partial-sum order is not reproduced; the difference is rounding only)."""
    N, C, H, W = first.shape
    a, b = first.double(), torch.nn.functional.pad(second.double(), (4, 4, 4, 4))
    out = torch.empty(N, 81, H, W, dtype=torch.float64)
    for dy in range(-4, 5):
        for dx in range(-4, 5):
            out[:, 9 * (dy + 4) + (dx + 4)] = (a * b[:, :, 4 + dy:4 + dy + H, 4 + dx:4 + dx + W]).sum(1) / C
    return out.float()


def reference_batch_edt(img):
    """vfi_models/ops/cupy_ops/batch_edt.py:44-100 with the launch fixed as described in main()."""
    import importlib

    mod = importlib.import_module("vfi_models.ops.cupy_ops.batch_edt")
    from vfi_models.ops.cupy_ops import utils

    name, text = mod._batch_edt_kernel
    kernel = utils.cuda_launch(utils.cuda_kernel(name, text, {}))
    if len(img.shape) == 4:
        assert img.shape[1] == 1
        img = img.squeeze(1)
        expand = True
    else:
        expand = False
    bs, h, w = img.shape
    diam2 = h**2 + w**2
    block = 1024
    grid = (img.nelement() + block - 1) // block
    data = ((1 - img.type(torch.float32)) * diam2).contiguous()
    intermed = torch.zeros_like(data)
    kernel(grid=(grid, 1, 1), block=(block, 1, 1), args=[utils.cuda_int32(bs), utils.cuda_int32(h), utils.cuda_int32(w),
                                                         utils.cuda_float32(diam2), data.data_ptr(), intermed.data_ptr()])
    intermed = intermed.permute(0, 2, 1).contiguous()
    out = torch.zeros_like(intermed)
    kernel(grid=(grid, 1, 1), block=(block, 1, 1), args=[utils.cuda_int32(bs), utils.cuda_int32(w), utils.cuda_int32(h),
                                                         utils.cuda_float32(diam2), intermed.data_ptr(), out.data_ptr()])
    ans = out.permute(0, 2, 1).sqrt()
    if expand:
        ans = ans.unsqueeze(1)
    return ans


def main():
    from oracle import ref_import

    if not ref_import.available():
        raise SystemExit("make_golden_ops.py needs the reference tree (build host only)")
    ops = ref_import.reference_ops()
    g = torch.Generator().manual_seed(20261015)
    out = {}

    # sepconv: SepConv++'s 51 taps on a small image; taps normalised so that outputs are O(1)
    for name, (N, C, Ho, Wo, K) in {"sepconv_k51": (2, 4, 9, 13, 51), "sepconv_k5": (1, 3, 7, 11, 5)}.items():
        x = torch.rand(N, C, Ho + K - 1, Wo + K - 1, generator=g)
        ver = torch.rand(N, K, Ho, Wo, generator=g)
        hor = torch.rand(N, K, Ho, Wo, generator=g)
        ver, hor = ver / ver.sum(1, keepdim=True), hor / hor.sum(1, keepdim=True)
        y = ops.sepconv_func.apply(x, ver, hor)
        out.update({f"{name}_in": x, f"{name}_ver": ver, f"{name}_hor": hor, f"{name}_out": y})

    # AdaCoF at STMFNet's F = 5, dilation 1, offsets of both signs (truncation toward zero), some beyond the border
    for name, (N, C, Ho, Wo, F, d, amp) in {"adacof_f5": (2, 3, 12, 17, 5, 1, 3.0), "adacof_f3d2": (1, 3, 9, 10, 3, 2, 6.0)}.items():
        H, W = Ho + (F - 1) * d, Wo + (F - 1) * d
        x = torch.rand(N, C, H, W, generator=g)
        w = torch.rand(N, F * F, Ho, Wo, generator=g)
        w = w / w.sum(1, keepdim=True)
        oi = (torch.rand(N, F * F, Ho, Wo, generator=g) * 2 - 1) * amp
        oj = (torch.rand(N, F * F, Ho, Wo, generator=g) * 2 - 1) * amp
        y = ops.FunctionAdaCoF.apply(x, w, oi, oj, d)
        out.update({f"{name}_in": x, f"{name}_w": w, f"{name}_oi": oi, f"{name}_oj": oj, f"{name}_out": y})

    # distance transform: binary masks.  (The reference's ops/__init__.py imports the NAME batch_edt from cupy_ops, where it is
    # the submodule cupy_ops/batch_edt.py — its cupy_ops/__init__.py does not re-export the function — hence the attribute.)
    # The reference's batch_edt itself cannot run: it calls cuda_launch(name, text), while its cupy_ops/utils.py:229 takes one
    # key (EISAI is disabled upstream).  reference_batch_edt below follows its lines with the launch through
    # cuda_launch(cuda_kernel(...)) — the kernel text is the reference's own, _batch_edt_kernel.
    # Cases: sparse dots, a line, one empty image, and a 4-D input.
    edt = reference_batch_edt
    m = (torch.rand(3, 23, 37, generator=g) > 0.97).float()
    m[1, :, 20] = 1.0
    m[2] = 0.0
    out["edt_mask3"], out["edt_mask3_out"] = m, edt(m)
    m4 = (torch.rand(2, 1, 16, 9, generator=g) > 0.9).float()
    out["edt_mask4"], out["edt_mask4_out"] = m4, edt(m4)

    # correlation: torch restatement (the stand-in refuses the reference's shared-memory kernel)
    for name, (N, C, H, W) in {"corr_c32": (2, 32, 11, 14), "corr_c196": (1, 196, 5, 7)}.items():
        a = torch.randn(N, C, H, W, generator=g)
        b = torch.randn(N, C, H, W, generator=g)
        out.update({f"{name}_a": a, f"{name}_b": b, f"{name}_out": correlation_restated(a, b)})

    np.savez_compressed(OUT, **{k: v.contiguous().numpy().astype(np.float32) for k, v in out.items()})
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
