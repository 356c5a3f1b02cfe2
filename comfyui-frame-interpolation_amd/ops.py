"""The reference's custom-op interface (vfi_models/ops, ``ops/__init__.py:21``), name for name, on this package's HIP kernels.

With a two-line patch to the reference's ``vfi_models/ops/__init__.py`` ("Option B: ops backend") every upstream
node that imports ``vfi_models.ops`` runs its custom ops on gfx950:

    softsplat / softsplat_func / FunctionSoftsplat / ModuleSoftsplat   -> vfi_softsplat_sum (NHWC; permuted here)
    costvol_func                                                        -> vfi_costvol9x9    (NHWC; permuted here)
    sepconv_func                                                        -> vfi_sepconv
    FunctionAdaCoF                                                      -> vfi_adacof
    FunctionCorrelation / ModuleCorrelation / _FunctionCorrelation      -> vfi_correlation81
    batch_edt                                                           -> vfi_edt

The torch-side arithmetic of the reference's wrappers (softsplat's metric concatenation and normalisation, batch_edt's data
preparation) is kept as it is.  Every launch goes to ``torch.cuda.current_stream()`` of the operands' device.  Forward only:
``backward`` raises NotImplementedError.  There is no fallback: a CPU tensor, a dtype the kernel does not take or a missing
library raises.
"""
import ctypes as C
import math

import torch

from . import _lib

__all__ = ["softsplat", "ModuleSoftsplat", "FunctionSoftsplat", "softsplat_func", "costvol_func", "sepconv_func", "init",
           "batch_edt", "FunctionAdaCoF", "ModuleCorrelation", "FunctionCorrelation", "_FunctionCorrelation"]


def init():
    """Checks that a GPU is visible and that libvfi_hip.so loads (the reference's init() checks for an NVIDIA device)."""
    if not torch.cuda.is_available():
        raise RuntimeError("cfi_amd.ops: no GPU visible; the HIP ops backend needs an MI355X (gfx950)")
    _lib.load()


def _check(what, *tensors):
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: expected a tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise RuntimeError(f"{what}: tensors must be on the GPU, got one on {t.device}")
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: the HIP kernel takes float32 tensors, got {t.dtype}")
    dev = tensors[0].device
    for t in tensors[1:]:
        if t.device != dev:
            raise RuntimeError(f"{what}: tensors on {dev} and {t.device}")


def _strides(t):
    return (C.c_longlong * 4)(*t.stride())


def _call(name, dev, *args):
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(getattr(lib, name)(*args, stream), name)


def _no_backward(name):
    raise NotImplementedError(f"cfi_amd.ops.{name}: backward is not implemented (the HIP ops backend is forward-only, for inference)")


def _nchw_to_nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- softsplat (cupy_ops/softsplat.py) ------------------------------------------------------------------------------------------

class softsplat_func(torch.autograd.Function):
    """Summation splat of NCHW ``tenIn`` along ``tenFlow`` [N,2,H,W].  The kernel is the NHWC one of the M2M node
    (vfi_softsplat_sum); operands are permuted to NHWC and the result back to a contiguous NCHW tensor."""

    @staticmethod
    def forward(self, tenIn, tenFlow):
        _check("softsplat_func", tenIn, tenFlow)
        N, Cc, H, W = tenIn.shape
        if tuple(tenFlow.shape) != (N, 2, H, W):
            raise ValueError(f"softsplat_func: flow of shape {tuple(tenFlow.shape)} for input {tuple(tenIn.shape)}")
        src, flow = _nchw_to_nhwc(tenIn), _nchw_to_nhwc(tenFlow)
        out = torch.empty_like(src)
        _call("vfi_softsplat_sum", tenIn.device, src.data_ptr(), flow.data_ptr(), out.data_ptr(), N, H, W, Cc)
        return out.permute(0, 3, 1, 2).contiguous()

    @staticmethod
    def backward(self, tenOutgrad):
        _no_backward("softsplat_func")


def FunctionSoftsplat(tenInput, tenFlow, tenMetric, strType):
    assert tenMetric is None or tenMetric.shape[1] == 1
    assert strType in ["summation", "average", "linear", "softmax"]

    if strType == "average":
        tenInput = torch.cat([tenInput, tenInput.new_ones(tenInput.shape[0], 1, tenInput.shape[2], tenInput.shape[3])], 1)
    elif strType == "linear":
        tenInput = torch.cat([tenInput * tenMetric, tenMetric], 1)
    elif strType == "softmax":
        tenInput = torch.cat([tenInput * tenMetric.exp(), tenMetric.exp()], 1)

    tenOutput = softsplat_func.apply(tenInput, tenFlow)

    if strType != "summation":
        tenNormalize = tenOutput[:, -1:, :, :]
        tenNormalize[tenNormalize == 0.0] = 1.0
        tenOutput = tenOutput[:, :-1, :, :] / tenNormalize

    return tenOutput


class ModuleSoftsplat(torch.nn.Module):
    def __init__(self, strType):
        super().__init__()
        self.strType = strType

    def forward(self, tenInput, tenFlow, tenMetric):
        return FunctionSoftsplat(tenInput, tenFlow, tenMetric, self.strType)


def softsplat(tenIn: torch.Tensor, tenFlow: torch.Tensor, tenMetric: torch.Tensor, strMode: str):
    assert strMode.split("-")[0] in ["sum", "avg", "linear", "soft"]

    if strMode == "sum":
        assert tenMetric is None
    if strMode == "avg":
        assert tenMetric is None
    if strMode.split("-")[0] == "linear":
        assert tenMetric is not None
    if strMode.split("-")[0] == "soft":
        assert tenMetric is not None

    if strMode == "avg":
        tenIn = torch.cat([tenIn, tenIn.new_ones([tenIn.shape[0], 1, tenIn.shape[2], tenIn.shape[3]])], 1)
    elif strMode.split("-")[0] == "linear":
        tenIn = torch.cat([tenIn * tenMetric, tenMetric], 1)
    elif strMode.split("-")[0] == "soft":
        tenIn = torch.cat([tenIn * tenMetric.exp(), tenMetric.exp()], 1)

    tenOut = softsplat_func.apply(tenIn, tenFlow)

    if strMode.split("-")[0] in ["avg", "linear", "soft"]:
        tenNormalize = tenOut[:, -1:, :, :]

        if len(strMode.split("-")) == 1:
            tenNormalize = tenNormalize + 0.0000001
        elif strMode.split("-")[1] == "addeps":
            tenNormalize = tenNormalize + 0.0000001
        elif strMode.split("-")[1] == "zeroeps":
            tenNormalize[tenNormalize == 0.0] = 1.0
        elif strMode.split("-")[1] == "clipeps":
            tenNormalize = tenNormalize.clip(0.0000001, None)

        tenOut = tenOut[:, :-1, :, :] / tenNormalize

    return tenOut


# ---- costvol (cupy_ops/costvol.py) -------------------------------------------------------------------------------------------------

class costvol_func(torch.autograd.Function):
    """9x9 mean-L1 cost volume [N,81,H,W] of NCHW ``tenOne`` against ``tenTwo`` (cast to float32 like the reference's
    custom_fwd(cast_inputs=float32)).  The kernel is the NHWC one of the M2M node (vfi_costvol9x9), which takes C % 4 == 0."""

    @staticmethod
    def forward(self, tenOne, tenTwo):
        tenOne, tenTwo = tenOne.float(), tenTwo.float()
        _check("costvol_func", tenOne, tenTwo)
        N, Cc, H, W = tenOne.shape
        if tuple(tenTwo.shape) != (N, Cc, H, W):
            raise ValueError(f"costvol_func: shapes {tuple(tenOne.shape)} and {tuple(tenTwo.shape)} differ")
        if Cc % 4:
            raise ValueError(f"costvol_func: {Cc} channels; the HIP kernel takes a multiple of 4")
        one, two = _nchw_to_nhwc(tenOne), _nchw_to_nhwc(tenTwo)
        out = one.new_empty([N, H, W, 81])
        _call("vfi_costvol9x9", tenOne.device, one.data_ptr(), Cc, two.data_ptr(), Cc, 0, out.data_ptr(), N, H, W, Cc, 81, 0)
        return out.permute(0, 3, 1, 2).contiguous()

    @staticmethod
    def backward(self, tenOutgrad):
        _no_backward("costvol_func")


# ---- sepconv (cupy_ops/sepconv.py) -------------------------------------------------------------------------------------------------

class sepconv_func(torch.autograd.Function):
    """out[n,c,y,x] = sum_fy sum_fx tenIn[n,c,y+fy,x+fx] * tenVer[n,fy,y,x] * tenHor[n,fx,y,x]; operands cast to float32 and
    read through their strides."""

    @staticmethod
    def forward(self, tenIn, tenVer, tenHor):
        tenIn, tenVer, tenHor = tenIn.float(), tenVer.float(), tenHor.float()
        _check("sepconv_func", tenIn, tenVer, tenHor)
        tenOut = tenIn.new_empty([tenIn.shape[0], tenIn.shape[1], tenVer.shape[2] and tenHor.shape[2],
                                  tenVer.shape[3] and tenHor.shape[3]])
        N, Cc, Hin, Win = tenIn.shape
        K = tenVer.shape[1]
        Ho, Wo = tenOut.shape[2], tenOut.shape[3]
        if tenHor.shape[1] != K or tuple(tenVer.shape) != (N, K, Ho, Wo) or tuple(tenHor.shape) != (N, K, Ho, Wo):
            raise ValueError(f"sepconv_func: ver {tuple(tenVer.shape)} / hor {tuple(tenHor.shape)} for input {tuple(tenIn.shape)}")
        _call("vfi_sepconv", tenIn.device, tenIn.data_ptr(), _strides(tenIn), tenVer.data_ptr(), _strides(tenVer),
              tenHor.data_ptr(), _strides(tenHor), tenOut.data_ptr(), _strides(tenOut), N, Cc, Hin, Win, Ho, Wo, K)
        return tenOut

    @staticmethod
    def backward(self, tenOutgrad):
        _no_backward("sepconv_func")


# ---- AdaCoF (cupy_ops/adacof.py) ---------------------------------------------------------------------------------------------------

class FunctionAdaCoF(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, weight, offset_i, offset_j, dilation):
        _check("FunctionAdaCoF", input, weight, offset_i, offset_j)
        intSample = input.size(0)
        intInputDepth = input.size(1)
        intInputHeight = input.size(2)
        intInputWidth = input.size(3)
        intFilterSize = int(math.sqrt(weight.size(1)))
        intOutputHeight = weight.size(2)
        intOutputWidth = weight.size(3)

        assert intInputHeight - ((intFilterSize - 1) * dilation + 1) == intOutputHeight - 1
        assert intInputWidth - ((intFilterSize - 1) * dilation + 1) == intOutputWidth - 1

        assert input.is_contiguous() == True
        assert weight.is_contiguous() == True
        assert offset_i.is_contiguous() == True
        assert offset_j.is_contiguous() == True

        F2 = intFilterSize * intFilterSize
        want = (intSample, F2, intOutputHeight, intOutputWidth)
        if weight.size(1) != F2 or tuple(offset_i.shape) != want or tuple(offset_j.shape) != want or weight.size(0) != intSample:
            raise ValueError(f"FunctionAdaCoF: weight {tuple(weight.shape)} / offsets {tuple(offset_i.shape)}, "
                             f"{tuple(offset_j.shape)} for input {tuple(input.shape)}")

        output = input.new_empty(intSample, intInputDepth, intOutputHeight, intOutputWidth)
        _call("vfi_adacof", input.device, input.data_ptr(), weight.data_ptr(), offset_i.data_ptr(), offset_j.data_ptr(),
              output.data_ptr(), intSample, intInputDepth, intInputHeight, intInputWidth, intFilterSize, int(dilation),
              intOutputHeight, intOutputWidth)
        return output

    @staticmethod
    def backward(ctx, gradOutput):
        _no_backward("FunctionAdaCoF")


# ---- correlation (cupy_ops/correlation.py) -----------------------------------------------------------------------------------------

class _FunctionCorrelation(torch.autograd.Function):
    @staticmethod
    def forward(self, first, second):
        _check("FunctionCorrelation", first, second)
        if first.shape != second.shape or first.dim() != 4:
            raise ValueError(f"FunctionCorrelation: shapes {tuple(first.shape)} and {tuple(second.shape)}")
        N, Cc, H, W = first.shape
        output = first.new_empty([N, 81, H, W])
        _call("vfi_correlation81", first.device, first.data_ptr(), _strides(first), second.data_ptr(), _strides(second),
              output.data_ptr(), N, Cc, H, W)
        return output

    @staticmethod
    def backward(self, gradOutput):
        _no_backward("FunctionCorrelation")


def FunctionCorrelation(tenFirst, tenSecond):
    return _FunctionCorrelation.apply(tenFirst, tenSecond)


class ModuleCorrelation(torch.nn.Module):
    def __init__(self):
        super(ModuleCorrelation, self).__init__()

    def forward(self, tenFirst, tenSecond):
        return _FunctionCorrelation.apply(tenFirst, tenSecond)


# ---- distance transform (cupy_ops/batch_edt.py) ------------------------------------------------------------------------------------

def batch_edt(img, block=1024):
    """Euclidean distance to the nearest non-zero pixel of `img` (bs,h,w) or (bs,1,h,w); an empty image gives sqrt(h^2 + w^2).
    Like the reference's wrapper it takes a mask of any real dtype (data = (1 - img.float()) * diam2) and returns img's dtype.
    `block` (the reference's CUDA block size) is accepted and ignored."""
    if len(img.shape) == 4:
        assert img.shape[1] == 1
        img = img.squeeze(1)
        expand = True
    else:
        expand = False
    if not img.is_cuda:
        raise RuntimeError(f"batch_edt: tensors must be on the GPU, got one on {img.device}")
    if img.is_complex():
        raise TypeError(f"batch_edt: a real mask is expected, got {img.dtype}")
    bs, h, w = img.shape
    diam2 = h**2 + w**2
    odtype = img.dtype

    data = ((1 - img.type(torch.float32)) * diam2).contiguous()
    intermed = torch.empty_like(data)
    out = torch.empty_like(data)
    _call("vfi_edt", img.device, data.data_ptr(), intermed.data_ptr(), out.data_ptr(), bs, h, w, float(diam2))
    ans = out.type(odtype) if odtype != out.dtype else out

    if expand:
        ans = ans.unsqueeze(1)
    return ans
