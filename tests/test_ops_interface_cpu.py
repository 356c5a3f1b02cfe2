"""cfi_amd.ops is the reference's custom-op interface name for name (vfi_models/ops/__init__.py:21): the same exports and the
same call signatures, so a two-line patch to the reference's ops/__init__.py can import it instead of cupy_ops / taichi_ops.
No GPU needed: only names, signatures and the CPU-side errors are checked here (tests/test_gpu_ref_ops.py runs the kernels)."""
import ast
import inspect
import os
import re
import warnings

import pytest
import torch

from cfi_amd import ops

REF_OPS = "/root/reference/vfi_models/ops"
EXPORTS = ["softsplat", "ModuleSoftsplat", "FunctionSoftsplat", "softsplat_func", "costvol_func", "sepconv_func", "init",
           "batch_edt", "FunctionAdaCoF", "ModuleCorrelation", "FunctionCorrelation", "_FunctionCorrelation"]

# name -> (attribute whose signature is compared, parameter names) as the reference's cupy_ops declares them
SIGNATURES = {
    "softsplat": (None, ["tenIn", "tenFlow", "tenMetric", "strMode"]),
    "FunctionSoftsplat": (None, ["tenInput", "tenFlow", "tenMetric", "strType"]),
    "ModuleSoftsplat": ("__init__", ["self", "strType"]),
    "ModuleSoftsplat.forward": ("forward", ["self", "tenInput", "tenFlow", "tenMetric"]),
    "softsplat_func": ("forward", ["self", "tenIn", "tenFlow"]),
    "costvol_func": ("forward", ["self", "tenOne", "tenTwo"]),
    "sepconv_func": ("forward", ["self", "tenIn", "tenVer", "tenHor"]),
    "init": (None, []),
    "batch_edt": (None, ["img", "block"]),
    "FunctionAdaCoF": ("forward", ["ctx", "input", "weight", "offset_i", "offset_j", "dilation"]),
    "ModuleCorrelation": ("__init__", ["self"]),
    "ModuleCorrelation.forward": ("forward", ["self", "tenFirst", "tenSecond"]),
    "FunctionCorrelation": (None, ["tenFirst", "tenSecond"]),
    "_FunctionCorrelation": ("forward", ["self", "first", "second"]),
}


def _reference_present():
    return os.path.isfile(os.path.join(REF_OPS, "__init__.py"))


def _reference_exports():
    src = open(os.path.join(REF_OPS, "__init__.py")).read()
    m = re.search(r"from \.cupy_ops import ([^\n]+)", src)
    return [n.strip() for n in m.group(1).split(",")]


def _reference_signatures():
    """parameter names of every def / class method in the reference's cupy_ops sources (ast: nothing is imported or run)"""
    out = {}
    d = os.path.join(REF_OPS, "cupy_ops")
    for f in sorted(os.listdir(d)):
        if not f.endswith(".py"):
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")      # the reference's kernel strings carry escapes like '\('
            tree = ast.parse(open(os.path.join(d, f)).read())
        for node in tree.body:
            if isinstance(node, ast.FunctionDef):
                out[node.name] = [a.arg for a in node.args.args]
            elif isinstance(node, ast.ClassDef):
                for sub in node.body:
                    if isinstance(sub, ast.FunctionDef):
                        out[f"{node.name}.{sub.name}"] = [a.arg for a in sub.args.args]
    return out


def test_exports_match_the_reference_import_list():
    want = _reference_exports() if _reference_present() else EXPORTS
    assert want == EXPORTS
    assert sorted(ops.__all__) == sorted(want)
    for name in want:
        assert hasattr(ops, name), name


def _params(name):
    attr, _ = SIGNATURES[name]
    obj = getattr(ops, name.split(".")[0])
    if attr is not None:
        obj = getattr(obj, attr)
    return list(inspect.signature(obj).parameters)


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signatures_match_the_reference(name):
    got = _params(name)
    assert got == SIGNATURES[name][1], (name, got)
    if _reference_present():
        ref = _reference_signatures()
        attr = SIGNATURES[name][0]
        cls = name.split(".")[0]
        key = cls if attr is None else f"{cls}.{attr}"
        assert ref[key] == got, (name, ref[key], got)


def test_autograd_functions_are_autograd_functions():
    for name in ("softsplat_func", "costvol_func", "sepconv_func", "FunctionAdaCoF", "_FunctionCorrelation"):
        assert issubclass(getattr(ops, name), torch.autograd.Function), name
    assert issubclass(ops.ModuleSoftsplat, torch.nn.Module) and issubclass(ops.ModuleCorrelation, torch.nn.Module)


def test_cpu_tensors_raise():
    x = torch.zeros(1, 4, 64, 64)
    f = torch.zeros(1, 2, 64, 64)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.softsplat_func.apply(x, f)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.costvol_func.apply(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.sepconv_func.apply(torch.zeros(1, 4, 14, 14), torch.zeros(1, 51, 1, 1), torch.zeros(1, 51, 1, 1))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.FunctionCorrelation(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.FunctionAdaCoF.apply(torch.zeros(1, 3, 8, 8), torch.zeros(1, 25, 4, 4), torch.zeros(1, 25, 4, 4),
                                 torch.zeros(1, 25, 4, 4), 1)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.batch_edt(torch.zeros(1, 8, 8))


def test_init_without_a_gpu_raises():
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    with pytest.raises(RuntimeError, match="GPU"):
        ops.init()
