"""CPU tests of the fused sparse Adam step (SparseGaussianAdam, _C.sparse_adam / _C.adamUpdate; include/stp_raster.h: stp_sparse_adam): the
class and what it refuses, the C ABI's declaration, export and argument validation (which runs before any launch, so without a GPU), the
loader's message for a library without the symbol, the float64 yardstick of the GPU tests on a hand-computed case, and the kernel's
row-index multiplier (csrc/stp_adam_div.h) against the integer division."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import torch_ref_sparse_adam as tra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class StpAdamTensor(ctypes.Structure):
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("numel", ctypes.c_longlong), ("lr", ctypes.c_float), ("eps", ctypes.c_float)]


def test_class_is_an_adam():
    import diff_gaussian_rasterization as dgr
    assert issubclass(dgr.SparseGaussianAdam, torch.optim.Adam) and "SparseGaussianAdam" in dgr.__all__
    ps = [torch.nn.Parameter(torch.zeros(5, 3)), torch.nn.Parameter(torch.zeros(5, 1))]
    opt = dgr.SparseGaussianAdam([{"params": [ps[0]], "lr": 1e-3, "name": "xyz"}, {"params": [ps[1]], "lr": 2e-3, "name": "opacity"}], lr=0.0, eps=1e-15)
    assert [g["lr"] for g in opt.param_groups] == [1e-3, 2e-3] and all(g["eps"] == 1e-15 and g["betas"] == (0.9, 0.999) for g in opt.param_groups)
    assert [g["name"] for g in opt.param_groups] == ["xyz", "opacity"]
    assert len(opt.state) == 0   # (created by the first step, for tensors with a gradient)
    opt.step(torch.ones(5, dtype=torch.bool), 5)   # no gradient anywhere: nothing to do, nothing created, no library call
    assert len(opt.state) == 0 and opt.last_launches == 0
    assert set(opt.state_dict()) == {"state", "param_groups"}


@pytest.mark.parametrize("option, value", [("weight_decay", 0.01), ("amsgrad", True), ("maximize", True), ("capturable", True), ("fused", True),
                                           ("foreach", True)])
def test_refusals_at_construction(option, value):
    import diff_gaussian_rasterization as dgr
    p = torch.nn.Parameter(torch.zeros(4, 3))
    with pytest.raises(ValueError, match=option):
        dgr.SparseGaussianAdam([p], lr=1e-3, eps=1e-15, **{option: value})
    with pytest.raises(ValueError, match=option):   # ... and as a group's option
        dgr.SparseGaussianAdam([{"params": [p], option: value}], lr=1e-3, eps=1e-15)
    dgr.SparseGaussianAdam([p], lr=1e-3, eps=1e-15, **{option: 0 if option == "weight_decay" else False})   # (switched off: fine)


def test_more_than_one_tensor_in_a_group_is_refused():
    import diff_gaussian_rasterization as dgr
    a, b = torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(4, 1))
    with pytest.raises(AssertionError, match="more than one tensor in group"):
        dgr.SparseGaussianAdam([a, b], lr=1e-3, eps=1e-15)
    opt = dgr.SparseGaussianAdam([{"params": [a]}, {"params": [b]}], lr=1e-3, eps=1e-15)
    opt.param_groups[0]["params"].append(torch.nn.Parameter(torch.zeros(4, 2)))   # (a group edited later is caught by the step)
    with pytest.raises(AssertionError, match="more than one tensor in group"):
        opt.step(torch.ones(4, dtype=torch.bool), 4)
    with pytest.raises(TypeError, match="nesterov"):
        dgr.SparseGaussianAdam([a], lr=1e-3, eps=1e-15, nesterov=True)


def test_cpu_tensors_have_no_path():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    p = torch.nn.Parameter(torch.zeros(4, 3))
    p.grad = torch.ones(4, 3)
    opt = dgr.SparseGaussianAdam([p], lr=1e-3, eps=1e-15)
    with pytest.raises(RuntimeError, match="no CPU path"):
        opt.step(torch.ones(4, dtype=torch.bool), 4)
    assert torch.equal(p.detach(), torch.zeros(4, 3))
    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.sparse_adam([z], [z.clone()], [z.clone()], [z.clone()], torch.ones(4, dtype=torch.int32), [1e-3], [1e-15], 0.9, 0.999, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.adamUpdate(z, z.clone(), z.clone(), z.clone(), torch.ones(4, dtype=torch.bool), 1e-3, 0.9, 0.999, 1e-15, 4, 3)


def test_header_declares_the_step():
    h = open(os.path.join(ROOT, "include", "stp_raster.h")).read()
    assert int(re.search(r"#define\s+STP_ABI_VERSION\s+(\d+)\b", h).group(1)) == 7
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"typedef\s+struct\s*\{\s*float\s*\*\s*param\s*;\s*const\s+float\s*\*\s*grad\s*;\s*float\s*\*\s*exp_avg\s*;\s*float\s*\*\s*exp_avg_sq\s*;"
                     r"\s*long\s+long\s+numel\s*;\s*float\s+lr\s*,\s*eps\s*;\s*\}\s*StpAdamTensor\s*;", h)
    assert re.search(r"int\s+stp_sparse_adam\s*\(\s*int\s+n_tensors\s*,\s*const\s+StpAdamTensor\s*\*\s*tensors\s*,\s*int\s+N\s*,\s*const\s+void\s*\*\s*visible\s*,"
                     r"\s*int\s+visible_kind\s*,\s*float\s+beta1\s*,\s*float\s+beta2\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)


def test_library_exports_the_step_and_the_abi_stays_7():
    from diff_gaussian_rasterization import _C
    L = _C._load()
    assert hasattr(L, "stp_sparse_adam") and _C._require("stp_sparse_adam") is not None
    assert L.stp_abi_version() == 7
    nm = subprocess.run(["nm", "-D", "--defined-only", _C.library_path()], capture_output=True, text=True).stdout
    assert re.search(r" T stp_sparse_adam$", nm, re.M)
    assert callable(_C._native().sparse_adam)


def test_loader_message_for_a_library_without_the_symbols(monkeypatch):
    from diff_gaussian_rasterization import _C
    monkeypatch.setattr(_C, "_lib", types.SimpleNamespace())   # a loaded library that predates the export
    with pytest.raises(RuntimeError) as ex:
        _C._require("stp_sparse_adam")
    assert str(ex.value) == f"{_C.library_path()} does not export stp_sparse_adam (a library built before the sparse Adam step): rebuild it"
    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="does not export stp_sparse_adam"):
        _C.sparse_adam([z], [z], [z], [z], torch.ones(4, dtype=torch.bool), [1e-3], [1e-15], 0.9, 0.999, 4)


def _call(L, tensors, N, visible, kind):
    arr = (StpAdamTensor * max(len(tensors), 1))(*tensors)
    return L.stp_sparse_adam(len(tensors), ctypes.cast(arr, ctypes.c_void_p), N, visible, kind, 0.9, 0.999, None)


def test_c_abi_validates_before_any_launch():
    """The refusals come before the first launch, so they need no GPU; the pointers are never followed (they are host addresses here)."""
    from diff_gaussian_rasterization import _C
    L = _C._load()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    good = StpAdamTensor(a, a, a, a, 12, 1e-3, 1e-15)
    err = lambda: L.stp_last_error().decode()
    assert _call(L, [StpAdamTensor(a, a, a, a, 10, 1e-3, 1e-15)], 3, a, 0) == -1   # STP_ERR_INVALID_ARGUMENT
    assert "tensor 0" in err() and "numel 10 is not a multiple of N = 3" in err()
    assert _call(L, [good, StpAdamTensor(a, a, a, a, 10, 1e-3, 1e-15)], 3, a, 1) == -1   # (the second tensor: the first is not updated either)
    assert "tensor 1" in err() and "not a multiple" in err()
    assert _call(L, [good], 3, a, 2) == -1
    assert "unknown visible_kind 2" in err()
    assert _call(L, [good], 3, a, -1) == -1 and "unknown visible_kind" in err()
    assert _call(L, [StpAdamTensor(a, None, a, a, 12, 1e-3, 1e-15)], 3, a, 0) == -1 and "null pointer" in err()
    assert _call(L, [good], 3, None, 0) == -1 and "null visible" in err()
    assert _call(L, [good], -3, a, 0) == -1 and "negative count" in err()
    assert L.stp_sparse_adam(-1, None, 3, a, 0, 0.9, 0.999, None) == -1 and "negative count" in err()
    assert _call(L, [StpAdamTensor(a, a, a, a, 1 << 31, 1e-3, 1e-15)], 1, a, 0) == -1 and ">= 2^31" in err()
    assert _call(L, [StpAdamTensor(a, a, a, a, -4, 1e-3, 1e-15)], 1, a, 0) == -1 and "negative numel" in err()
    assert _call(L, [good], 0, a, 0) == -1 and "not a multiple" in err()   # (elements, but no rows)
    # empty work: no launch, 0
    assert L.stp_sparse_adam(0, None, 5, a, 0, 0.9, 0.999, None) == 0
    assert _call(L, [StpAdamTensor(None, None, None, None, 0, 1e-3, 1e-15)], 0, None, 0) == 0
    assert _call(L, [StpAdamTensor(a, a, a, a, 0, 1e-3, 1e-15)] * 3, 7, a, 1) == 0


def test_yardstick_on_a_hand_computed_case():
    """Three Gaussians of one element: the first visible from a zero state, the second visible with state, the third invisible.  With
    b1 = 0.5, b2 = 0.75, lr = 0.25, eps = 0.5 (all exact in float32) every value below is exact in binary floating point."""
    p = np.array([[1.0], [2.0], [3.0]], np.float32)
    g = np.array([[2.0], [-4.0], [np.nan]], np.float32)
    m = np.array([[0.0], [2.0], [5.0]], np.float32)
    v = np.array([[0.0], [1.0], [6.0]], np.float32)
    pn, mn, vn = tra.step(p, g, m, v, np.array([True, True, False]), lr=0.25, eps=0.5, b1=0.5, b2=0.75)
    # row 0: m = 0.5 * 2 = 1, v = 0.25 * 4 = 1, p = 1 - 0.25 * 1 / (1 + 0.5) = 1 - 1/6
    # row 1: m = 0.5 * 2 + 0.5 * -4 = -1, v = 0.75 * 1 + 0.25 * 16 = 4.75, p = 2 + 0.25 / (sqrt(4.75) + 0.5)
    assert mn.tolist() == [[1.0], [-1.0], [5.0]] and vn.tolist() == [[1.0], [4.75], [6.0]]
    assert pn[0, 0] == 1.0 - 0.25 / 1.5 and pn[1, 0] == 2.0 + 0.25 / (np.sqrt(4.75) + 0.5) and pn[2, 0] == 3.0
    assert pn.dtype == np.float64
    # the int32 radii form: > 0 = visible
    pr, mr, vr = tra.step(p, g, m, v, np.array([3, 1, 0], np.int32), lr=0.25, eps=0.5, b1=0.5, b2=0.75)
    assert np.array_equal(pr, pn) and np.array_equal(mr, mn) and np.array_equal(vr, vn)
    p2, m2, v2 = tra.step(p, g, m, v, np.array([-1, 0, -7], np.int32), lr=0.25, eps=0.5)
    assert np.array_equal(p2, p) and np.array_equal(m2, m) and np.array_equal(v2, v)
    # the coefficients are rounded to float32 ONCE and 1 - b is formed from the rounded value
    b1 = float(np.float32(0.9))
    _, m3, _ = tra.step(p, g, m, v, np.array([True, True, True]), lr=1e-3, eps=1e-15)
    assert m3[1, 0] == b1 * 2.0 + (1.0 - b1) * -4.0 and m3[1, 0] != 0.9 * 2.0 + (1.0 - 0.9) * -4.0
    assert float(np.float32(1.0) - np.float32(0.9)) == 1.0 - b1   # (the float32 difference is exact: the yardstick's is the kernel's)
    # 0 / (0 + eps) is a step of exactly 0
    p4, m4, v4 = tra.step(p[:1], np.zeros((1, 1), np.float32), np.zeros((1, 1), np.float32), np.zeros((1, 1), np.float32), np.array([True]), lr=1e-3, eps=1e-15)
    assert p4[0, 0] == 1.0 and m4[0, 0] == 0.0 and v4[0, 0] == 0.0


def test_row_index_multiplier_is_the_integer_division(tmp_path):
    """The kernel forms e / M with a host-computed multiplier (csrc/stp_adam_div.h); tests/cpp/adam_div_check.cpp runs the same header on the
    host against e / M for M in 1..64 and e around every multiple of 2^16 up to 2^31 - 1."""
    exe = str(tmp_path / "adam_div_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "stopthepop-rasterization_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "adam_div_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"ok \d+\n", r.stdout) and int(r.stdout.split()[1]) > 64 * 32768 * 100
