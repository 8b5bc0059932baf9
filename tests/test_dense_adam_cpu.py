"""CPU tests of the fused dense Adam step (GaussianAdam, _C.dense_adam; include/stp_raster.h: stp_dense_adam): the C ABI's declaration, struct
layout, export and argument validation (which runs before any launch, so without a GPU), the loader's message for a library without the symbol,
the class and what it refuses without a device, and the float64 yardstick of the GPU tests (tests/torch_ref_dense_adam.py) held against the thing
the kernel replaces: torch's own CPU float32 torch.optim.Adam with the two regularisers differentiated by autograd."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import torch_ref_dense_adam as trd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOATS = ("beta1", "one_minus_beta1", "beta2", "one_minus_beta2", "step_size", "bias2_sqrt", "eps")


class StpDenseAdamTensor(ctypes.Structure):
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("numel", ctypes.c_longlong)] + [(n, ctypes.c_float) for n in FLOATS] + [("reg_kind", ctypes.c_int32), ("reg_coef", ctypes.c_float)]


def entry(a, numel=12, reg_kind=0, bias2_sqrt=0.5, ptrs=None):
    p = ptrs if ptrs is not None else (a, a, a, a)
    return StpDenseAdamTensor(p[0], p[1], p[2], p[3], numel, 0.9, 0.1, 0.999, 0.001, 1e-3, bias2_sqrt, 1e-15, reg_kind, 0.0)


def test_header_declares_the_step_and_the_abi_stays_7():
    h = open(os.path.join(ROOT, "include", "stp_raster.h")).read()
    assert int(re.search(r"#define\s+STP_ABI_VERSION\s+(\d+)\b", h).group(1)) == 7
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"typedef\s+struct\s*\{\s*float\s*\*\s*param\s*;\s*const\s+float\s*\*\s*grad\s*;\s*float\s*\*\s*exp_avg\s*;\s*float\s*\*\s*exp_avg_sq\s*;"
                     r"\s*long\s+long\s+numel\s*;\s*float\s+beta1\s*,\s*one_minus_beta1\s*,\s*beta2\s*,\s*one_minus_beta2\s*,\s*step_size\s*,\s*bias2_sqrt\s*,"
                     r"\s*eps\s*;\s*int32_t\s+reg_kind\s*;\s*float\s+reg_coef\s*;\s*\}\s*StpDenseAdamTensor\s*;", h)
    assert re.search(r"int\s+stp_dense_adam\s*\(\s*int\s+n_tensors\s*,\s*const\s+StpDenseAdamTensor\s*\*\s*tensors\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)


def test_struct_layout_is_the_compilers(tmp_path):
    """The ctypes mirror the tests call through has the offsets the C compiler gives the header's struct."""
    names = [f[0] for f in StpDenseAdamTensor._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "stp_raster.h"\nint main(void) {\n'
                   + "".join(f'    printf("%zu ", offsetof(StpDenseAdamTensor, {n}));\n' for n in names)
                   + '    printf("%zu\\n", sizeof(StpDenseAdamTensor));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [getattr(StpDenseAdamTensor, n).offset for n in names] + [ctypes.sizeof(StpDenseAdamTensor)]
    assert got[-1] == 80 and got[4] == 32 and got[-3] == 68


def test_export_line_is_optional():
    text = open(os.path.join(ROOT, "stopthepop-rasterization_amd", "csrc", "host", "stp_exports.h")).read()
    assert re.search(r'^\s*X\(dense_adam,\s*false,\s*"the dense Adam step"\)', text, re.M)


def test_library_exports_the_step_and_the_abi_stays_7():
    from diff_gaussian_rasterization import _C
    L = _C._load()
    assert hasattr(L, "stp_dense_adam") and _C._require("stp_dense_adam") is not None
    assert L.stp_abi_version() == 7
    nm = subprocess.run(["nm", "-D", "--defined-only", _C.library_path()], capture_output=True, text=True).stdout
    assert re.search(r" T stp_dense_adam$", nm, re.M)
    assert callable(_C._native().dense_adam)


def test_loader_message_for_a_library_without_the_symbol(monkeypatch):
    from diff_gaussian_rasterization import _C
    monkeypatch.setattr(_C, "_lib", types.SimpleNamespace())   # a loaded library that predates the export
    with pytest.raises(RuntimeError) as ex:
        _C._require("stp_dense_adam")
    assert str(ex.value) == f"{_C.library_path()} does not export stp_dense_adam (a library built before the dense Adam step): rebuild it"
    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="does not export stp_dense_adam"):
        _C.dense_adam([z], [z], [z], [z], [_C.dense_adam_coefficients(1e-3, 0.9, 0.999, 1e-8, 1)], [0])


def _call(L, tensors):
    arr = (StpDenseAdamTensor * max(len(tensors), 1))(*tensors)
    return L.stp_dense_adam(len(tensors), ctypes.cast(arr, ctypes.c_void_p), None)


def test_c_abi_validates_before_any_launch():
    """The refusals come before the first launch, so they need no GPU; the pointers are never followed (they are host addresses here).  Every
    refused table but one begins with a good tensor: had it been launched, the call would have failed in another way (there is no device)."""
    from diff_gaussian_rasterization import _C
    L = _C._load()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    good = entry(a)
    err = lambda: L.stp_last_error().decode()
    assert _call(L, [good, entry(a, numel=-4)]) == -1 and "tensor 1" in err() and "negative numel" in err()   # STP_ERR_INVALID_ARGUMENT
    assert _call(L, [good, entry(a, numel=1 << 31)]) == -1 and "tensor 1" in err() and ">= 2^31" in err()
    for kind in (3, -1, 1 << 20):
        assert _call(L, [good, entry(a, reg_kind=kind)]) == -1 and f"unknown reg_kind {kind}" in err()
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        assert _call(L, [good, entry(a, bias2_sqrt=bad)]) == -1 and "tensor 1" in err() and "bias2_sqrt" in err()
    for k in range(4):
        ptrs = [a] * 4
        ptrs[k] = None
        assert _call(L, [good, entry(a, ptrs=ptrs)]) == -1 and "tensor 1" in err() and "null pointer" in err()
    assert _call(L, [entry(a, numel=-1)]) == -1 and "tensor 0" in err()
    assert L.stp_dense_adam(-1, None, None) == -1 and "negative count" in err()
    assert L.stp_dense_adam(2, None, None) == -1 and "null tensor table" in err()
    assert all(x == 0.0 for x in buf)   # (nothing was written through the good tensor's pointers)
    # empty work: no launch, 0 -- nothing of an entry without elements is looked at
    assert L.stp_dense_adam(0, None, None) == 0
    assert _call(L, [entry(None, numel=0, ptrs=(None,) * 4, bias2_sqrt=0.0, reg_kind=9)] * 3) == 0


def test_class_is_an_adam():
    import diff_gaussian_rasterization as dgr
    assert issubclass(dgr.GaussianAdam, torch.optim.Adam) and "GaussianAdam" in dgr.__all__
    ps = [torch.nn.Parameter(torch.zeros(5, 3)), torch.nn.Parameter(torch.zeros(5, 1)), torch.nn.Parameter(torch.zeros(5, 4))]
    opt = dgr.GaussianAdam([{"params": ps[:2], "lr": 1e-3, "name": "a"}, {"params": [ps[2]], "betas": (0.5, 0.75), "name": "opacity"}], lr=0.0, eps=1e-15)
    assert [g["lr"] for g in opt.param_groups] == [1e-3, 0.0] and all(g["eps"] == 1e-15 for g in opt.param_groups)
    assert [g["betas"] for g in opt.param_groups] == [(0.9, 0.999), (0.5, 0.75)]
    default = dgr.GaussianAdam([ps[0]])   # torch's signature and defaults
    assert default.defaults["lr"] == 1e-3 and default.defaults["betas"] == (0.9, 0.999) and default.defaults["eps"] == 1e-8
    assert len(opt.state) == 0   # (created by the first step, for tensors with a gradient)
    assert opt.step() is None and opt.step(lambda: 3.5) == 3.5   # no gradient anywhere: nothing to do, nothing created, no library call
    assert len(opt.state) == 0 and opt.last_launches == 0
    assert set(opt.state_dict()) == {"state", "param_groups"}
    # regularisers: a group key, read at every step
    opt.set_regularizer("opacity", "sigmoid", 0.01)
    assert opt.param_groups[1]["reg"] == ("sigmoid", 0.01) and opt.param_groups[0].get("reg") is None
    opt.set_regularizer("opacity", None)
    assert opt.param_groups[1]["reg"] is None
    with pytest.raises(ValueError, match="tanh"):
        opt.set_regularizer("opacity", "tanh", 0.01)
    assert opt.param_groups[1]["reg"] is None
    with pytest.raises(ValueError, match="nobody"):
        opt.set_regularizer("nobody", "exp", 0.01)
    opt.param_groups[0]["reg"] = ("cosh", 1.0)   # (a group edited by hand is caught by the step)
    with pytest.raises(ValueError, match="cosh"):
        opt.step()
    assert dgr.GaussianAdam([{"params": [ps[0]], "reg": ("exp", 0.01)}]).param_groups[0]["reg"] == ("exp", 0.01)
    with pytest.raises(ValueError, match="reg"):
        dgr.GaussianAdam([{"params": [ps[0]], "reg": "exp"}])


@pytest.mark.parametrize("option, value", [("weight_decay", 0.01), ("amsgrad", True), ("maximize", True), ("capturable", True), ("differentiable", True),
                                           ("fused", True), ("foreach", True)])
def test_refusals_at_construction(option, value):
    import diff_gaussian_rasterization as dgr
    p = torch.nn.Parameter(torch.zeros(4, 3))
    with pytest.raises(ValueError, match=option):
        dgr.GaussianAdam([p], lr=1e-3, eps=1e-15, **{option: value})
    with pytest.raises(ValueError, match=option):   # ... and as a group's option
        dgr.GaussianAdam([{"params": [p], option: value}], lr=1e-3, eps=1e-15)
    opt = dgr.GaussianAdam([p], lr=1e-3, eps=1e-15, **{option: 0 if option == "weight_decay" else False})   # (switched off: fine)
    opt.param_groups[0][option] = value   # (switched on later: caught by the step)
    with pytest.raises(ValueError, match=option):
        opt.step()


def test_tensor_lr_and_unknown_options_are_refused():
    import diff_gaussian_rasterization as dgr
    p = torch.nn.Parameter(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="tensor lr"):
        dgr.GaussianAdam([p], lr=torch.tensor(1e-3))
    with pytest.raises(ValueError, match="tensor lr"):
        dgr.GaussianAdam([{"params": [p], "lr": torch.tensor(1e-3)}], lr=1e-3)
    with pytest.raises(TypeError, match="nesterov"):
        dgr.GaussianAdam([p], nesterov=True)


def _no_change(opt, tensors, before):
    assert all(torch.equal(t, b) for t, b in zip(tensors, before)) and len(opt.state) == 0 and opt.last_launches == 0


def test_step_refusals_that_need_no_device():
    """Each names the tensor; a refused step updates nothing, creates no state and counts no step -- also for the good tensors before the bad one."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C

    def make(bad_param, bad_grad):
        good = torch.nn.Parameter(torch.ones(4, 3))
        good.grad = torch.ones(4, 3)
        bad = torch.nn.Parameter(bad_param)
        bad.grad = bad_grad
        return dgr.GaussianAdam([{"params": [good], "name": "xyz"}, {"params": [good.detach().clone().requires_grad_(), bad], "name": "second"}], lr=1e-3), good, bad

    opt, good, bad = make(torch.ones(4, 3), torch.ones(4, 3))
    with pytest.raises(RuntimeError, match=r"group 'xyz' tensor 0: param is on cpu: there is no CPU path"):
        opt.step()
    _no_change(opt, (good, bad), (torch.ones(4, 3), torch.ones(4, 3)))
    opt, good, bad = make(torch.ones(4, 3, dtype=torch.float64), torch.ones(4, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"group 'second' tensor 1: param: expected float32, got torch.float64"):
        opt.step()
    _no_change(opt, (good,), (torch.ones(4, 3),))
    opt, good, bad = make(torch.ones(4, 3), torch.ones(4, 3).to_sparse())
    with pytest.raises(RuntimeError, match=r"group 'second' tensor 1: sparse gradients are not supported"):
        opt.step()
    _no_change(opt, (good,), (torch.ones(4, 3),))
    opt, good, bad = make(torch.ones(3, 4).t(), torch.ones(4, 3))
    with pytest.raises(RuntimeError, match=r"group 'second' tensor 1: param must be contiguous"):
        opt.step()
    opt, good, bad = make(torch.ones(4, 3), torch.ones(4, 3))
    bad.grad = torch.ones(3, 4).t()
    with pytest.raises(RuntimeError, match=r"group 'second' tensor 1: grad must be contiguous"):
        opt.step()
    _no_change(opt, (good,), (torch.ones(4, 3),))
    # a state a trainer has put there itself (its surgery after a densification) is checked like the rest, and stays as it is
    opt, good, bad = make(torch.ones(4, 3), torch.ones(4, 3))
    opt.state[good] = {"step": torch.tensor(7.0), "exp_avg": torch.zeros(3, 4).t(), "exp_avg_sq": torch.zeros(4, 3)}
    with pytest.raises(RuntimeError, match=r"group 'xyz' tensor 0: exp_avg must be contiguous"):
        opt.step()
    assert float(opt.state[good]["step"]) == 7.0 and bad not in opt.state
    # the binding under the class refuses the same
    z = torch.zeros(4, 3)
    co = [_C.dense_adam_coefficients(1e-3, 0.9, 0.999, 1e-8, 1)]
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.dense_adam([z], [z.clone()], [z.clone()], [z.clone()], co, [0])
    with pytest.raises(RuntimeError, match="one entry per tensor"):
        _C.dense_adam([z], [z.clone()], [z.clone()], [z.clone()], co + co, [0])
    assert _C.dense_adam([], [], [], [], [], []) == 0


def test_coefficients_follow_torchs_convention():
    """Formed in float64 from the Python values and rounded once: 1 - beta2 is NOT the float32 difference from the rounded beta2."""
    from diff_gaussian_rasterization import _C
    c = _C.dense_adam_coefficients(1.6e-4, 0.9, 0.999, 1e-15, 10, 0.01, 1031)
    assert c == (0.9, 1.0 - 0.9, 0.999, 1.0 - 0.999, 1.6e-4 / (1.0 - 0.9 ** 10), (1.0 - 0.999 ** 10) ** 0.5, 1e-15, 0.01 / 1031)
    k = trd.coefficients(1.6e-4, 1e-15, 10, weight=0.01, numel=1031)
    assert [k[n] for n in ("b1", "omb1", "b2", "omb2", "step_size", "bias2_sqrt", "eps", "c")] == [float(np.float32(x)) for x in c]
    assert k["omb2"] != float(np.float32(1.0) - np.float32(0.999)) and abs(k["omb2"] / float(np.float32(1.0) - np.float32(0.999)) - 1.0) > 1e-5


def test_yardstick_on_a_hand_computed_case():
    """b1 = 0.5, b2 = 0.75, t = 1: step_size = lr / 0.5, bias2_sqrt = 0.5; every value below is exact in binary floating point."""
    p = np.array([1.0, 0.0], np.float32)
    g = np.array([2.0, 0.0], np.float32)
    z = np.zeros(2, np.float32)
    pn, mn, vn = trd.step(p, g, z, z, lr=0.25, eps=0.5, t=1, b1=0.5, b2=0.75)
    # element 0: m = 1, v = 1, p = 1 - 0.5 * 1 / (1 / 0.5 + 0.5) = 0.8; element 1: 0 / (0 + eps): a step of exactly 0
    assert mn.tolist() == [1.0, 0.0] and vn.tolist() == [1.0, 0.0] and pn[0] == 1.0 - 0.5 / 2.5 and pn[1] == 0.0 and pn.dtype == np.float64
    # "sigmoid" at p = 0: s = 1/2, r = c / 4 with c = weight / numel = 1/2;  "exp" at p = 0: r = c
    _, ms, _ = trd.step(z, z, z, z, lr=0.25, eps=0.5, t=1, b1=0.5, b2=0.75, reg=("sigmoid", 1.0))
    _, me, _ = trd.step(z, z, z, z, lr=0.25, eps=0.5, t=1, b1=0.5, b2=0.75, reg=("exp", 1.0))
    assert ms.tolist() == [0.0625, 0.0625] and me.tolist() == [0.25, 0.25]
    bm, bv, bp, dg = trd.bounds(p, g, z, z, lr=0.25, eps=0.5, t=1, b1=0.5, b2=0.75)
    assert bm[1] == bv[1] == bp[1] == dg[1] == 0.0 and bm[0] > 0 and bv[0] > 0 and bp[0] > 0


HYPER = [(1.6e-4, 1e-15), (5e-2, 1e-8)]
CASES = [((1031, 3), None, None), ((1031, 1), ("sigmoid", 0.01), 16.0), ((1031, 3), ("exp", 0.01), 16.0)]


@pytest.mark.parametrize("t", [1, 2, 10, 1000, 30000])
def test_torch_adam_with_autograd_regularisers_stays_within_the_bounds(t):
    """The yardstick models the thing replaced: torch's CPU float32 Adam (single-tensor form), the regulariser added to the loss as a 3DGS-MCMC
    trainer adds it, lands within the yardstick's bounds at every element."""
    worst = [0.0] * 4
    for (shape, reg, p_to), (lr, eps) in ((c, h) for c in CASES for h in HYPER):
        p0, g0, m0, v0 = trd.make_inputs(shape, seed=t + len(shape) + (0 if reg is None else len(reg[0])), p_log_uniform_to=p_to)
        if t == 1:
            m0, v0 = np.zeros_like(m0), np.zeros_like(v0)
        param = torch.nn.Parameter(torch.from_numpy(p0.copy()))
        opt = torch.optim.Adam([param], lr=lr, eps=eps, foreach=False)
        if t > 1:
            opt.state[param] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m0.copy()), "exp_avg_sq": torch.from_numpy(v0.copy())}
        param.grad = torch.from_numpy(g0.copy())
        if reg is not None:
            act = torch.sigmoid(param) if reg[0] == "sigmoid" else torch.exp(param)
            (reg[1] * torch.abs(act).mean()).backward()
        gr = param.grad.numpy().copy()
        opt.step()
        assert float(opt.state[param]["step"]) == t
        p_ref, m_ref, v_ref = trd.step(p0, g0, m0, v0, lr, eps, t, reg=reg)
        bm, bv, bp, dg = trd.bounds(p0, g0, m0, v0, lr, eps, t, reg=reg)
        k = trd.coefficients(lr, eps, t, weight=reg[1] if reg else 0.0, numel=p0.size)
        g_ref = g0.astype(np.float64) + trd.regulariser(p0.astype(np.float64), reg[0] if reg else None, k["c"])[0]
        got = (gr, opt.state[param]["exp_avg"].numpy(), opt.state[param]["exp_avg_sq"].numpy(), param.detach().numpy())
        for i, (name, x, ref, bound) in enumerate((("g'", got[0], g_ref, dg), ("m", got[1], m_ref, bm), ("v", got[2], v_ref, bv), ("p", got[3], p_ref, bp))):
            err = np.abs(x.astype(np.float64) - ref)
            assert np.all(np.isfinite(x)), name
            ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
            worst[i] = max(worst[i], ratio)
            assert np.all(err <= bound), f"t={t} {shape} reg={reg} lr={lr}: {name} worst error / bound {ratio:.3g}"
    print(f"\nt={t}: torch CPU Adam, worst error / bound  g' {worst[0]:.2f}  m {worst[1]:.2f}  v {worst[2]:.2f}  p {worst[3]:.2f}")
