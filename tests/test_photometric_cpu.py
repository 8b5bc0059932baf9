"""CPU tests of the fused photometric loss (photometric_terms, fused_ssim, photometric_loss; include/stp_raster.h: stp_photometric_forward /
stp_photometric_backward): the float64 yardstick of the GPU tests against autograd and a hand-computed case, its bounds against the same
formulas in float32 (inside, with a factor 2 to spare) and against four broken versions (outside), the Python surface and what it refuses,
the C ABI's declarations, exports and argument validation (which runs before any launch, so without a GPU), and the loader's message for a
library without the symbols."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import torch_ref_photometric as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("random", "smooth", "constant", "identical")
SHAPE = (3, 37, 53)
GRADS = ((0.8, -0.2), (1.0, 0.0), (0.0, 1.0))

_cache = {}


def _yardstick(family):
    """(x, y, out, {g: (grad, grad bound)}, out bound) of one family at SHAPE: computed once, shared, never modified."""
    if family not in _cache:
        x, y = ref.images(family, *SHAPE, seed=3)
        out = ref.terms(x, y)
        per_g = {}
        out_bound = None
        for g in GRADS:
            out_bound, grad_bound = ref.bounds(x, y, *g)
            per_g[g] = (ref.grad(x, y, *g), grad_bound)
        _cache[family] = (x, y, out, per_g, out_bound)
    return _cache[family]


def _worst(err, bound):
    """The largest err / bound; an error of exactly 0 counts as 0 whatever the bound."""
    err, bound = torch.as_tensor(err).reshape(-1), torch.as_tensor(bound).reshape(-1)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max())


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------------
def test_window_is_the_float32_table_of_the_kernel():
    k = np.arange(11)
    w = np.exp(-(k - 5.0) ** 2 / 4.5)
    w /= w.sum()
    assert ref.WINDOW32.dtype == np.float32 and np.array_equal(ref.WINDOW32, w.astype(np.float32))
    assert np.array_equal(ref.WINDOW.numpy(), ref.WINDOW32.astype(np.float64)) and np.array_equal(ref.WINDOW32, ref.WINDOW32[::-1])
    src = open(os.path.join(ROOT, "stopthepop-rasterization_amd", "csrc", "stp_loss.hip")).read()
    table = re.search(r"constexpr\s+float\s+LOSS_WIN\[6\]\s*=\s*\{([^}]*)\}", src).group(1)
    kernel = np.array([np.float32(t.strip().rstrip("f")) for t in table.split(",")], np.float32)
    assert np.array_equal(kernel, ref.WINDOW32[:6])   # (the kernel holds w_0 .. w_5: w_{10-k} = w_k)


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 7, 5), (3, 37, 53), (3, 16, 70)])
def test_closed_form_gradient_is_autograd_of_the_terms(shape):
    x, y = ref.images("random", *shape, seed=5)
    if shape[1] > 1:
        y[0, 1, 0] = x[0, 1, 0]   # one pixel with x == y: sign(0) = 0
    for g0, g1 in ((0.8, -0.2), (0.3, 1.7)):
        xt = ref.planes_of(x).requires_grad_(True)
        out = ref.terms_t(xt, ref.planes_of(y))
        (g0 * out[0] + g1 * out[1]).backward()
        closed = ref.grad(x, y, g0, g1)
        assert float((closed - xt.grad).abs().max()) <= 1e-12 * float(xt.grad.abs().max())


def test_yardstick_on_a_hand_computed_case():
    """A 1 x 1 x 1 image: only the window's centre sees the pixel, blur(v) = w5^2 v."""
    x, y = np.float32(0.75), np.float32(0.25)
    c = float(ref.WINDOW32[5]) ** 2
    mu1, mu2 = c * 0.75, c * 0.25
    s1, s2, s12 = c * 0.5625 - mu1 * mu1, c * 0.0625 - mu2 * mu2, c * 0.1875 - mu1 * mu2
    A, B, Cc, D = 2 * mu1 * mu2 + 1e-4, 2 * s12 + 9e-4, mu1 * mu1 + mu2 * mu2 + 1e-4, s1 + s2 + 9e-4
    m = A * B / (Cc * D)
    out = ref.terms(np.full((1, 1, 1), x), np.full((1, 1, 1), y))
    assert out.dtype == torch.float64 and float(out[0]) == 0.5 and abs(float(out[1]) - m) <= 1e-15
    d1 = 2 * mu2 * B / (Cc * D) - 2 * mu2 * A / (Cc * D) - 2 * mu1 * A * B / (Cc * Cc * D) + 2 * mu1 * A * B / (Cc * D * D)
    d2, d3 = -A * B / (Cc * D * D), 2 * A / (Cc * D)
    g = ref.grad(np.full((1, 1, 1), x), np.full((1, 1, 1), y), 0.8, -0.2)
    want = -0.2 * c * (d1 + 2 * 0.75 * d2 + 0.25 * d3) + 0.8
    assert g.shape == (1, 1, 1, 1) and abs(float(g) - want) <= 1e-14 * abs(want)
    # the other sign of the L1 term, and sign(0) = 0 with SSIM = 1
    assert float(ref.grad(np.full((1, 1, 1), y), np.full((1, 1, 1), x), 1.0, 0.0)) == -1.0
    same = ref.terms(np.full((1, 1, 1), x), np.full((1, 1, 1), x))
    assert float(same[0]) == 0.0 and abs(float(same[1]) - 1.0) <= 1e-15
    assert float(ref.grad(np.full((1, 1, 1), x), np.full((1, 1, 1), x), 1.0, 0.0)) == 0.0


def test_reduction_chain_and_constants():
    TW, TH = ref.tile()
    assert (TW, TH) == (64, 16)
    assert ref.reduction_chain(1, 1, 1) == 4 + 6 + 3 + 1 + 6 + 3
    assert ref.reduction_chain(3, 1080, 1920) == 22 + -(-3 * 68 * 30 // 256)
    assert ref.K <= 32 and ref.U == 2.0 ** -24


# ---- the bounds: wide enough for float32, too tight for a wrong formula ------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_float32_composition_stays_inside_the_bounds(family):
    """The same formulas in float32 on the CPU (torch's conv2d, a 121-tap window): inside the bounds at the committed K with a factor 2 to spare."""
    x, y, out, per_g, out_bound = _yardstick(family)
    out32 = ref.terms(x, y, dtype=torch.float32).double()
    worst = [_worst((out32 - out).abs(), out_bound)]
    for g, (grad64, grad_bound) in per_g.items():
        grad32 = ref.grad(x, y, *g, dtype=torch.float32).double()
        worst.append(_worst((grad32 - grad64).abs(), grad_bound))
    print(family, "worst error / bound: out %.3g, gradients %s" % (worst[0], ["%.3g" % w for w in worst[1:]]))
    assert max(worst) <= 0.5, f"{family}: worst error / bound {max(worst):.3g} (out, then the gradients: {worst})"


@pytest.mark.parametrize("mutation, switches", [("replicate padding", dict(padding="replicate")), ("window shifted by one pixel", dict(shift=1)),
                                                ("C2 replaced by C1", dict(c2=ref.C1)), ("dropped 2x blur(s d2) term", dict(drop_d2=True))])
def test_mutated_versions_fall_outside_the_bounds(mutation, switches):
    """Float64 evaluations of a WRONG formula on the random family: the bounds are not vacuous."""
    x, y, out, per_g, out_bound = _yardstick("random")
    g = GRADS[0]
    grad64, grad_bound = per_g[g]
    wrong = ref.grad(x, y, *g, **switches)
    worst_grad = _worst((wrong - grad64).abs(), grad_bound)
    assert worst_grad > 1.0, f"{mutation}: the gradient stays inside the bounds ({worst_grad:.3g})"
    if "drop_d2" not in switches:   # (the dropped term is a fault of the backward alone)
        wrong_out = ref.terms(x, y, **switches)
        worst_out = _worst((wrong_out - out).abs()[1:], out_bound[1:])
        assert worst_out > 1.0, f"{mutation}: out[1] stays inside the bounds ({worst_out:.3g})"


# ---- the Python surface -------------------------------------------------------------------------------------------------------------------
def test_names_are_exported():
    import diff_gaussian_rasterization as dgr
    for name in ("photometric_terms", "fused_ssim", "photometric_loss"):
        assert name in dgr.__all__ and callable(getattr(dgr, name))


def test_padding_valid_is_refused():
    import diff_gaussian_rasterization as dgr
    a = torch.zeros(3, 8, 8)
    with pytest.raises(ValueError, match="valid"):
        dgr.fused_ssim(a, a, padding="valid")
    with pytest.raises(ValueError, match="valid"):
        dgr.fused_ssim(a, a, "valid", False)


def test_cpu_tensors_have_no_path():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    a, b = torch.rand(3, 8, 8), torch.rand(3, 8, 8)
    for call in (lambda: dgr.photometric_terms(a, b), lambda: dgr.photometric_loss(a, b), lambda: dgr.fused_ssim(a, b),
                 lambda: dgr.fused_ssim(a, b, train=False), lambda: dgr.photometric_loss(a.requires_grad_(True), b),
                 lambda: _C.photometric_forward(a, b, True), lambda: _C.photometric_backward(a, b, torch.zeros(3, 3, 8, 8), torch.zeros(2))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_refusals():
    """Each a RuntimeError, raised before anything is looked at on a device."""
    import diff_gaussian_rasterization as dgr
    a = torch.rand(3, 8, 8)
    for fn in (dgr.photometric_terms, dgr.photometric_loss, dgr.fused_ssim):
        with pytest.raises(RuntimeError, match="expected float32 tensor, got Double"):
            fn(a.double(), a.double())
        with pytest.raises(RuntimeError, match="expected float32 tensor, got Half"):
            fn(a, a.half())
        with pytest.raises(RuntimeError, match=r"image has shape \[3, 8, 8\], target has \[3, 8, 7\]"):
            fn(a, a[:, :, :7])
        with pytest.raises(RuntimeError, match=r"must be \(C, H, W\) or \(B, C, H, W\), got 2 dimensions"):
            fn(a[0], a[0])
        with pytest.raises(RuntimeError, match=r"must be \(C, H, W\) or \(B, C, H, W\), got 5 dimensions"):
            fn(a[None, None], a[None, None])
        with pytest.raises(RuntimeError, match="expected all tensors on cpu, got one on meta"):
            fn(a, torch.empty(3, 8, 8, device="meta"))
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(a[None], a[None])


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_calls():
    h = open(os.path.join(ROOT, "include", "stp_raster.h")).read()
    assert int(re.search(r"#define\s+STP_ABI_VERSION\s+(\d+)\b", h).group(1)) == 7
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    f = r"\s*const\s+float\s*\*\s*%s\s*,"
    assert re.search(r"size_t\s+stp_photometric_workspace_floats\s*\(\s*int\s+planes\s*,\s*int\s+H\s*,\s*int\s+W\s*\)\s*;", h)
    assert re.search(r"int\s+stp_photometric_forward\s*\(\s*int\s+planes\s*,\s*int\s+H\s*,\s*int\s+W\s*," + f % "image" + f % "target"
                     + r"\s*float\s*\*\s*out2\s*,\s*float\s*\*\s*maps\s*,\s*float\s*\*\s*workspace\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)
    assert re.search(r"int\s+stp_photometric_backward\s*\(\s*int\s+planes\s*,\s*int\s+H\s*,\s*int\s+W\s*," + f % "image" + f % "target" + f % "maps"
                     + f % "dL_dout2" + r"\s*float\s*\*\s*dL_dimage\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)


SYMBOLS = ("stp_photometric_workspace_floats", "stp_photometric_forward", "stp_photometric_backward")


def test_library_exports_the_calls_and_the_abi_stays_7():
    from diff_gaussian_rasterization import _C
    L = _C._load()
    assert L.stp_abi_version() == 7
    nm = subprocess.run(["nm", "-D", "--defined-only", _C.library_path()], capture_output=True, text=True).stdout
    for name in SYMBOLS:
        assert hasattr(L, name) and _C._require(name) is not None
        assert re.search(r" T %s$" % name, nm, re.M)
        assert _C._SYMBOL_FEATURE[name] == "the photometric loss"
    assert callable(_C._native().photometric_forward) and callable(_C._native().photometric_backward)


def test_loader_message_for_a_library_without_the_symbols(monkeypatch):
    from diff_gaussian_rasterization import _C
    import diff_gaussian_rasterization as dgr
    monkeypatch.setattr(_C, "_lib", types.SimpleNamespace())   # a loaded library that predates the exports
    for name in SYMBOLS:
        with pytest.raises(RuntimeError) as ex:
            _C._require(name)
        assert str(ex.value) == f"{_C.library_path()} does not export {name} (a library built before the photometric loss): rebuild it"
    z = torch.zeros(3, 4, 4)
    with pytest.raises(RuntimeError, match="does not export stp_photometric_"):
        dgr.photometric_loss(z, z)
    with pytest.raises(RuntimeError, match="does not export stp_photometric_backward"):
        _C.photometric_backward(z, z, torch.zeros(3, 3, 4, 4), torch.zeros(2))


def test_c_abi_validates_before_any_launch():
    """The refusals come before the first launch, so they need no GPU; the pointers are never followed (they are host addresses here)."""
    from diff_gaussian_rasterization import _C
    L = _C._load()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    err = lambda: L.stp_last_error().decode()
    fwd, bwd = L.stp_photometric_forward, L.stp_photometric_backward
    assert fwd(-1, 4, 4, a, a, a, a, a, None) == -1 and "negative size" in err()   # STP_ERR_INVALID_ARGUMENT
    assert fwd(3, 4, -4, a, a, a, None, a, None) == -1 and "negative size" in err()
    assert bwd(3, -4, 4, a, a, a, a, a, None) == -1 and "negative size" in err()
    assert fwd(2, 32768, 32768, a, a, a, a, a, None) == -1 and ">= 2^31" in err()
    assert fwd(65536, 65536, 65536, a, a, a, a, a, None) == -1 and ">= 2^31" in err()   # (an int product would wrap to 0)
    assert bwd(2 ** 31 - 1, 2, 1, a, a, a, a, a, None) == -1 and ">= 2^31" in err()
    for k in range(3, 8):
        if k == 6:
            continue   # maps: NULL is a forward without maps
        args = [3, 4, 4, a, a, a, a, a, None]
        args[k] = None
        assert fwd(*args) == -1 and "null pointer" in err(), k
    assert fwd(3, 4, 4, a, a, a, None, None, None) == -1 and "null pointer" in err()
    assert bwd(3, 4, 4, a, a, None, a, a, None) == -1 and "null maps" in err()
    for k in (3, 4, 6, 7):
        args = [3, 4, 4, a, a, a, a, a, None]
        args[k] = None
        assert bwd(*args) == -1 and "null pointer" in err(), k
    # empty work: no launch, 0, nothing touched
    assert fwd(0, 4, 4, None, None, None, None, None, None) == 0 and fwd(3, 0, 4, a, a, a, a, a, None) == 0 and fwd(3, 4, 0, a, a, a, None, a, None) == 0
    assert bwd(0, 4, 4, None, None, None, None, None, None) == 0 and bwd(3, 0, 4, a, a, a, a, a, None) == 0 and bwd(3, 4, 0, a, a, a, a, a, None) == 0
    assert all(v == 0.0 for v in buf)
    TW, TH = ref.tile()
    ws = L.stp_photometric_workspace_floats
    assert ws(1, 1, 1) == 2 and ws(3, TH, TW) == 6 and ws(3, TH + 1, TW + 1) == 24 and ws(1, 5, 3 * TW - 1) == 6
    assert ws(0, 4, 4) == 0 and ws(-1, 4, 4) == 0 and ws(2, 32768, 32768) == 0


def test_argument_check_program(tmp_path):
    """tests/cpp/photometric_args_check.cpp: the same refusals and empty calls from a stand-alone C++ program, built with the command line
    of tests/cpp/Makefile's rule for api_smoke.bin (compiler, flags, include and library paths), into a temporary directory."""
    lib = os.path.join(ROOT, "stopthepop-rasterization_amd", "diff_gaussian_rasterization")
    exe = str(tmp_path / "photometric_args_check.bin")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "photometric_args_check.cpp"), "-o", exe, "-L", lib, "-lstp_raster", f"-Wl,-rpath,{lib}"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"ok \d+\n", r.stdout) and int(r.stdout.split()[1]) >= 35
