"""CPU tests of Mip-Splatting's 3D filter (compute_3d_filter, filtered_activations, _C.compute_3d_filter, _C.mip_activations,
_C.mip_activations_backward; include/stp_raster.h: stp_mip_filter_3d, stp_mip_activations_forward / _backward): the public names, the C ABI's
declarations, exports and argument validation (which runs before any launch, so without a GPU), what the functions refuse, pins of the float64
yardstick tests/torch_ref_mip_filter.py on hand-computed cases, the check of the input builders, and the MEASUREMENT that fixes the GPU tests'
tolerances: the worst error of the restatement of the kernels' own evaluation order against the yardstick, on exactly the GPU tests' inputs.

Measured (numpy on the CPU)                                                       GPU bound = 4 x measured
  filter_3d, relative (worst at C = 67)                              7.8e-7  ->  FILTER_BOUND       = 3.12e-6
  scales, relative                                                   1.6e-7  ->  SCALES_BOUND       = 6.4e-7
  opacities, relative                                                3.6e-7  ->  OPACITIES_BOUND    = 1.44e-6
  grad_scaling, relative to the row's largest |grad_scaling|         4.0e-7  ->  GRAD_SCALING_BOUND = 1.6e-6
  grad_opacity, relative                                             4.2e-7  ->  GRAD_OPACITY_BOUND = 1.68e-6
The factor 4 covers the kernel's fused multiply-adds and the few-ulp differences between the device's and numpy's exp / sqrt / division.  The
filter's error is the cancellation of the view transform's terms where z is small beside them; every `valid` decision of the restatement is the
float64 one on these inputs, which lie 1e-4 away from every threshold.

The builders' figures (the candidates inside the margin, the rows no camera sees) are those of THESE builders -- scenes.uniform(41, 7, .) and the
focal lengths of torch_ref_mip_filter.cameras -- and are pinned below: C <= 5 leaves rows without a camera (the fix-up path), C = 67 none."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import torch_ref_mip_filter as trf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("stp_mip_filter_3d", "stp_mip_activations_forward", "stp_mip_activations_backward")


def test_names_are_public():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import compute_3d_filter, filtered_activations   # noqa: F401
    assert "compute_3d_filter" in dgr.__all__ and "filtered_activations" in dgr.__all__
    from diff_gaussian_rasterization import _C
    assert callable(_C.compute_3d_filter) and callable(_C.mip_activations) and callable(_C.mip_activations_backward)


def test_header_declares_the_calls():
    h = open(os.path.join(ROOT, "include", "stp_raster.h")).read()
    assert int(re.search(r"#define\s+STP_ABI_VERSION\s+(\d+)\b", h).group(1)) == 7
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    cf, f = r"const\s+float\s*\*\s*", r"float\s*\*\s*"
    assert re.search(r"int\s+stp_mip_filter_3d\s*\(\s*int\s+P\s*,\s*int\s+C\s*,\s*" + cf + r"xyz\s*,\s*" + cf + r"world_view_transforms\s*,\s*" + cf + r"intrinsics\s*,"
                     r"\s*void\s*\*\s*workspace\s*,\s*" + f + r"filter_3d\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)
    assert re.search(r"int\s+stp_mip_activations_forward\s*\(\s*int\s+P\s*,\s*" + cf + r"scaling\s*,\s*" + cf + r"opacity\s*,\s*" + cf + r"filter_3d\s*,\s*" + f + r"scales\s*,\s*"
                     + f + r"opacities\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)
    assert re.search(r"int\s+stp_mip_activations_backward\s*\(\s*int\s+P\s*,\s*" + cf + r"scaling\s*,\s*" + cf + r"opacity\s*,\s*" + cf + r"filter_3d\s*,\s*" + cf
                     + r"grad_scales\s*,\s*" + cf + r"grad_opacities\s*,\s*" + f + r"grad_scaling\s*,\s*" + f + r"grad_opacity\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)


def test_library_exports_the_calls_and_the_abi_stays_7():
    from diff_gaussian_rasterization import _C
    L = _C._load()
    assert L.stp_abi_version() == 7
    nm = subprocess.run(["nm", "-D", "--defined-only", _C.library_path()], capture_output=True, text=True).stdout
    for name in SYMBOLS:
        assert hasattr(L, name) and _C._require(name) is not None
        assert re.search(r" T " + name + r"$", nm, re.M)
    host = _C._native()
    assert callable(host.compute_3d_filter) and callable(host.mip_activations) and callable(host.mip_activations_backward)


def test_loader_message_for_a_library_without_the_symbols(monkeypatch):
    import types
    from diff_gaussian_rasterization import _C
    monkeypatch.setattr(_C, "_lib", types.SimpleNamespace())   # a loaded library that predates the exports
    s, o, f = torch.zeros(2, 3), torch.zeros(2), torch.ones(2)
    for name, call in (("stp_mip_filter_3d", lambda: _C.compute_3d_filter(torch.zeros(2, 3), torch.zeros(1, 4, 4), torch.ones(1, 4))),
                       ("stp_mip_activations_forward", lambda: _C.mip_activations(s, o, f)),
                       ("stp_mip_activations_backward", lambda: _C.mip_activations_backward(s, o, f, s, None))):
        with pytest.raises(RuntimeError) as ex:
            call()
        assert str(ex.value) == f"{_C.library_path()} does not export {name} (a library built before the Mip-Splatting 3D filter): rebuild it"


def test_c_abi_validates_before_any_launch():
    """The refusals come before the launch, so they need no GPU (a launch here would fail with STP_ERR_HIP, not -1); the pointers are never
    followed (they are host addresses)."""
    from diff_gaussian_rasterization import _C
    L = _C._load()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    err = lambda: L.stp_last_error().decode()
    filt = lambda P=4, C=2, xyz=a, views=a, intr=a, ws=a, out=a: L.stp_mip_filter_3d(P, C, xyz, views, intr, ws, out, None)
    assert filt(P=-1) == -1 and "stp_mip_filter_3d" in err() and "negative P" in err()
    assert filt(C=-1) == -1 and "stp_mip_filter_3d" in err() and "negative C" in err()
    assert filt(C=0) == -1 and "stp_mip_filter_3d: C == 0" in err()
    assert filt(P=0, C=0) == -1 and "C == 0" in err()                       # (what is wrong is refused all the same)
    assert filt(C=1 << 24) == -1 and "2^24" in err()
    for name in ("xyz", "views", "intr", "ws", "out"):
        assert filt(**{name: None}) == -1 and "stp_mip_filter_3d: null pointer" in err()
    assert filt(P=0) == 0 and filt(P=0, xyz=None, views=None, intr=None, ws=None, out=None) == 0   # empty work: no launch, 0

    fwd = lambda P=4, s=a, o=a, f=a, so=a, oo=a: L.stp_mip_activations_forward(P, s, o, f, so, oo, None)
    assert fwd(P=-3) == -1 and "stp_mip_activations_forward" in err() and "negative P" in err()
    for name in ("s", "o", "f", "so", "oo"):
        assert fwd(**{name: None}) == -1 and "stp_mip_activations_forward: null pointer" in err()
    assert fwd(P=0) == 0 and fwd(P=0, s=None, o=None, f=None, so=None, oo=None) == 0

    bwd = lambda P=4, s=a, o=a, f=a, gs=a, go=a, gso=a, goo=a: L.stp_mip_activations_backward(P, s, o, f, gs, go, gso, goo, None)
    assert bwd(P=-3) == -1 and "stp_mip_activations_backward" in err() and "negative P" in err()
    for name in ("s", "o", "f", "gso", "goo"):
        assert bwd(**{name: None}) == -1 and "stp_mip_activations_backward: null pointer" in err()
    assert bwd(gs=None, go=None) == -1 and "stp_mip_activations_backward: null pointer" in err() and "both absent" in err()
    assert bwd(P=0) == 0 and bwd(P=0, s=None, o=None, f=None, gs=None, go=None, gso=None, goo=None) == 0
    assert all(x == 0.0 for x in buf)


def test_cpu_tensors_have_no_path():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    xyz, views, intr = torch.zeros(4, 3), torch.eye(4)[None].repeat(2, 1, 1), torch.ones(2, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.compute_3d_filter(xyz, views, intr)
    s, o, f = torch.zeros(4, 3, requires_grad=True), torch.zeros(4, 1, requires_grad=True), torch.ones(4, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.filtered_activations(s, o, f)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.mip_activations_backward(s.detach(), o.detach(), f, torch.ones(4, 3), None)


def test_refusals_name_the_argument():
    """What is wrong with the tensors themselves is refused before where they live is looked at: every refusal can be met without a GPU."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    xyz, views, intr = torch.zeros(4, 3), torch.eye(4)[None].repeat(2, 1, 1), torch.ones(2, 4)
    for args, what in (((xyz.double(), views, intr), "compute_3d_filter: xyz: expected float32"), ((xyz, views.half(), intr), "world_view_transforms: expected float32"),
                       ((xyz, views, intr.double()), "intrinsics: expected float32"), ((torch.zeros(4, 4), views, intr), r"xyz must be \(P, 3\)"),
                       ((xyz, torch.zeros(2, 16), intr), r"world_view_transforms must be \(C, 4, 4\)"), ((xyz, views, torch.ones(3, 4)), r"intrinsics must be \(2, 4\)"),
                       ((xyz, views, torch.ones(2, 3)), r"intrinsics must be \(2, 4\)"), ((xyz, views[:0], intr[:0]), "C == 0"),
                       ((xyz[:0], views[:0], intr[:0]), "C == 0")):
        with pytest.raises(RuntimeError, match=what):
            dgr.compute_3d_filter(*args)
    s, o, f = torch.zeros(4, 3), torch.zeros(4, 1), torch.ones(4)
    for args, what in (((s.double(), o, f), "filtered_activations: scaling: expected float32"), ((s, o.half(), f), "opacity: expected float32"),
                       ((s, o, f.double()), "filter_3d: expected float32"), ((torch.zeros(4, 4), o, f), r"scaling must be \(P, 3\)"),
                       ((s, torch.zeros(3), f), "opacity has 3 rows, scaling has 4"), ((s, torch.zeros(2, 2), f), r"opacity must be \(n,\) or \(n, 1\)"),
                       ((s, o, torch.ones(5, 1)), "filter_3d has 5 rows, scaling has 4"), ((s, o, torch.ones(4, 2)), r"filter_3d must be \(n,\) or \(n, 1\)")):
        with pytest.raises(RuntimeError, match=what):
            dgr.filtered_activations(*args)
    for args, what in (((s, o, f, None, None), "both None"), ((s, o, f, torch.zeros(4, 2), None), r"grad_scales must be \(4, 3\)"),
                       ((s, o, f, None, torch.zeros(3)), "grad_opacities has 3 rows"), ((s, o, f, s.double(), None), "grad_scales: expected float32")):
        with pytest.raises(RuntimeError, match=what):
            _C.mip_activations_backward(*args)


def test_example_refuses_the_filter_with_raw_params():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_render", os.path.join(ROOT, "examples", "train_render.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(SystemExit, match="--filter-3d cannot be combined with --raw-params: .*do not read filter_3d"):
        mod.main(["--filter-3d", "--raw-params"])


# ---- the yardstick, pinned on hand-computed cases --------------------------------------------------------------------------------------------------

def _identity_camera(fx=50.0, fy=40.0, W=64.0, H=48.0):
    return np.eye(4, dtype=np.float32)[None], np.float32([[fx, fy, W, H]])


def test_yardstick_pins_of_the_filter():
    views, intr = _identity_camera()
    # a point on the optical axis at depth 4: distance 4, filter = 4 / 50 * sqrt(0.2)
    out, any_, _ = trf.filter_3d(np.float32([[0, 0, 4.0]]), views, intr)
    assert any_.tolist() == [True] and abs(out[0, 0] - 4.0 / 50.0 * np.sqrt(0.2)) < 1e-16
    # a point just behind z = 0.2 is not valid and takes the maximum over the valid rows (4)
    out, any_, _ = trf.filter_3d(np.float32([[0, 0, 4.0], [0, 0, 0.19999], [0, 0, 1.0]]), views, intr)
    assert any_.tolist() == [True, False, True]
    assert np.allclose(out[:, 0], np.array([4.0, 4.0, 1.0]) / 50.0 * np.sqrt(0.2), rtol=1e-15)
    # the 15 % border: u = x / z * 50 + 32 against [-9.6, 73.6]: at z = 1, x = 0.83 gives 73.5 (inside), x = 0.834 gives 73.7 (outside);
    # v = y / z * 40 + 24 against [-7.2, 55.2]: y = -0.77 gives -6.8 (inside), y = -0.79 gives -7.6 (outside)
    pts = np.float32([[0.83, 0, 1], [0.834, 0, 1], [-0.83, 0, 1], [-0.834, 0, 1], [0, -0.77, 1], [0, -0.79, 1], [0, 0.77, 1], [0, 0.79, 1], [0, 0, 2.5]])
    out, any_, _ = trf.filter_3d(pts, views, intr)
    assert any_.tolist() == [True, False, True, False, True, False, True, False, True]
    assert np.allclose(out[~any_, 0], 2.5 / 50.0 * np.sqrt(0.2), rtol=1e-15) and np.allclose(out[any_, 0][:-1], 1.0 / 50.0 * np.sqrt(0.2), rtol=1e-15)
    # no valid row at all: every row keeps 100000 (upstream raises); the restatement agrees
    behind = np.float32([[0, 0, -1.0], [5.0, 0, 1.0]])
    out, any_, _ = trf.filter_3d(behind, views, intr)
    assert not any_.any() and np.allclose(out[:, 0], 100000.0 / 50.0 * np.sqrt(0.2), rtol=1e-15)
    got, _ = trf.filter_kernel_order(behind, views, intr)
    assert np.allclose(got, out, rtol=1e-6)
    # the minimum over cameras, max_c(focal_x) over all of them (the second camera sees nothing: it looks the other way), a NaN row takes the maximum
    back = np.diag([-1.0, 1.0, -1.0, 1.0]).astype(np.float32)
    views2, intr2 = np.stack([views[0], back]), np.float32([[50, 40, 64, 48], [80, 40, 64, 48]])
    out, any_, valid = trf.filter_3d(np.float32([[0, 0, 4.0], [np.nan, 0, 1.0], [0, 0, 2.0]]), views2, intr2)
    assert valid.tolist() == [[True, False], [False, False], [True, False]]
    assert np.allclose(out[:, 0], np.array([4.0, 4.0, 2.0]) / 80.0 * np.sqrt(0.2), rtol=1e-15)
    got, valid32 = trf.filter_kernel_order(np.float32([[0, 0, 4.0], [np.nan, 0, 1.0], [0, 0, 2.0]]), views2, intr2)
    assert np.array_equal(valid, valid32) and np.allclose(got, out, rtol=1e-6)


def test_yardstick_pins_of_the_activations():
    # e = 1 (scaling 0), f = 1: scales = sqrt(2), r = 1/2 per axis, opacities = sigmoid(0) * sqrt(1/8)
    s, o, gs, go = trf.activations(np.zeros((1, 3), np.float32), np.zeros(1, np.float32), np.ones(1, np.float32), np.ones((1, 3), np.float32), np.ones(1, np.float32))
    assert np.allclose(s, np.sqrt(2.0), rtol=1e-15) and abs(o[0] - 0.5 * np.sqrt(0.125)) < 1e-16
    # grad_scaling_j = g_s e^2 / scales + g_o opacities (1 - r_j) = 1 / sqrt(2) + opacities / 2;  grad_opacity = g_o sqrt(1/8) / 4
    assert np.allclose(gs, 1.0 / np.sqrt(2.0) + 0.25 * np.sqrt(0.125), rtol=1e-14) and abs(go[0] - 0.25 * np.sqrt(0.125)) < 1e-16
    # filter 0: exp(scaling) and sigmoid(opacity)
    sc, op = np.float32([[-2.0, 0.5, 1.0]]), np.float32([1.5])
    s, o, _, _ = trf.activations(sc, op, np.zeros(1, np.float32))
    assert np.allclose(s, np.exp(sc.astype(np.float64)), rtol=1e-15) and np.allclose(o, 1.0 / (1.0 + np.exp(-1.5)), rtol=1e-15)
    # the restatement's formulas are the yardstick's (ratio form against determinant form), also where one gradient is absent
    a = trf.activation_inputs(64)
    for cs, co in trf.GRAD_CASES:
        g = (a["g_scales"] if cs else None), (a["g_opacities"] if co else None)
        ref = trf.activations(a["scaling"], a["opacity"], a["filter_3d"], *g)
        got = trf.activations_backward_kernel_order(a["scaling"], a["opacity"], a["filter_3d"], *g)
        assert np.allclose(got[0], ref[2], rtol=1e-4, atol=1e-7) and np.allclose(got[1], ref[3], rtol=1e-4, atol=1e-9)
        if not co:
            assert np.all(ref[3] == 0) and np.all(got[1] == 0)


# ---- the builders ----------------------------------------------------------------------------------------------------------------------------------

INVALID_ROWS = {1: 342, 3: 10, 5: 1, 67: 0}   # rows of points(C) that no camera of cameras(C) sees


def test_builders_cover_what_the_gpu_tests_need():
    assert trf.P == 1031 and trf.CAMERA_COUNTS == (1, 3, 5, 67)
    cand = trf.candidates()
    assert cand.shape == (2062, 3) and cand.dtype == np.float32 and cand.min() >= -6.0 and cand.max() <= 6.0
    for C in trf.CAMERA_COUNTS:
        xyz, dropped = trf.points(C)
        views, intr = trf.cameras(C)
        assert xyz.shape == (1031, 3) and views.shape == (C, 4, 4) and intr.shape == (C, 4) and views.dtype == intr.dtype == np.float32
        assert dropped <= 22, (C, dropped)
        valid, z, margin = trf.classify(xyz, views, intr)
        assert margin.min() >= trf.MARGIN
        _, valid32 = trf.filter_kernel_order(xyz, views, intr)
        assert np.array_equal(valid, valid32), C                 # the float32 and the float64 classifications agree on every kept point
        invalid = int((~valid.any(axis=1)).sum())
        print(f"\nC = {C}: {dropped} of 2062 candidates inside the margin, {invalid} rows without a camera")
        assert invalid == INVALID_ROWS[C]
        away = [c for c in range(C) if c % 5 == 4]
        assert not valid[:, away].any()                          # the cameras that look away see nothing
        assert len(set(intr[:, 0].tolist())) == min(C, 4) and 60 <= intr[:, 2].min() and intr[:, 2].max() <= 70
    assert INVALID_ROWS[1] > 0 and INVALID_ROWS[3] > 0 and INVALID_ROWS[5] > 0 and INVALID_ROWS[67] == 0   # fix-up path at C <= 5, pure minimum at C = 67
    a = trf.activation_inputs()
    assert a["scaling"].shape == (1031, 3) and -9.0 <= a["scaling"].min() and a["scaling"].max() <= 1.0
    assert a["opacity"].shape == (1031,) and 2.5 < a["opacity"].std() < 3.5
    assert np.exp(-8.0) * (1 - 1e-6) <= a["filter_3d"].min() and a["filter_3d"].max() <= np.exp(-1.0) * (1 + 1e-6)


# ---- the measurement -------------------------------------------------------------------------------------------------------------------------------

def test_measured_tolerance_of_the_filter():
    worst = 0.0
    for C in trf.CAMERA_COUNTS:
        xyz, _ = trf.points(C)
        views, intr = trf.cameras(C)
        ref, valid_any, valid = trf.filter_3d(xyz, views, intr)
        got, valid32 = trf.filter_kernel_order(xyz, views, intr)
        assert got.dtype == np.float32 and got.shape == (trf.P, 1) and np.array_equal(valid, valid32)
        e = trf.relative_error(got, ref)
        print(f"\nfilter restatement, C = {C}: worst relative error {e:.3g}")
        worst = max(worst, e)
    print(f"\nfilter restatement: worst relative error {worst:.3g}; GPU bound {trf.FILTER_BOUND:.3g}")
    assert 0.5 * trf.FILTER_MEASURED <= worst <= trf.FILTER_MEASURED
    assert trf.FILTER_BOUND == 4 * trf.FILTER_MEASURED


def test_measured_tolerance_of_the_activations():
    a = trf.activation_inputs()
    ref_s, ref_o, _, _ = trf.activations(a["scaling"], a["opacity"], a["filter_3d"])
    got_s, got_o = trf.activations_kernel_order(a["scaling"], a["opacity"], a["filter_3d"])
    es, eo = trf.relative_error(got_s, ref_s), trf.relative_error(got_o, ref_o)
    print(f"\nactivations restatement: worst relative error scales {es:.3g} (GPU bound {trf.SCALES_BOUND:.3g}), opacities {eo:.3g} (GPU bound {trf.OPACITIES_BOUND:.3g})")
    assert 0.5 * trf.SCALES_MEASURED <= es <= trf.SCALES_MEASURED and 0.5 * trf.OPACITIES_MEASURED <= eo <= trf.OPACITIES_MEASURED
    worst_s = worst_o = 0.0
    for cs, co in trf.GRAD_CASES:
        g = (a["g_scales"] if cs else None), (a["g_opacities"] if co else None)
        _, _, ref_gs, ref_go = trf.activations(a["scaling"], a["opacity"], a["filter_3d"], *g)
        got_gs, got_go = trf.activations_backward_kernel_order(a["scaling"], a["opacity"], a["filter_3d"], *g)
        worst_s, worst_o = max(worst_s, trf.row_error(got_gs, ref_gs)), max(worst_o, trf.row_error(got_go, ref_go))
    print(f"\nbackward restatement: worst row-relative error grad_scaling {worst_s:.3g} (GPU bound {trf.GRAD_SCALING_BOUND:.3g}), grad_opacity {worst_o:.3g} "
          f"(GPU bound {trf.GRAD_OPACITY_BOUND:.3g})")
    assert 0.5 * trf.GRAD_SCALING_MEASURED <= worst_s <= trf.GRAD_SCALING_MEASURED and 0.5 * trf.GRAD_OPACITY_MEASURED <= worst_o <= trf.GRAD_OPACITY_MEASURED
    assert (trf.SCALES_BOUND, trf.OPACITIES_BOUND, trf.GRAD_SCALING_BOUND, trf.GRAD_OPACITY_BOUND) == \
        (4 * trf.SCALES_MEASURED, 4 * trf.OPACITIES_MEASURED, 4 * trf.GRAD_SCALING_MEASURED, 4 * trf.GRAD_OPACITY_MEASURED)
