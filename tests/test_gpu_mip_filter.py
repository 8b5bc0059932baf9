"""GPU tests of Mip-Splatting's 3D filter (compute_3d_filter, filtered_activations; include/stp_raster.h: stp_mip_filter_3d,
stp_mip_activations_forward / _backward) against the float64 yardstick tests/torch_ref_mip_filter.py.

Tolerances: 4 times the worst error of the CPU restatement of the kernels' evaluation order on exactly these inputs, as
tests/test_mip_filter_cpu.py measures it: filter 3.12e-6, scales 6.4e-7, opacities 1.44e-6 (relative); grad_scaling 1.6e-6 (relative to the row's
largest |grad_scaling|), grad_opacity 1.68e-6 (relative).  The inputs lie 1e-4 away from every threshold of the filter, so every `valid`
decision must be the float64 one: a row the yardstick sees takes its own distance, a row it does not see takes the maximum, bit for bit.

The filter kernel owns one Gaussian per lane in workgroups of 256 and reads the cameras at a wave-uniform index (no chunks: every C takes the
same path); its second kernel takes max_c(focal_x) with a stride of 256 cameras per lane, so C = 300 is the size at which that loop turns
twice.  The activation kernels own four rows per lane where every pointer is 16-byte aligned (P % 4 rows in a tail) and one otherwise.

Measured on MI355X: filter 6.7e-7 (C = 67; 4.2e-7 at C = 300), scales 1.2e-7, opacities 2.6e-7, grad_scaling 3.1e-7 (3.7e-7 with three
log-scales of -15), grad_opacity 3.5e-7; through the rasterizer the two routes' gradients differ by at most 9.4e-7 of the largest entry."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import helpers
import torch_ref_mip_filter as trf
from helpers import FULL_STP, _rel, settings_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def dgr():
    import diff_gaussian_rasterization as d
    return d


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- the filter ----------------------------------------------------------------------------------------------------------------------------------

_runs = {}


def filter_run(C):
    """-> (xyz, views, intrinsics, yardstick (filter, valid_any), the kernel's result on the device) of the shared inputs, computed once"""
    if C not in _runs:
        xyz, _ = trf.points(C)
        views, intr = trf.cameras(C)
        ref, valid_any, _ = trf.filter_3d(xyz, views, intr)
        _runs[C] = (xyz, views, intr, ref, valid_any, dgr().compute_3d_filter(dev(xyz), dev(views), dev(intr)))
    return _runs[C]


def check_filter(label, got, ref, valid_any):
    assert got.shape == ref.shape and got.dtype == torch.float32 and got.is_cuda and not got.requires_grad
    e = trf.relative_error(got.cpu().numpy(), ref)
    print(f"\n{label}: worst relative error {e:.3g} (bound {trf.FILTER_BOUND:.3g}), {int((~valid_any).sum())} rows without a camera")
    assert e <= trf.FILTER_BOUND
    if valid_any.any() and not valid_any.all():   # rows invalid everywhere equal the maximum over the valid rows bit for bit
        top = got[dev(valid_any)].max()
        assert torch.equal(bits(got[dev(~valid_any)]), bits(top).expand_as(got[dev(~valid_any)]))


@pytest.mark.parametrize("C", trf.CAMERA_COUNTS)
def test_filter_against_the_yardstick(C):
    xyz, views, intr, ref, valid_any, got = filter_run(C)
    assert got.shape == (trf.P, 1)
    check_filter(f"C = {C}", got, ref, valid_any)
    assert (C == 67) == bool(valid_any.all())   # the fix-up path at C <= 5, the pure minimum at C = 67


def test_filter_with_more_cameras_than_a_workgroup_has_lanes():
    """C = 300 (points(300): the candidates clear of these 300 cameras' thresholds): the second kernel's loop over the focal lengths turns twice."""
    xyz, views, intr, ref, valid_any, got = filter_run(300)
    check_filter("C = 300", got, ref, valid_any)


def test_filter_single_camera_looking_away():
    xyz, _ = trf.points(1)
    views, intr = trf.cameras(5)
    views, intr = views[4:5], intr[4:5]   # c % 5 == 4: looks directly away from the origin
    ref, valid_any, _ = trf.filter_3d(xyz, views, intr)
    got = dgr().compute_3d_filter(dev(xyz), dev(views), dev(intr))
    want = np.float32(np.float32(100000.0) / intr[0, 0]) * np.float32(0.4472135955)   # 100000 / focal_x * sqrt(0.2), in the kernel's order
    assert not valid_any.any()
    assert torch.equal(got, torch.full((trf.P, 1), float(want), device=DEV))
    assert trf.relative_error(got.cpu().numpy(), ref) <= trf.FILTER_BOUND


def test_filter_focal_maximum_is_over_all_cameras():
    """The largest focal_x belongs to a camera that sees nothing (it looks away) -- as camera 299 of 300 too, behind the first stride of the
    second kernel's loop."""
    for C in (5, 300):
        xyz, views, intr, _, _, base = filter_run(C)
        last = C - 1
        assert last % 5 == 4
        intr2 = intr.copy()
        intr2[last, 0] = 2.0 * intr[:, 0].max()   # (a camera that looks away: its focal length changes no decision)
        ref, valid_any, _ = trf.filter_3d(xyz, views, intr2)
        got = dgr().compute_3d_filter(dev(xyz), dev(views), dev(intr2))
        assert trf.relative_error(got.cpu().numpy(), ref) <= trf.FILTER_BOUND
        ratio = (base.double() / got.double()).cpu().numpy()
        assert np.allclose(ratio, 2.0, rtol=1e-6)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
def test_filter_prefixes(n):
    """Rows are independent apart from the maximum: a prefix against the yardstick run of that prefix, and the rows some camera sees against the
    full run's rows, bit for bit."""
    xyz, views, intr, _, valid_any, full = filter_run(3)
    ref, any_n, _ = trf.filter_3d(xyz[:n], views, intr)
    got = dgr().compute_3d_filter(dev(xyz[:n]), dev(views), dev(intr))
    assert got.shape == (n, 1)
    assert trf.relative_error(got.cpu().numpy(), ref) <= trf.FILTER_BOUND
    assert np.array_equal(any_n, valid_any[:n])
    if any_n.any():
        seen = dev(any_n)
        assert torch.equal(bits(got[seen]), bits(full[:n][seen]))
        assert torch.equal(bits(got[~seen]), bits(got[seen].max()).expand_as(got[~seen]))
    else:
        assert torch.equal(got, torch.full_like(got, float(got[0, 0]))) and float(got[0, 0]) > 100.0   # nobody is seen: 100000 / focal * sqrt(0.2)


def test_filter_edge_inputs():
    xyz, views, intr, ref, valid_any, full = filter_run(3)
    d_views, d_intr = dev(views), dev(intr)
    empty = dgr().compute_3d_filter(dev(xyz[:0]), d_views, d_intr)
    assert empty.shape == (0, 1) and empty.dtype == torch.float32 and empty.is_cuda
    with pytest.raises(RuntimeError, match="C == 0"):
        dgr().compute_3d_filter(dev(xyz), d_views[:0], d_intr[:0])
    with pytest.raises(RuntimeError, match="intrinsics: expected all tensors on"):
        dgr().compute_3d_filter(dev(xyz), d_views, d_intr.cpu())
    # one NaN row takes the maximum and changes no other row (row 0 is seen by a camera: the maximum does not hang on it alone)
    row = int(np.flatnonzero(valid_any)[0])
    assert float(full[row, 0]) < float(full.max())
    poisoned = xyz.copy()
    poisoned[row, 1] = np.nan
    got = dgr().compute_3d_filter(dev(poisoned), d_views, d_intr)
    keep = torch.ones(trf.P, dtype=torch.bool, device=DEV)
    keep[row] = False
    assert torch.equal(bits(got[keep]), bits(full[keep])) and torch.equal(bits(got[row]), bits(full.max().reshape(1)))
    # a non-contiguous xyz gives the bits of its contiguous copy; so do non-contiguous cameras
    wide = torch.zeros(trf.P, 5, device=DEV)
    wide[:, 1:4] = dev(xyz)
    view = wide[:, 1:4]
    assert not view.is_contiguous()
    assert same_bits(dgr().compute_3d_filter(view, d_views, d_intr), full)
    assert same_bits(dgr().compute_3d_filter(dev(xyz), d_views.transpose(1, 2).contiguous().transpose(1, 2), d_intr), full)
    # two calls give equal bits; a leaf that requires grad is read like any tensor and nothing is recorded
    again = dgr().compute_3d_filter(dev(xyz).requires_grad_(True), d_views, d_intr)
    assert same_bits(again, full) and not again.requires_grad and again.grad_fn is None


# ---- the activations -------------------------------------------------------------------------------------------------------------------------------

def act_inputs(n=trf.P):
    a = trf.activation_inputs(n)
    return a, {k: dev(v) for k, v in a.items()}


def check_forward(label, scales, opacities, a):
    ref_s, ref_o, _, _ = trf.activations(a["scaling"], a["opacity"], a["filter_3d"])
    es, eo = trf.relative_error(scales.detach().cpu().numpy(), ref_s), trf.relative_error(opacities.detach().cpu().numpy().reshape(-1), ref_o)
    print(f"\n{label}: worst relative error scales {es:.3g} (bound {trf.SCALES_BOUND:.3g}), opacities {eo:.3g} (bound {trf.OPACITIES_BOUND:.3g})")
    assert es <= trf.SCALES_BOUND and eo <= trf.OPACITIES_BOUND


def check_backward(label, g_scaling, g_opacity, a, use_s, use_o):
    _, _, ref_gs, ref_go = trf.activations(a["scaling"], a["opacity"], a["filter_3d"], a["g_scales"] if use_s else None, a["g_opacities"] if use_o else None)
    es, eo = trf.row_error(g_scaling.cpu().numpy(), ref_gs), trf.row_error(g_opacity.cpu().numpy().reshape(-1), ref_go)
    print(f"\n{label}: worst row-relative error grad_scaling {es:.3g} (bound {trf.GRAD_SCALING_BOUND:.3g}), grad_opacity {eo:.3g} (bound {trf.GRAD_OPACITY_BOUND:.3g})")
    assert es <= trf.GRAD_SCALING_BOUND and eo <= trf.GRAD_OPACITY_BOUND


@pytest.mark.parametrize("column", [False, True])
def test_activations_against_the_yardstick(column):
    """Forward and backward through autograd on leaves that require grad, with both opacity shapes, under random upstream gradients and under
    each of the two alone; filter_3d.grad stays None."""
    a, d = act_inputs()
    shape = (trf.P, 1) if column else (trf.P,)
    first = None
    for use_s, use_o in trf.GRAD_CASES:
        s, o = d["scaling"].clone().requires_grad_(True), d["opacity"].reshape(shape).clone().requires_grad_(True)
        f = d["filter_3d"].reshape(shape).clone().requires_grad_(True)   # (a buffer: it gets no gradient even where it asks for one)
        scales, opacities = dgr().filtered_activations(s, o, f)
        assert scales.shape == (trf.P, 3) and opacities.shape == shape and scales.requires_grad and opacities.requires_grad
        check_forward(f"column {column}", scales, opacities, a)
        if first is None:
            first = (scales.detach(), opacities.detach())
        else:   # equal inputs give equal bits
            assert same_bits(scales, first[0]) and same_bits(opacities, first[1])
        loss = torch.zeros((), device=DEV)
        if use_s:
            loss = loss + (scales * d["g_scales"]).sum()
        if use_o:
            loss = loss + (opacities * d["g_opacities"].reshape(shape)).sum()
        loss.backward()
        assert f.grad is None and s.grad.shape == (trf.P, 3) and o.grad.shape == shape
        check_backward(f"column {column} g_scales {use_s} g_opacities {use_o}", s.grad, o.grad, a, use_s, use_o)
        if not use_o:
            assert torch.equal(o.grad, torch.zeros_like(o.grad))


def test_activations_backward_is_deterministic_and_matches_the_binding():
    from diff_gaussian_rasterization import _C
    a, d = act_inputs()
    one = _C.mip_activations_backward(d["scaling"], d["opacity"], d["filter_3d"], d["g_scales"], d["g_opacities"])
    two = _C.mip_activations_backward(d["scaling"], d["opacity"][:, None], d["filter_3d"][:, None], d["g_scales"], d["g_opacities"][:, None])
    assert one[1].shape == (trf.P,) and two[1].shape == (trf.P, 1)
    assert same_bits(one[0], two[0]) and same_bits(one[1], two[1].reshape(-1))
    check_backward("binding", one[0], one[1], a, True, True)
    # an absent upstream gradient is a zero one, bit for bit
    only_s = _C.mip_activations_backward(d["scaling"], d["opacity"], d["filter_3d"], d["g_scales"], None)
    zeros_o = _C.mip_activations_backward(d["scaling"], d["opacity"], d["filter_3d"], d["g_scales"], torch.zeros_like(d["g_opacities"]))
    assert same_bits(only_s[0], zeros_o[0]) and torch.equal(only_s[1], torch.zeros_like(only_s[1]))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 257, trf.P])
def test_activations_narrow_path_equals_the_wide_path(n):
    """A view offset by one row starts 12 (scaling) and 4 (opacity, filter_3d) bytes into its storage: it takes the narrow path, and its result
    equals the wide path's on the same rows bit for bit -- forward and backward, tails and single rows included."""
    from diff_gaussian_rasterization import _C
    a, d = act_inputs(n + 1)
    view = {k: v[1:] for k, v in d.items()}
    copy = {k: v[1:].clone() for k, v in d.items()}
    assert all(v.is_contiguous() and v.data_ptr() % 16 != 0 for v in view.values()) and all(v.data_ptr() % 16 == 0 for v in copy.values())
    narrow, wide = _C.mip_activations(view["scaling"], view["opacity"], view["filter_3d"]), _C.mip_activations(copy["scaling"], copy["opacity"], copy["filter_3d"])
    assert same_bits(narrow[0], wide[0]) and same_bits(narrow[1], wide[1])
    narrow = _C.mip_activations_backward(view["scaling"], view["opacity"], view["filter_3d"], view["g_scales"], view["g_opacities"])
    wide = _C.mip_activations_backward(copy["scaling"], copy["opacity"], copy["filter_3d"], copy["g_scales"], copy["g_opacities"])
    assert same_bits(narrow[0], wide[0]) and same_bits(narrow[1], wide[1])
    tail = {k: v[1:] for k, v in a.items()}
    check_forward(f"n = {n}", *_C.mip_activations(copy["scaling"], copy["opacity"], copy["filter_3d"]), tail)
    check_backward(f"n = {n}", wide[0], wide[1], tail, True, True)


def test_activations_special_values():
    from diff_gaussian_rasterization import _C
    a, d = act_inputs()
    # filter_3d = 0: exp(scaling) and sigmoid(opacity), to within the bounds (no bit is promised: the root of e * e is the hardware's)
    zero = torch.zeros_like(d["filter_3d"])
    scales, opacities = _C.mip_activations(d["scaling"], d["opacity"], zero)
    ref_s, ref_o = np.exp(a["scaling"].astype(np.float64)), 1.0 / (1.0 + np.exp(-a["opacity"].astype(np.float64)))
    assert trf.relative_error(scales.cpu().numpy(), ref_s) <= trf.SCALES_BOUND and trf.relative_error(opacities.cpu().numpy(), ref_o) <= trf.OPACITIES_BOUND
    # three scalings of -15 (e^2 = 9e-14 beside f^2 of 1e-7 .. 0.14): finite, non-NaN outputs and gradients, still within the bounds
    small = dict(a, scaling=np.full_like(a["scaling"], -15.0))
    ds = torch.full_like(d["scaling"], -15.0)
    scales, opacities = _C.mip_activations(ds, d["opacity"], d["filter_3d"])
    g = _C.mip_activations_backward(ds, d["opacity"], d["filter_3d"], d["g_scales"], d["g_opacities"])
    for t in (scales, opacities, *g):
        assert bool(torch.isfinite(t).all())
    assert bool((scales > 0).all()) and bool((opacities > 0).all())
    check_forward("scaling -15", scales, opacities, small)
    check_backward("scaling -15", g[0], g[1], small, True, True)
    empty = dgr().filtered_activations(d["scaling"][:0], d["opacity"][:0], d["filter_3d"][:0])
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,)
    with pytest.raises(RuntimeError, match="filter_3d: expected all tensors on"):
        dgr().filtered_activations(d["scaling"], d["opacity"], d["filter_3d"].cpu())


# ---- with the rasterizer ---------------------------------------------------------------------------------------------------------------------------

MODES = {"global": settings_dict(0), "hier": settings_dict(**FULL_STP)}


@pytest.mark.parametrize("mode", list(MODES))
def test_filtered_activations_feed_the_rasterizer(mode):
    """A 1000-Gaussian 64 x 48 frame rendered from filtered_activations(...) against the torch composition of the same formulas feeding the same
    rasterizer call: the gradients on _scaling and _opacity agree within the activations' gradient bound plus the tolerance
    tests/test_gpu_raw_params.py uses between its two routes (2e-5 of the tensor's largest entry: float atomics in the render half)."""
    from diff_gaussian_rasterization import scenes
    sc = scenes.make_scene(P=1000, W=64, H=48, sigma_min=1.0, sigma_max=9.0, seed=4)
    t = lambda x, rg=False: torch.tensor(np.asarray(x, np.float32), device=DEV).requires_grad_(rg)
    views = t(sc.viewmatrix)[None]
    intr = torch.tensor([[sc.W / (2.0 * sc.tanfovx), sc.H / (2.0 * sc.tanfovy), sc.W, sc.H]], dtype=torch.float32, device=DEV)
    filter_3d = dgr().compute_3d_filter(t(sc.means3D), views, intr)
    assert filter_3d.shape == (1000, 1) and bool((filter_3d > 0).all())
    op = np.clip(np.asarray(sc.opacities, np.float64), 1e-4, 1 - 1e-4)
    raw_scaling, raw_opacity = np.log(np.asarray(sc.scales, np.float64)), np.log(op / (1 - op)).reshape(-1, 1)
    results = {}
    for route in ("fused", "torch"):
        scaling, opacity = t(raw_scaling, True), t(raw_opacity, True)
        if route == "fused":
            scales, opacities = dgr().filtered_activations(scaling, opacity, filter_3d)
        else:   # the formulas of the issue, composed in torch
            e2, f2 = torch.square(torch.exp(scaling)), torch.square(filter_3d)
            scales = torch.sqrt(e2 + f2)
            opacities = torch.sigmoid(opacity) * torch.sqrt((e2 / (e2 + f2)).prod(dim=1, keepdim=True))
        means3D = t(sc.means3D)
        rast = dgr().GaussianRasterizer(helpers.api_settings(sc, helpers.ext_settings(MODES[mode]), DEV))
        out = rast(means3D, torch.zeros_like(means3D, requires_grad=True), opacities, shs=t(sc.shs), scales=scales, rotations=t(sc.rotations))
        (out[0] * t(sc.dL_dout)).sum().backward()
        results[route] = (out[0].detach(), scaling.grad.cpu().double().numpy(), opacity.grad.cpu().double().numpy(), int((out[1] > 0).sum()))
    fused, ref = results["fused"], results["torch"]
    assert fused[3] > 100 and float(np.abs(ref[1]).max()) > 0 and float(np.abs(ref[2]).max()) > 0
    assert float((fused[0] - ref[0]).abs().max()) < 1e-4   # (the two routes' scales and opacities differ by roundings)
    for name, k, bound in (("_scaling", 1, trf.GRAD_SCALING_BOUND), ("_opacity", 2, trf.GRAD_OPACITY_BOUND)):
        r = _rel(fused[k], ref[k])
        print(f"\n{mode} {name}: largest difference relative to the largest entry {r:.3g} (bound {bound + trf.RASTER_ROUTE_TOLERANCE:.3g})")
        assert r <= bound + trf.RASTER_ROUTE_TOLERANCE


def test_example_with_the_3d_filter():
    """examples/train_render.py --filter-3d --iters 6 --points 2000: render() feeds filtered_activations to the rasterizer and the short fit descends."""
    spec = importlib.util.spec_from_file_location("train_render", os.path.join(ROOT, "examples", "train_render.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    first, last = mod.main(["--filter-3d", "--iters", "6", "--points", "2000"])
    assert np.isfinite(first) and np.isfinite(last) and last < first, (first, last)
