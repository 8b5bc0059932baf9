"""Float64 yardstick of Mip-Splatting's 3D filter (include/stp_raster.h: stp_mip_filter_3d, stp_mip_activations_forward / _backward), the
restatements of the kernels' own evaluation order that fix the tolerances on the CPU, and the inputs the CPU measurement and the GPU tests share.

filter_3d(): the formulas of compute_3d_filter literally, in float64 from the float32 inputs, with the division in the screen test:
    valid = z > 0.2  and  -0.15 W <= x / max(z, 0.001) * focal_x + W / 2 <= 1.15 W  and the same in y;   distance = min over valid cameras of z
    rows without a valid camera take max(distance[valid_any]) (100000 where there is none);   filter = distance / max_c(focal_x) * sqrt(0.2)
activations(): UPSTREAM's determinant form in torch float64 -- scales = sqrt(e^2 + f^2), opacities = sigmoid(o) * sqrt(prod e^2 / prod (e^2 + f^2)) --
and its gradients from torch.autograd.
filter_kernel_order() / activations_kernel_order() / activations_backward_kernel_order(): what csrc/stp_mip_filter.hip computes, operation by
operation, in numpy float32 (numpy has no fused multiply-add: the chains round once more per step than the kernel's, which the factor 4 between
the measured error and the GPU bound covers, with the few-ulp differences between the device's and numpy's exp / sqrt)."""
import math

import numpy as np
import torch

from diff_gaussian_rasterization import scenes

P = 1031                      # not a multiple of 4, 64 or 256
CAMERA_COUNTS = (1, 3, 5, 67)
MARGIN = 1e-4                 # the kept points are this far (relative to 0.2, the width, the height) from every threshold in every camera
FAR, NEAR, BORDER = 100000.0, 0.2, 0.15

# The worst errors of the restatements against the yardstick on the inputs below, as tests/test_mip_filter_cpu.py measures them (rounded up to
# two digits), and the GPU tests' bounds: 4 times that.  Forward values: relative.  Gradients: per output, relative to the largest magnitude of
# that output's yardstick gradient in the row.
FILTER_MEASURED = 7.8e-7         # (C = 67: the cancellation of the fma chain's terms in a small z)
SCALES_MEASURED = 1.6e-7
OPACITIES_MEASURED = 3.6e-7
GRAD_SCALING_MEASURED = 4.0e-7
GRAD_OPACITY_MEASURED = 4.2e-7
FILTER_BOUND, SCALES_BOUND, OPACITIES_BOUND = 4 * FILTER_MEASURED, 4 * SCALES_MEASURED, 4 * OPACITIES_MEASURED
GRAD_SCALING_BOUND, GRAD_OPACITY_BOUND = 4 * GRAD_SCALING_MEASURED, 4 * GRAD_OPACITY_MEASURED
# The rasterizer test compares two routes through the SAME rasterizer call: the activations' gradient bound plus the tolerance
# tests/test_gpu_raw_params.py uses between its two routes (float atomics in the render half), relative to the tensor's largest entry.
RASTER_ROUTE_TOLERANCE = 2e-5


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------

def cameras(C):
    """-> (world_view_transforms (C, 4, 4), intrinsics (C, 4)) float32.  Camera c sits at (7 cos a, 1.5 sin 3a, 7 sin a), a = 2 pi c / C + 0.1, and
    looks at the origin -- every camera with c % 5 == 4 directly AWAY from it.  Focal lengths and image sizes (about 64 x 48) vary with c."""
    views, intrinsics = np.zeros((C, 4, 4), np.float32), np.zeros((C, 4), np.float32)
    for c in range(C):
        a = 2.0 * math.pi * c / C + 0.1
        eye = np.array([7.0 * math.cos(a), 1.5 * math.sin(3.0 * a), 7.0 * math.sin(a)])
        target = 2.0 * eye if c % 5 == 4 else np.zeros(3)
        views[c] = scenes.look_at_view(eye, target).astype(np.float32)
        intrinsics[c] = (42.0 + 3.0 * (c % 4), 45.0 + 2.0 * (c % 3), 64.0 + 2.0 * (c % 3), 48.0 + 2.0 * (c % 2))
    return views, intrinsics


def camera_space(xyz, views, dtype=np.float64):
    """-> (x, y, z) of shape (P, C): p_cam = [p, 1] @ M in `dtype`, from the float32 inputs."""
    p, M = np.asarray(xyz, np.float32).astype(dtype), np.asarray(views, np.float32).astype(dtype)
    cam = np.einsum("pk,ckj->pcj", p, M[:, :3, :3]) + M[None, :, 3, :3]
    return cam[..., 0], cam[..., 1], cam[..., 2]


def classify(xyz, views, intrinsics):
    """The float64 decisions -> (valid (P, C) bool, z (P, C), margin (P, C)): margin = the smallest relative distance to a threshold that counts --
    |z - 0.2| / 0.2 and, in front of the depth test only, |u - bound| / W and |v - bound| / H for the four screen bounds."""
    K = np.asarray(intrinsics, np.float32).astype(np.float64)
    fx, fy, W, H = (K[None, :, j] for j in range(4))
    x, y, z = camera_space(xyz, views)
    zc = np.maximum(z, 0.001)
    u, v = x / zc * fx + W / 2.0, y / zc * fy + H / 2.0
    in_screen = (u >= -BORDER * W) & (u <= (1.0 + BORDER) * W) & (v >= -BORDER * H) & (v <= (1.0 + BORDER) * H)
    valid = (z > NEAR) & in_screen
    screen = np.minimum(np.minimum(np.abs(u + BORDER * W), np.abs(u - (1.0 + BORDER) * W)) / W, np.minimum(np.abs(v + BORDER * H), np.abs(v - (1.0 + BORDER) * H)) / H)
    margin = np.where(z > NEAR, np.minimum(np.abs(z - NEAR) / NEAR, screen), np.abs(z - NEAR) / NEAR)
    return valid, z, margin


def candidates():
    """2 P float32 points, uniform in [-6, 6]^3."""
    return (scenes.uniform(41, 7, 6 * P).reshape(2 * P, 3) * 12.0 - 6.0).astype(np.float32)


_points = {}


def points(C):
    """-> (xyz (P, 3) float32, the candidates dropped): the first P candidates clear of every threshold in every one of cameras(C) by MARGIN."""
    if C not in _points:
        cand = candidates()
        views, intrinsics = cameras(C)
        clear = classify(cand, views, intrinsics)[2].min(axis=1) >= MARGIN
        assert int(clear.sum()) >= P, (C, int(clear.sum()))
        _points[C] = (np.ascontiguousarray(cand[clear][:P]), int((~clear).sum()))
    return _points[C][0].copy(), _points[C][1]


def activation_inputs(n=P):
    """-> dict of float32 arrays: scaling (n, 3) U(-9, 1), opacity (n,) N(0, 3), filter_3d (n,) exp(U(-8, -1)), and the upstream gradients g_scales
    (n, 3), g_opacities (n,) N(0, 1)."""
    return {"scaling": (scenes.uniform(43, 1, 3 * n).reshape(n, 3) * 10.0 - 9.0).astype(np.float32),
            "opacity": (3.0 * scenes.normal(43, 2, n)).astype(np.float32),
            "filter_3d": np.exp(scenes.uniform(43, 3, n) * 7.0 - 8.0).astype(np.float32),
            "g_scales": scenes.normal(43, 4, 3 * n).reshape(n, 3).astype(np.float32),
            "g_opacities": scenes.normal(43, 5, n).astype(np.float32)}


# ---- the float64 yardstick -----------------------------------------------------------------------------------------------------------------------

def filter_3d(xyz, views, intrinsics):
    """-> (filter (P, 1) float64, valid_any (P,) bool, valid (P, C) bool)"""
    valid, z, _ = classify(xyz, views, intrinsics)
    distance = np.where(valid, z, FAR).min(axis=1, initial=FAR)
    valid_any = valid.any(axis=1)
    if valid_any.any():
        distance[~valid_any] = distance[valid_any].max()
    focal = float(np.asarray(intrinsics, np.float32)[:, 0].astype(np.float64).max())
    return (distance / focal * 0.2 ** 0.5)[:, None], valid_any, valid


def activations(scaling, opacity, filter_3d, g_scales=None, g_opacities=None):
    """Upstream's determinant form in float64 -> (scales (n, 3), opacities (n,), grad_scaling, grad_opacity) as float64 arrays; the gradients (of
    sum(scales * g_scales) + sum(opacities * g_opacities), an absent g counting as zero) are None when both g are."""
    s = torch.tensor(np.asarray(scaling, np.float32), dtype=torch.float64, requires_grad=True)
    o = torch.tensor(np.asarray(opacity, np.float32).reshape(-1), dtype=torch.float64, requires_grad=True)
    f = torch.tensor(np.asarray(filter_3d, np.float32).reshape(-1, 1), dtype=torch.float64)
    e2 = torch.square(torch.exp(s))
    d = e2 + torch.square(f)
    scales = torch.sqrt(d)
    opacities = torch.sigmoid(o) * torch.sqrt(e2.prod(dim=1) / d.prod(dim=1))
    if g_scales is None and g_opacities is None:
        return scales.detach().numpy(), opacities.detach().numpy(), None, None
    loss = torch.zeros((), dtype=torch.float64)
    if g_scales is not None:
        loss = loss + (scales * torch.tensor(np.asarray(g_scales, np.float32), dtype=torch.float64)).sum()
    if g_opacities is not None:
        loss = loss + (opacities * torch.tensor(np.asarray(g_opacities, np.float32).reshape(-1), dtype=torch.float64)).sum()
    gs, go = torch.autograd.grad(loss, (s, o), allow_unused=True)
    zero = lambda g, like: np.zeros(like.shape) if g is None else g.numpy()
    return scales.detach().numpy(), opacities.detach().numpy(), zero(gs, s), zero(go, o)


# ---- the kernels' evaluation order, float32 ------------------------------------------------------------------------------------------------------------

F = np.float32


def filter_kernel_order(xyz, views, intrinsics):
    """-> (filter (P, 1) float32, valid (P, C) bool): csrc/stp_mip_filter.hip's order -- p_cam[k] = p2 M[2][k] + (p1 M[1][k] + (p0 M[0][k] + M[3][k])),
    the screen test division-free, |x focal_x| <= (0.65 W) z -- every step rounded to float32 (the kernel's chains are fmas)."""
    p, M, K = np.asarray(xyz, F), np.asarray(views, F), np.asarray(intrinsics, F)
    cam = [p[:, 2:3] * M[None, :, 2, k] + (p[:, 1:2] * M[None, :, 1, k] + (p[:, 0:1] * M[None, :, 0, k] + M[None, :, 3, k])) for k in range(3)]
    x, y, z = cam
    assert z.dtype == F
    with np.errstate(invalid="ignore"):
        valid = (z > F(NEAR)) & (np.abs(x * K[None, :, 0]) <= (F(0.65) * K[None, :, 2]) * z) & (np.abs(y * K[None, :, 1]) <= (F(0.65) * K[None, :, 3]) * z)
    distance = np.where(valid, z, F(FAR)).min(axis=1, initial=F(FAR)).astype(F)
    valid_any = valid.any(axis=1)
    if valid_any.any():
        distance[~valid_any] = distance[valid_any].max()
    out = (distance / K[:, 0].max()) * F(0.4472135955)
    assert out.dtype == F
    return out[:, None], valid


def _row_terms(scaling, opacity, filter_3d):
    s, o, f = np.asarray(scaling, F), np.asarray(opacity, F).reshape(-1), np.asarray(filter_3d, F).reshape(-1, 1)
    e = np.exp(s)
    e2, f2 = e * e, f * f
    d = e2 + f2   # (the kernel's is fma(e, e, f2): one rounding less)
    scl = np.sqrt(d)
    r = e2 / d
    sig = F(1.0) / (F(1.0) + np.exp(-o))
    c = np.sqrt((r[:, 0] * r[:, 1]) * r[:, 2])
    opa = sig * c
    assert all(a.dtype == F for a in (scl, r, sig, c, opa))
    return e2, f2, d, scl, sig, c, opa


def activations_kernel_order(scaling, opacity, filter_3d):
    """-> (scales (n, 3), opacities (n,)) float32 in the kernel's order"""
    _, _, _, scl, _, _, opa = _row_terms(scaling, opacity, filter_3d)
    return scl, opa


def activations_backward_kernel_order(scaling, opacity, filter_3d, g_scales=None, g_opacities=None):
    """-> (grad_scaling (n, 3), grad_opacity (n,)) float32 in the kernel's order; an absent upstream gradient is zeros"""
    e2, f2, d, scl, sig, c, opa = _row_terms(scaling, opacity, filter_3d)
    gs = np.zeros_like(scl) if g_scales is None else np.asarray(g_scales, F)
    go = np.zeros_like(opa) if g_opacities is None else np.asarray(g_opacities, F).reshape(-1)
    t = (go * opa)[:, None]
    g_scaling = gs * (e2 / scl) + t * (f2 / d)
    g_opacity = ((go * c) * sig) * (F(1.0) / (F(1.0) + np.exp(np.asarray(opacity, F).reshape(-1))))   # (1 - sig as sigmoid(-o): no cancellation)
    assert g_scaling.dtype == F and g_opacity.dtype == F
    return g_scaling, g_opacity


# ---- error measures ---------------------------------------------------------------------------------------------------------------------------------

def relative_error(got, ref):
    """the largest |got - ref| / |ref| over the elements (ref float64, nowhere zero)"""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape and np.all(ref != 0) and np.all(np.isfinite(got))
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def row_error(got, ref):
    """the largest over rows of  max_j |got - ref| / max_j |ref|  (rows whose yardstick gradient is zero throughout must be zero in got)"""
    got, ref = np.asarray(got, np.float64).reshape(len(ref), -1), np.asarray(ref, np.float64).reshape(len(ref), -1)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    top = np.abs(ref).max(axis=1)
    assert np.all(got[top == 0] == 0)
    keep = top > 0
    return float(np.max(np.abs(got - ref).max(axis=1)[keep] / top[keep])) if keep.any() else 0.0


GRAD_CASES = ((True, True), (True, False), (False, True))   # (g_scales given, g_opacities given)
