"""Float64 autograd reference of the camera gradients: torch_ref's renderer with viewmatrix, projmatrix and campos as leaves.

The three camera tensors are independent leaves, and a view-space coordinate clamped to the 1.3 * tan_fov band inside the EWA Jacobian is
a constant, as in the rasterizer's backward: both conventions are spelled out at torch_ref.render_core(camera_leaves=True), which this
module calls.  Its own: Gaussians placed in the clamped band.
"""
from __future__ import annotations

import numpy as np

import torch_ref
from torch_ref import quat_to_rot  # noqa: F401  (the GPU tests build their covariances with it)


def render(scene, order="global", proper_ewa_scaling=False, use_cov3D_precomp=False, depth_key="z"):
    """Returns (image (3,H,W) float64 tensor, dict of leaf tensors with requires_grad), camera leaves included."""
    img, leaves, _ = torch_ref.render_core(scene, order, proper_ewa_scaling, use_cov3D_precomp, depth_key, camera_leaves=True)
    del leaves["means2D"]   # (the NDC shift is torch_ref's own leaf)
    return img, leaves


def with_clamped_gaussians(scene, z=10.0, ratio=1.4, sigma_px=4.0, opacity=0.5, y_band=False):
    """A copy of `scene` with two Gaussians appended whose view-space means lie in the clamped band (|x / z| = ratio * tan_fovx >
    1.3 * tan_fovx, one on each side), wide enough (sigma_px pixels) that their footprints reach into the frame.
    y_band: two more behind them, in the band of the other axis (|y / z| = ratio * tan_fovy, one on each side, x inside the frame),
    sized by the y focal length."""
    import copy
    sc = copy.deepcopy(scene)
    V = np.asarray(sc.viewmatrix, np.float64)
    focal = sc.W / (2.0 * sc.tanfovx)
    pts_view = np.array([[ratio * sc.tanfovx * z, 0.1 * sc.tanfovy * z, z], [-ratio * sc.tanfovx * z, -0.2 * sc.tanfovy * z, z]])
    s = sigma_px * z / focal
    sizes = [[s, 0.8 * s, 0.9 * s], [0.9 * s, s, 0.7 * s]]
    q = np.array([[0.9, 0.1, 0.3, 0.3], [0.8, -0.2, 0.4, 0.4]])
    colors = [[0.8, 0.3, 0.2], [0.1, 0.6, 0.9]]
    if y_band:
        pts_view = np.concatenate([pts_view, [[0.15 * sc.tanfovx * z, ratio * sc.tanfovy * z, z], [-0.3 * sc.tanfovx * z, -ratio * sc.tanfovy * z, z]]])
        sy = sigma_px * z / (sc.H / (2.0 * sc.tanfovy))
        sizes += [[0.8 * sy, sy, 0.9 * sy], [sy, 0.7 * sy, 0.9 * sy]]
        q = np.concatenate([q, [[0.7, 0.3, -0.1, 0.5], [0.6, -0.4, 0.2, -0.3]]])
        colors += [[0.4, 0.9, 0.3], [0.7, 0.2, 0.6]]
    n = len(pts_view)
    world = (pts_view - V[3, :3]) @ np.linalg.inv(V[:3, :3])
    f32 = lambda a: np.asarray(a, np.float32)
    sc.means3D = f32(np.concatenate([sc.means3D, world]))
    sc.scales = f32(np.concatenate([sc.scales, sizes]))
    sc.rotations = f32(np.concatenate([sc.rotations, q / np.linalg.norm(q, axis=1, keepdims=True)]))
    sc.opacities = f32(np.concatenate([sc.opacities, [[opacity]] * n]))
    if sc.shs is not None:
        sc.shs = f32(np.concatenate([sc.shs, np.tile(sc.shs[:1], (n, 1, 1))]))
    if sc.colors_precomp is not None:
        sc.colors_precomp = f32(np.concatenate([sc.colors_precomp, colors]))
    return sc


def loss_and_grads(scene, **kw):
    """(image, {leaf name: gradient of sum(dL_dout * image)}) in float64 numpy."""
    img, grads = torch_ref.loss_and_grads(scene, camera_leaves=True, **kw)
    del grads["means2D"]   # (the NDC shift is torch_ref's own leaf)
    return img, grads
