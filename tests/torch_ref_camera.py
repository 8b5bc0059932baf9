"""Float64 autograd reference of the camera gradients: torch_ref.render's maths with viewmatrix, projmatrix and campos as leaves.

Same splatting maths as torch_ref.render (textbook EWA, real SH basis, alpha compositing in a per-pixel order), written
independently of the HIP kernels, with two conventions spelled out where the camera enters:
  * the three camera tensors are INDEPENDENT leaves, as the rasterizer reads them (it never checks that projmatrix = viewmatrix @ P
    or that campos is the camera centre);
  * the 1.3 * tan_fov clamp of the view-space mean inside the EWA Jacobian is differentiated as the rasterizer differentiates it for
    means3D (the reference's backward.cu): a clamped coordinate is a constant -- it carries no gradient to the view-space mean,
    and its value enters J as a number.  (torch_ref differentiates clamp(x / z) * z, which also moves with z; the two agree for every
    Gaussian inside the band.)
Culling, tile binning and every sort key are non-differentiable here, as in the product.
"""
from __future__ import annotations

import numpy as np
import torch

from torch_ref import eval_sh, quat_to_rot


def render(scene, order="global", proper_ewa_scaling=False, use_cov3D_precomp=False, depth_key="z"):
    """Returns (image (3,H,W) float64 tensor, dict of leaf tensors with requires_grad), camera leaves included."""
    dd = torch.float64
    t = lambda a: torch.tensor(np.asarray(a), dtype=dd)
    W, H = scene.W, scene.H
    V = t(scene.viewmatrix).requires_grad_(True)
    PM = t(scene.projmatrix).requires_grad_(True)
    cam = t(scene.campos).requires_grad_(True)
    INV, bg = t(scene.inv_viewprojmatrix), t(scene.bg)
    leaves = {"viewmatrix": V, "projmatrix": PM, "campos": cam}
    means = t(scene.means3D).requires_grad_(True); leaves["means3D"] = means
    opac = t(scene.opacities).requires_grad_(True); leaves["opacities"] = opac
    scales = t(scene.scales).requires_grad_(True); leaves["scales"] = scales
    rots = t(scene.rotations).requires_grad_(True); leaves["rotations"] = rots
    P = means.shape[0]

    Rm = quat_to_rot(rots)
    Sd = torch.diag_embed((scene.scale_modifier * scales) ** 2)
    Sigma = Rm @ Sd @ Rm.transpose(1, 2)
    if use_cov3D_precomp:
        c6 = torch.stack([Sigma[:, 0, 0], Sigma[:, 0, 1], Sigma[:, 0, 2], Sigma[:, 1, 1], Sigma[:, 1, 2], Sigma[:, 2, 2]], 1)
        c6 = c6.detach().clone().requires_grad_(True); leaves["cov3D_precomp"] = c6
        Sigma = torch.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]], 1).reshape(-1, 3, 3)

    pv = means @ V[:3, :3] + V[3, :3]          # view-space means (row-vector convention)
    tz = pv[:, 2]
    near_ok = (tz > 0.2).detach()
    fx, fy = W / (2 * scene.tanfovx), H / (2 * scene.tanfovy)
    limx, limy = 1.3 * scene.tanfovx, 1.3 * scene.tanfovy
    with torch.no_grad():
        rx, ry = pv[:, 0] / tz, pv[:, 1] / tz
        in_x, in_y = (rx >= -limx) & (rx <= limx), (ry >= -limy) & (ry <= limy)
        cx, cy = torch.clamp(rx, -limx, limx) * tz, torch.clamp(ry, -limy, limy) * tz
    txc = torch.where(in_x, pv[:, 0], cx)
    tyc = torch.where(in_y, pv[:, 1], cy)
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -fx * txc / (tz * tz), zero, fy / tz, -fy * tyc / (tz * tz)], 1).reshape(-1, 2, 3)
    JW = J @ V[:3, :3].T                          # W = V[:3,:3]^T: p_view = W p + t
    cov2 = JW @ Sigma @ JW.transpose(1, 2)
    a0, b0, c0 = cov2[:, 0, 0], cov2[:, 0, 1], cov2[:, 1, 1]
    a, b, c = a0 + 0.3, b0, c0 + 0.3
    det = a * c - b * b
    o = opac[:, 0]
    if proper_ewa_scaling:
        o = o * torch.sqrt(torch.clamp((a0 * c0 - b0 * b0) / det, min=0.000025))
    cA, cB, cC = c / det, -b / det, a / det

    ph = torch.cat([means, torch.ones(P, 1, dtype=dd)], 1) @ PM
    ndc = ph[:, :2] / (ph[:, 3:4] + 1e-7)
    mx = ((ndc[:, 0] + 1) * W - 1) * 0.5
    my = ((ndc[:, 1] + 1) * H - 1) * 0.5

    if scene.shs is not None:
        shs = t(scene.shs).requires_grad_(True); leaves["shs"] = shs
        d = means - cam
        d = d / d.norm(dim=1, keepdim=True)
        col = torch.clamp(eval_sh(scene.sh_degree, shs, d), min=0.0)
    else:
        col = t(scene.colors_precomp).requires_grad_(True); leaves["colors_precomp"] = col

    with torch.no_grad():   # binning (3.33 sigma rectangle of tiles), culling
        mid = 0.5 * (a + c)
        lam = mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.01))
        radius = 3.33 * torch.sqrt(lam)
        visible = near_ok & (det != 0) & (o >= 1.0 / 255.0)
        x0 = torch.clamp(torch.floor((mx - radius) / 16), 0, (W + 15) // 16)
        x1 = torch.clamp(torch.ceil((mx + radius) / 16), 0, (W + 15) // 16)
        y0 = torch.clamp(torch.floor((my - radius) / 16), 0, (H + 15) // 16)
        y1 = torch.clamp(torch.ceil((my + radius) / 16), 0, (H + 15) // 16)
        visible &= ((x1 - x0) * (y1 - y0)) > 0

    ys, xs = torch.meshgrid(torch.arange(H, dtype=dd), torch.arange(W, dtype=dd), indexing="ij")
    px, py = xs.reshape(-1), ys.reshape(-1)
    dx = mx[None, :] - px[:, None]
    dy = my[None, :] - py[:, None]
    power = -0.5 * (cA[None] * dx * dx + cC[None] * dy * dy) - cB[None] * dx * dy
    G = torch.exp(torch.clamp(power, max=0.0))
    alpha = torch.clamp(o[None] * G, max=0.99)
    with torch.no_grad():   # per-pixel order: non-differentiable
        camd = cam.detach()
        tx_, ty_ = torch.floor(px / 16), torch.floor(py / 16)
        in_rect = (tx_[:, None] >= x0[None]) & (tx_[:, None] < x1[None]) & (ty_[:, None] >= y0[None]) & (ty_[:, None] < y1[None])
        keep = in_rect & visible[None] & (power <= 0) & (alpha >= 1.0 / 255.0)
        if order == "global":
            key = (tz if depth_key == "z" else (means - camd).norm(dim=1))[None].expand(px.shape[0], P)
        else:   # depth along each pixel's ray
            s_cl = torch.clamp(scales, min=1e-3) * scene.scale_modifier
            Sinv = Rm @ torch.diag_embed(1.0 / (s_cl ** 2)) @ Rm.transpose(1, 2)
            ndcx, ndcy = px * (2.0 / W) - 1.0, py * (2.0 / H) - 1.0
            pw = ndcx[:, None] * INV[0][None] + ndcy[:, None] * INV[1][None] + INV[3][None]
            pw = pw[:, :3] / pw[:, 3:4]
            v = pw - camd
            v = v / v.norm(dim=1, keepdim=True)
            u = torch.einsum("pij,pj->pi", Sinv, means - camd)
            key = (v @ u.T) / torch.clamp(torch.einsum("ni,pij,nj->np", v, Sinv, v), min=1e-5)
            keep &= key >= 0
        key = torch.where(keep, key, torch.full_like(key, float("inf")))
        idx = torch.argsort(key, dim=1, stable=True)
    a_s = torch.gather(torch.where(keep, alpha, torch.zeros_like(alpha)), 1, idx)
    one_m = 1 - a_s
    Tbefore = torch.cumprod(torch.cat([torch.ones(a_s.shape[0], 1, dtype=dd), one_m[:, :-1]], 1), 1)
    with torch.no_grad():
        stop = (Tbefore * one_m) < 1e-4
        alive = torch.cumsum(stop.to(torch.int64), 1) == 0
    wgt = torch.where(alive, a_s * Tbefore, torch.zeros_like(a_s))
    C = (wgt[..., None] * col[idx]).sum(1)
    T_final = torch.where(alive, one_m, torch.ones_like(one_m)).prod(1)
    img = C + T_final[:, None] * bg[None]
    return img.T.reshape(3, H, W), leaves


def with_clamped_gaussians(scene, z=10.0, ratio=1.4, sigma_px=4.0, opacity=0.5):
    """A copy of `scene` with two Gaussians appended whose view-space means lie in the clamped band (|x / z| = ratio * tan_fovx >
    1.3 * tan_fovx, one on each side), wide enough (sigma_px pixels) that their footprints reach into the frame."""
    import copy
    sc = copy.deepcopy(scene)
    V = np.asarray(sc.viewmatrix, np.float64)
    focal = sc.W / (2.0 * sc.tanfovx)
    pts_view = np.array([[ratio * sc.tanfovx * z, 0.1 * sc.tanfovy * z, z], [-ratio * sc.tanfovx * z, -0.2 * sc.tanfovy * z, z]])
    world = (pts_view - V[3, :3]) @ np.linalg.inv(V[:3, :3])
    s = sigma_px * z / focal
    f32 = lambda a: np.asarray(a, np.float32)
    sc.means3D = f32(np.concatenate([sc.means3D, world]))
    sc.scales = f32(np.concatenate([sc.scales, [[s, 0.8 * s, 0.9 * s], [0.9 * s, s, 0.7 * s]]]))
    q = np.array([[0.9, 0.1, 0.3, 0.3], [0.8, -0.2, 0.4, 0.4]])
    sc.rotations = f32(np.concatenate([sc.rotations, q / np.linalg.norm(q, axis=1, keepdims=True)]))
    sc.opacities = f32(np.concatenate([sc.opacities, [[opacity], [opacity]]]))
    if sc.shs is not None:
        sc.shs = f32(np.concatenate([sc.shs, np.tile(sc.shs[:1], (2, 1, 1))]))
    if sc.colors_precomp is not None:
        sc.colors_precomp = f32(np.concatenate([sc.colors_precomp, [[0.8, 0.3, 0.2], [0.1, 0.6, 0.9]]]))
    return sc


def loss_and_grads(scene, **kw):
    """(image, {leaf name: gradient of sum(dL_dout * image)}) in float64 numpy."""
    img, leaves = render(scene, **kw)
    loss = (img * torch.tensor(scene.dL_dout, dtype=torch.float64)).sum()
    names = list(leaves.keys())
    grads = torch.autograd.grad(loss, [leaves[n] for n in names], allow_unused=True)
    return img.detach().numpy(), {n: (None if g is None else g.detach().numpy()) for n, g in zip(names, grads)}
