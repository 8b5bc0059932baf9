"""Float64 autograd yardstick of absgrad: torch_ref.render's maths with the per-pixel screen offsets as a leaf.

absgrad[i] = (sum_p |g_x,p(i)|, sum_p |g_y,p(i)|, 0), where g_p(i) is what pixel p adds to dL/dmeans2D[i] (include/stp_raster.h:
stp_set_backward_absgrad).  A Gaussian's 2D mean reaches pixel p only through the offsets dx[p, i] = mx[i] - px, dy[p, i] = my[i] - py,
so with an N x P leaf added to each offset matrix, dL/d(dx[p, i]) IS pixel p's contribution in pixel units, and the NDC shift that
means2D stands for (torch_ref.render: mx = ((ndc + 1) W - 1) / 2) scales it by W / 2 (H / 2 for y):

    absgrad_x[i] = 0.5 W sum_p |dL/d(dx[p, i])|        means2D.grad_x[i] = 0.5 W sum_p dL/d(dx[p, i])

Same splatting maths as torch_ref.render (textbook EWA, real SH basis, alpha compositing in a per-pixel order), restated because the
offsets are not reachable from outside; shares no code with the kernels or the oracle.  Scales and rotations only (no precomputed
covariance, no proper_ewa_scaling): the offsets' path does not depend on either.
"""
from __future__ import annotations

import numpy as np
import torch

from torch_ref import eval_sh, quat_to_rot


def render(scene, order="global", depth_key="z"):
    """Returns (image (3,H,W) float64 tensor, (ddx, ddy)): the two N x P zero leaves added to the offset matrices."""
    dd = torch.float64
    t = lambda a: torch.tensor(np.asarray(a), dtype=dd)
    W, H = scene.W, scene.H
    V, PM, INV = t(scene.viewmatrix), t(scene.projmatrix), t(scene.inv_viewprojmatrix)
    cam, bg = t(scene.campos), t(scene.bg)
    means, opac, scales, rots = t(scene.means3D), t(scene.opacities), t(scene.scales), t(scene.rotations)
    P = means.shape[0]

    Rm = quat_to_rot(rots)
    Sigma = Rm @ torch.diag_embed((scene.scale_modifier * scales) ** 2) @ Rm.transpose(1, 2)
    pv = means @ V[:3, :3] + V[3, :3]
    tz = pv[:, 2]
    near_ok = tz > 0.2
    fx, fy = W / (2 * scene.tanfovx), H / (2 * scene.tanfovy)
    limx, limy = 1.3 * scene.tanfovx, 1.3 * scene.tanfovy
    txc = torch.clamp(pv[:, 0] / tz, -limx, limx) * tz
    tyc = torch.clamp(pv[:, 1] / tz, -limy, limy) * tz
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -fx * txc / (tz * tz), zero, fy / tz, -fy * tyc / (tz * tz)], 1).reshape(-1, 2, 3)
    JW = J @ V[:3, :3].T
    cov2 = JW @ Sigma @ JW.transpose(1, 2)
    a, b, c = cov2[:, 0, 0] + 0.3, cov2[:, 0, 1], cov2[:, 1, 1] + 0.3
    det = a * c - b * b
    o = opac[:, 0]
    cA, cB, cC = c / det, -b / det, a / det

    ph = torch.cat([means, torch.ones(P, 1, dtype=dd)], 1) @ PM
    ndc = ph[:, :2] / (ph[:, 3:4] + 1e-7)
    mx = ((ndc[:, 0] + 1) * W - 1) * 0.5
    my = ((ndc[:, 1] + 1) * H - 1) * 0.5

    if scene.shs is not None:
        d = means - cam
        col = torch.clamp(eval_sh(scene.sh_degree, t(scene.shs), d / d.norm(dim=1, keepdim=True)), min=0.0)
    else:
        col = t(scene.colors_precomp)

    # binning: 3.33 sigma rectangle of tiles (no culling options here)
    mid = 0.5 * (a + c)
    radius = 3.33 * torch.sqrt(mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.01)))
    visible = near_ok & (det != 0) & (o >= 1.0 / 255.0)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    x0, x1 = torch.clamp(torch.floor((mx - radius) / 16), 0, gx), torch.clamp(torch.ceil((mx + radius) / 16), 0, gx)
    y0, y1 = torch.clamp(torch.floor((my - radius) / 16), 0, gy), torch.clamp(torch.ceil((my + radius) / 16), 0, gy)
    visible &= ((x1 - x0) * (y1 - y0)) > 0

    ys, xs = torch.meshgrid(torch.arange(H, dtype=dd), torch.arange(W, dtype=dd), indexing="ij")
    px, py = xs.reshape(-1), ys.reshape(-1)             # N
    N = px.shape[0]
    ddx = torch.zeros(N, P, dtype=dd, requires_grad=True)   # the leaves: one offset per (pixel, Gaussian) pair
    ddy = torch.zeros(N, P, dtype=dd, requires_grad=True)
    dx = mx[None, :] - px[:, None] + ddx
    dy = my[None, :] - py[:, None] + ddy
    power = -0.5 * (cA[None] * dx * dx + cC[None] * dy * dy) - cB[None] * dx * dy
    G = torch.exp(torch.clamp(power, max=0.0))
    alpha = torch.clamp(o[None] * G, max=0.99)
    with torch.no_grad():
        tx_, ty_ = torch.floor(px / 16), torch.floor(py / 16)
        in_rect = (tx_[:, None] >= x0[None]) & (tx_[:, None] < x1[None]) & (ty_[:, None] >= y0[None]) & (ty_[:, None] < y1[None])
        keep = in_rect & visible[None] & (power <= 0) & (alpha >= 1.0 / 255.0)
        if order == "global":
            key = (tz if depth_key == "z" else (means - cam).norm(dim=1))[None].expand(N, P)
        else:
            # depth along each pixel's ray: (Sigma^-1 (mu - cam)) . v / (v^T Sigma^-1 v)
            s_cl = torch.clamp(scales, min=1e-3) * scene.scale_modifier
            Sinv = Rm @ torch.diag_embed(1.0 / (s_cl ** 2)) @ Rm.transpose(1, 2)
            ndcx, ndcy = px * (2.0 / W) - 1.0, py * (2.0 / H) - 1.0
            pw = ndcx[:, None] * INV[0][None] + ndcy[:, None] * INV[1][None] + INV[3][None]
            v = pw[:, :3] / pw[:, 3:4] - cam
            v = v / v.norm(dim=1, keepdim=True)            # N x 3
            num = v @ torch.einsum("pij,pj->pi", Sinv, means - cam).T
            den = torch.einsum("ni,pij,nj->np", v, Sinv, v)
            key = num / torch.clamp(den, min=1e-5)
            keep &= key >= 0
        key = torch.where(keep, key, torch.full_like(key, float("inf")))
        idx = torch.argsort(key, dim=1, stable=True)
    a_s = torch.gather(torch.where(keep, alpha, torch.zeros_like(alpha)), 1, idx)
    one_m = 1 - a_s
    Tbefore = torch.cumprod(torch.cat([torch.ones(N, 1, dtype=dd), one_m[:, :-1]], 1), 1)
    with torch.no_grad():
        alive = torch.cumsum(((Tbefore * one_m) < 1e-4).to(torch.int64), 1) == 0   # the first saturating entry ends the pixel
    wgt = torch.where(alive, a_s * Tbefore, torch.zeros_like(a_s))
    C = (wgt[..., None] * col[idx]).sum(1)
    T_final = torch.where(alive, one_m, torch.ones_like(one_m)).prod(1)
    img = C + T_final[:, None] * bg[None]
    return img.T.reshape(3, H, W), (ddx, ddy)


_cache = {}


def absgrad(scene, order="global", depth_key="z", key=None):
    """(image, absgrad (P, 2), signed (P, 2)) as float64 numpy arrays for the loss sum(scene.dL_dout * image): the sums over pixels of
    the absolute and of the signed per-pixel contributions, both in means2D's units.  key: a hashable name under which the (read-only)
    result is kept for the other tests of the session that need the same scene and order."""
    if key is not None and key in _cache:
        return _cache[key]
    img, (ddx, ddy) = render(scene, order=order, depth_key=depth_key)
    loss = (img * torch.tensor(scene.dL_dout, dtype=torch.float64)).sum()
    gx, gy = torch.autograd.grad(loss, [ddx, ddy])
    sx, sy = 0.5 * scene.W, 0.5 * scene.H
    out = (img.detach().numpy(),
           torch.stack([sx * gx.abs().sum(0), sy * gy.abs().sum(0)], 1).numpy(),
           torch.stack([sx * gx.sum(0), sy * gy.sum(0)], 1).numpy())
    for arr in out:
        arr.setflags(write=False)
    if key is not None:
        _cache[key] = out
    return out
