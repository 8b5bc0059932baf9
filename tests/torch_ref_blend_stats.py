"""Float64 yardstick of the blend statistics: torch_ref.render's maths restated to return the N x P matrix of blend weights.

The blend weight of a (pixel, Gaussian) pair is w = alpha * T, T the pixel's transmittance in front of the blend (include/stp_raster.h:
stp_set_backward_blend_stats).  blend_stats[i] = (sum_p w[p, i], max_p w[p, i], #{p : pair (p, i) blended}) over the pairs the
rasterizer blends: alpha >= 1/255, in front of the entry whose blend would take the pixel's transmittance below 1e-4.

Same splatting maths as torch_ref.render (textbook EWA, alpha compositing in a per-pixel order), restated because the weights are not
reachable from outside; shares no code with the kernels or the oracle.  No autograd: the statistics do not depend on the loss.
Scales and rotations only (no precomputed covariance, no proper_ewa_scaling).
"""
from __future__ import annotations

import numpy as np
import torch

from torch_ref import quat_to_rot

ALPHA_MIN, T_MIN = 1.0 / 255.0, 1e-4
YARD_SEED = 9   # seed of the P = 150, 40 x 36 scene the kernels are compared on: at most 1 % of its Gaussians are marked `near` (see weights())


def weights(scene, order="global", depth_key="z"):
    """Returns a dict of float64 / bool tensors:
    w (N, P): the blend weight of every pair, 0 where the pair is not blended;  blended (N, P): the pairs;  T_final (N,);
    near (N, P): pairs whose membership hangs on a rounding -- a candidate whose alpha lies within 1e-6 of 1/255, or an entry reached
    by its pixel whose T * (1 - alpha) lies within 1e-6 (relative) of 1e-4."""
    dd = torch.float64
    t = lambda a: torch.tensor(np.asarray(a), dtype=dd)
    W, H = scene.W, scene.H
    V, PM, INV = t(scene.viewmatrix), t(scene.projmatrix), t(scene.inv_viewprojmatrix)
    cam = t(scene.campos)
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

    # binning: 3.33 sigma rectangle of tiles (no culling options here)
    mid = 0.5 * (a + c)
    radius = 3.33 * torch.sqrt(mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.01)))
    visible = near_ok & (det != 0) & (o >= ALPHA_MIN)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    x0, x1 = torch.clamp(torch.floor((mx - radius) / 16), 0, gx), torch.clamp(torch.ceil((mx + radius) / 16), 0, gx)
    y0, y1 = torch.clamp(torch.floor((my - radius) / 16), 0, gy), torch.clamp(torch.ceil((my + radius) / 16), 0, gy)
    visible &= ((x1 - x0) * (y1 - y0)) > 0

    ys, xs = torch.meshgrid(torch.arange(H, dtype=dd), torch.arange(W, dtype=dd), indexing="ij")
    px, py = xs.reshape(-1), ys.reshape(-1)             # N
    N = px.shape[0]
    dx = mx[None, :] - px[:, None]
    dy = my[None, :] - py[:, None]
    power = -0.5 * (cA[None] * dx * dx + cC[None] * dy * dy) - cB[None] * dx * dy
    G = torch.exp(torch.clamp(power, max=0.0))
    alpha = torch.clamp(o[None] * G, max=0.99)
    tx_, ty_ = torch.floor(px / 16), torch.floor(py / 16)
    in_rect = (tx_[:, None] >= x0[None]) & (tx_[:, None] < x1[None]) & (ty_[:, None] >= y0[None]) & (ty_[:, None] < y1[None])
    cand = in_rect & visible[None] & (power <= 0)
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
        cand = cand & (key >= 0)
    keep = cand & (alpha >= ALPHA_MIN)
    key = torch.where(keep, key, torch.full_like(key, float("inf")))
    idx = torch.argsort(key, dim=1, stable=True)
    keep_s = torch.gather(keep, 1, idx)
    a_s = torch.gather(torch.where(keep, alpha, torch.zeros_like(alpha)), 1, idx)
    one_m = 1 - a_s
    Tbefore = torch.cumprod(torch.cat([torch.ones(N, 1, dtype=dd), one_m[:, :-1]], 1), 1)
    test_T = Tbefore * one_m
    stops = torch.cumsum((test_T < T_MIN).to(torch.int64), 1)
    alive = stops == 0                                   # the first saturating entry ends the pixel
    blended_s = alive & keep_s
    w_s = torch.where(blended_s, a_s * Tbefore, torch.zeros_like(a_s))
    T_final = torch.where(alive, one_m, torch.ones_like(one_m)).prod(1)
    # an entry is REACHED if no entry in front of it saturated the pixel (the saturating entry itself is reached)
    reached_s = keep_s & ((stops - (test_T < T_MIN).to(torch.int64)) == 0)
    near_T_s = reached_s & ((test_T - T_MIN).abs() <= 1e-6 * T_MIN)
    unsort = lambda m: torch.zeros_like(m).scatter(1, idx, m)
    near = (cand & ((alpha - ALPHA_MIN).abs() <= 1e-6)) | unsort(near_T_s)
    return {"w": unsort(w_s), "blended": unsort(blended_s), "T_final": T_final, "near": near}


_cache = {}


def blend_stats(scene, order="global", depth_key="z", key=None):
    """(stats (P, 3), explained (P,) bool, T_final (N,)) as numpy arrays (float64 / bool): per Gaussian the sum, the maximum and the count
    of its blend weights, and whether a pair of its hangs on a rounding (see weights()).  key: a hashable name under which the (read-only)
    result is kept for the other tests of the session that need the same scene and order."""
    if key is not None and key in _cache:
        return _cache[key]
    r = weights(scene, order=order, depth_key=depth_key)
    w = r["w"]
    stats = torch.stack([w.sum(0), w.max(0).values, r["blended"].sum(0).to(torch.float64)], 1)
    out = (stats.numpy(), r["near"].any(0).numpy(), r["T_final"].numpy())
    for arr in out:
        arr.setflags(write=False)
    if key is not None:
        _cache[key] = out
    return out
