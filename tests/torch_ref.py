"""Independent float64 PyTorch reference of the differentiable splatting maths (dense, tiny scenes).

This is NOT the oracle and shares no code with it or with the HIP kernels: it is written from the
textbook formulation (Sigma = R S^2 R^T, EWA projection J W Sigma W^T J^T, real SH basis, alpha
compositing with a per-pixel order) and differentiated by torch.autograd.  It pins the *value and
gradient maths* of oracle and kernels; discrete behaviour (tile binning, queue cadence) is pinned
elsewhere.  Ordering modes: "global" (sort by the global depth key) and "exact" (sort by each
pixel's own depth-along-ray, i.e. what the resorting modes converge to at low density).

One dense renderer, render_core(), serves every float64 yardstick of the tests: render() / loss_and_grads() here, and through its hooks
the camera gradients (torch_ref_camera.py), absgrad (torch_ref_absgrad.py), the blend statistics (torch_ref_blend_stats.py) and the
per-Gaussian bound on the colour gradient (torch_ref_colour_bound.py).  A further yardstick is a further hook, not a copy;
tests/test_yardstick_pin_cpu.py holds the first four to recorded values, tests/test_upstream_grad_cpu.py the fifth.  The part of it that
sees one Gaussian at a time is per_gaussian(), on which torch_ref_per_gaussian.py differentiates the per-Gaussian backward alone.
"""
from __future__ import annotations

import math

import numpy as np
import torch

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
SH_C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435]


def quat_to_rot(q):
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    return R  # textbook rotation matrix (row-major)


def eval_sh(deg, sh, dirs):
    x, y, z = dirs[:, 0:1], dirs[:, 1:2], dirs[:, 2:3]
    res = SH_C0 * sh[:, 0]
    if deg > 0:
        res = res - SH_C1 * y * sh[:, 1] + SH_C1 * z * sh[:, 2] - SH_C1 * x * sh[:, 3]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        res = (res + SH_C2[0] * xy * sh[:, 4] + SH_C2[1] * yz * sh[:, 5] + SH_C2[2] * (2 * zz - xx - yy) * sh[:, 6]
               + SH_C2[3] * xz * sh[:, 7] + SH_C2[4] * (xx - yy) * sh[:, 8])
    if deg > 2:
        res = (res + SH_C3[0] * y * (3 * xx - yy) * sh[:, 9] + SH_C3[1] * xy * z * sh[:, 10]
               + SH_C3[2] * y * (4 * zz - xx - yy) * sh[:, 11] + SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[:, 12]
               + SH_C3[4] * x * (4 * zz - xx - yy) * sh[:, 13] + SH_C3[5] * z * (xx - yy) * sh[:, 14]
               + SH_C3[6] * x * (xx - 3 * yy) * sh[:, 15])
    return res + 0.5


def per_gaussian(scene, proper_ewa_scaling=False, use_cov3D_precomp=False, camera_leaves=False, dtype=torch.float64, hooks=None):
    """The per-Gaussian part of render_core, from the leaves to what the render half reads of a Gaussian: the NDC mean, the conic, the
    opacity actually blended (with the proper_ewa_scaling factor) and the colour.  Returns (dict of leaf tensors with requires_grad, dict
    of intermediates "ndc" (P,2), "conic" (three (P,) tensors: xx, xy, yy), "opacity" (P,), "colour" (P,3) and what render_core and
    torch_ref_per_gaussian.py read besides).  No pixel enters, and no Gaussian reads another's row.
    dtype: float64 for every yardstick; torch_ref_per_gaussian.py also evaluates this function in float32 to measure what float32 can do.
    hooks: None for every yardstick of render_core.  torch_ref_per_gaussian.py passes the rasterizer's two conventions that are not
    plain derivatives: "conic" (a function of the three conic entries and det) and "ewa_factor" (of a0, b0, c0, a, c); its scale() reads
    the view matrix through "view_in_covariance" where it enters the covariance, to tell that path from the one through the mean."""
    hooks = hooks or {}
    dd = dtype
    t = lambda a: torch.tensor(np.asarray(a), dtype=dd)
    W, H = scene.W, scene.H
    V, PM, INV = t(scene.viewmatrix), t(scene.projmatrix), t(scene.inv_viewprojmatrix)
    cam, bg = t(scene.campos), t(scene.bg)
    leaves = {}
    if camera_leaves:
        leaves.update(viewmatrix=V.requires_grad_(True), projmatrix=PM.requires_grad_(True), campos=cam.requires_grad_(True))
    means = t(scene.means3D).requires_grad_(True); leaves["means3D"] = means
    opac = t(scene.opacities).requires_grad_(True); leaves["opacities"] = opac
    scales = t(scene.scales).requires_grad_(True); leaves["scales"] = scales
    rots = t(scene.rotations).requires_grad_(True); leaves["rotations"] = rots
    P = means.shape[0]
    ndc_shift = torch.zeros(P, 2, dtype=dd, requires_grad=True); leaves["means2D"] = ndc_shift

    Rm = quat_to_rot(rots)
    Sd = torch.diag_embed((scene.scale_modifier * scales) ** 2)
    Sigma = Rm @ Sd @ Rm.transpose(1, 2)
    if use_cov3D_precomp:
        c6 = torch.stack([Sigma[:, 0, 0], Sigma[:, 0, 1], Sigma[:, 0, 2], Sigma[:, 1, 1], Sigma[:, 1, 2], Sigma[:, 2, 2]], 1)
        if "cov3D_precomp" in scene.meta:   # the very array a caller passed, not the float64 one of the same Gaussians
            c6 = t(scene.meta["cov3D_precomp"])
        c6 = c6.detach().clone().requires_grad_(True); leaves["cov3D_precomp"] = c6
        Sigma_used = torch.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]], 1).reshape(-1, 3, 3)
    else:
        Sigma_used = Sigma

    pv = means @ V[:3, :3] + V[3, :3]                  # view-space means (row-vector convention)
    tz = pv[:, 2]
    fx, fy = W / (2 * scene.tanfovx), H / (2 * scene.tanfovy)
    limx, limy = 1.3 * scene.tanfovx, 1.3 * scene.tanfovy
    if camera_leaves:
        with torch.no_grad():
            rx, ry = pv[:, 0] / tz, pv[:, 1] / tz
            in_x, in_y = (rx >= -limx) & (rx <= limx), (ry >= -limy) & (ry <= limy)
            cx, cy = torch.clamp(rx, -limx, limx) * tz, torch.clamp(ry, -limy, limy) * tz
        txc = torch.where(in_x, pv[:, 0], cx)
        tyc = torch.where(in_y, pv[:, 1], cy)
    else:
        txc = torch.clamp(pv[:, 0] / tz, -limx, limx) * tz
        tyc = torch.clamp(pv[:, 1] / tz, -limy, limy) * tz
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -fx * txc / (tz * tz), zero, fy / tz, -fy * tyc / (tz * tz)], 1).reshape(-1, 2, 3)
    Wm = (hooks["view_in_covariance"](V) if "view_in_covariance" in hooks else V)[:3, :3].T  # p_view = Wm p + t
    JW = J @ Wm
    cov2 = JW @ Sigma_used @ JW.transpose(1, 2)
    a0, b0, c0 = cov2[:, 0, 0], cov2[:, 0, 1], cov2[:, 1, 1]
    a, b, c = a0 + 0.3, b0, c0 + 0.3
    det = a * c - b * b
    o = opac[:, 0]
    if proper_ewa_scaling and "ewa_factor" in hooks:
        o = o * hooks["ewa_factor"](a0, b0, c0, a, c)
    elif proper_ewa_scaling:
        o = o * torch.sqrt(torch.clamp((a0 * c0 - b0 * b0) / det, min=0.000025))
    cA, cB, cC = c / det, -b / det, a / det
    if "conic" in hooks:
        cA, cB, cC = hooks["conic"](cA, cB, cC, det)

    ph = torch.cat([means, torch.ones(P, 1, dtype=dd)], 1) @ PM
    ndc = ph[:, :2] / (ph[:, 3:4] + 1e-7) + ndc_shift
    mx = ((ndc[:, 0] + 1) * W - 1) * 0.5
    my = ((ndc[:, 1] + 1) * H - 1) * 0.5

    if scene.shs is not None:
        shs = t(scene.shs).requires_grad_(True); leaves["shs"] = shs
        d = means - cam
        d = d / d.norm(dim=1, keepdim=True)
        col = torch.clamp(eval_sh(scene.sh_degree, shs, d), min=0.0)
    else:
        col = t(scene.colors_precomp).requires_grad_(True); leaves["colors_precomp"] = col

    return leaves, dict(ndc=ndc, conic=(cA, cB, cC), opacity=o, colour=col, means=means, scales=scales, Rm=Rm, Sigma=Sigma, pv=pv,
                        a=a, c=c, det=det, mx=mx, my=my, cam=cam, bg=bg, INV=INV)


def render_core(scene, order="global", proper_ewa_scaling=False, use_cov3D_precomp=False, depth_key="z", camera_leaves=False,
                offset_leaves=False):
    """The one dense renderer.  Returns (image (3,H,W) float64 tensor, dict of leaf tensors with requires_grad, details).

    camera_leaves: viewmatrix, projmatrix and campos are leaves too (torch_ref_camera.py), with two conventions where the camera enters:
      * the three camera tensors are INDEPENDENT leaves, as the rasterizer reads them (it never checks that projmatrix = viewmatrix @ P
        or that campos is the camera centre); culling, tile binning and every sort key see the detached camera;
      * the 1.3 * tan_fov clamp of the view-space mean inside the EWA Jacobian is differentiated as the rasterizer differentiates it for
        means3D (the reference's backward.cu): a clamped coordinate is a constant -- it carries no gradient to the view-space mean, and
        its value enters J as a number.  Without the switch clamp(x / z) * z is differentiated, which also moves with z; the two agree
        for every Gaussian inside the band, where the switch puts x itself into J and not (x / z) * z: an ulp or two on the image.
    offset_leaves: two N x P zero leaves, "offsets_x" and "offsets_y", are added to the pixel offsets dx, dy (torch_ref_absgrad.py).
    details: what torch_ref_blend_stats.py reads, without gradients.  Per (pixel, Gaussian) pair, N x P in the Gaussians' own order:
    "w" the blend weight alpha * T (0 where the pair is not blended), "blended", "cand" (a candidate: in the tile rectangle, visible,
    power <= 0 and, in the exact order, not behind the camera -- whatever its alpha) and "alpha"; in each pixel's sorted order, with the
    sort index "idx": "test_T" = T * (1 - alpha) and "reached" (no entry in front of it saturated the pixel; the saturating entry
    itself is reached); "T_final" (N,).  And, WITH their graph, "per_gaussian": per_gaussian()'s intermediates, through which alone
    the image depends on the leaves (torch_ref_per_gaussian.py)."""
    dd = torch.float64
    leaves, pg = per_gaussian(scene, proper_ewa_scaling, use_cov3D_precomp, camera_leaves)
    means, scales, Rm, cam, bg, INV = pg["means"], pg["scales"], pg["Rm"], pg["cam"], pg["bg"], pg["INV"]
    (cA, cB, cC), o, col, tz = pg["conic"], pg["opacity"], pg["colour"], pg["pv"][:, 2]
    a, c, det, mx, my = pg["a"], pg["c"], pg["det"], pg["mx"], pg["my"]
    W, H, P = scene.W, scene.H, means.shape[0]
    near_ok = (tz > 0.2).detach()

    # binning, non-differentiable: 3.33 sigma rectangle of tiles (no culling options here)
    with torch.no_grad():
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
    px, py = xs.reshape(-1), ys.reshape(-1)             # N
    dx = mx[None, :] - px[:, None]                      # N x P
    dy = my[None, :] - py[:, None]
    if offset_leaves:   # one offset per (pixel, Gaussian) pair
        leaves["offsets_x"] = torch.zeros(px.shape[0], P, dtype=dd, requires_grad=True)
        leaves["offsets_y"] = torch.zeros(px.shape[0], P, dtype=dd, requires_grad=True)
        dx, dy = dx + leaves["offsets_x"], dy + leaves["offsets_y"]
    power = -0.5 * (cA[None] * dx * dx + cC[None] * dy * dy) - cB[None] * dx * dy
    G = torch.exp(torch.clamp(power, max=0.0))
    alpha = torch.clamp(o[None] * G, max=0.99)
    with torch.no_grad():   # per-pixel order: non-differentiable
        tx_, ty_ = torch.floor(px / 16), torch.floor(py / 16)
        in_rect = (tx_[:, None] >= x0[None]) & (tx_[:, None] < x1[None]) & (ty_[:, None] >= y0[None]) & (ty_[:, None] < y1[None])
        cand = in_rect & visible[None] & (power <= 0)
        if order == "global":
            key = (tz if depth_key == "z" else (means - cam).norm(dim=1))[None].expand(px.shape[0], P)
        else:
            # depth along each pixel's ray: (Sigma^-1 (mu - cam)) . v / (v^T Sigma^-1 v)
            s_cl = torch.clamp(scales, min=1e-3) * scene.scale_modifier
            Sinv = Rm @ torch.diag_embed(1.0 / (s_cl ** 2)) @ Rm.transpose(1, 2)
            ndcx, ndcy = px * (2.0 / W) - 1.0, py * (2.0 / H) - 1.0
            pw = ndcx[:, None] * INV[0][None] + ndcy[:, None] * INV[1][None] + INV[3][None]
            pw = pw[:, :3] / pw[:, 3:4]
            v = pw - cam
            v = v / v.norm(dim=1, keepdim=True)            # N x 3
            u = torch.einsum("pij,pj->pi", Sinv, means - cam)
            num = v @ u.T                                   # N x P
            den = torch.einsum("ni,pij,nj->np", v, Sinv, v)
            key = num / torch.clamp(den, min=1e-5)
            cand &= key >= 0
        keep = cand & (alpha >= 1.0 / 255.0)
        key = torch.where(keep, key, torch.full_like(key, float("inf")))
        idx = torch.argsort(key, dim=1, stable=True)
    a_s = torch.gather(torch.where(keep, alpha, torch.zeros_like(alpha)), 1, idx)
    one_m = 1 - a_s
    Tbefore = torch.cumprod(torch.cat([torch.ones(a_s.shape[0], 1, dtype=dd), one_m[:, :-1]], 1), 1)
    with torch.no_grad():
        test_T = Tbefore * one_m
        stop = test_T < 1e-4                              # first saturating entry ends the pixel
        stops = torch.cumsum(stop.to(torch.int64), 1)
        alive = stops == 0
    wgt = torch.where(alive, a_s * Tbefore, torch.zeros_like(a_s))
    col_s = col[idx]                                      # N x P x 3
    C = (wgt[..., None] * col_s).sum(1)
    T_final = torch.where(alive, one_m, torch.ones_like(one_m)).prod(1)
    img = C + T_final[:, None] * bg[None]
    with torch.no_grad():
        keep_s = torch.gather(keep, 1, idx)
        unsort = lambda m: torch.zeros_like(m).scatter(1, idx, m)
        details = {"w": unsort(wgt), "blended": unsort(alive & keep_s), "cand": cand, "alpha": alpha.detach(), "idx": idx,
                   "test_T": test_T, "reached": keep_s & ((stops - stop.to(torch.int64)) == 0), "T_final": T_final.detach()}
    details["per_gaussian"] = pg
    return img.T.reshape(3, H, W), leaves, details


def render(scene, order="global", proper_ewa_scaling=False, use_cov3D_precomp=False, depth_key="z"):
    """Returns (image (3,H,W) float64 tensor, dict of leaf tensors with requires_grad)."""
    return render_core(scene, order, proper_ewa_scaling, use_cov3D_precomp, depth_key)[:2]


def loss_and_grads(scene, **kw):
    """(image, {leaf name: gradient of sum(dL_dout * image)}) in float64 numpy; kw: render_core's."""
    img, leaves, _ = render_core(scene, **kw)
    w = torch.tensor(scene.dL_dout, dtype=torch.float64)
    loss = (img * w).sum()
    names = list(leaves.keys())
    grads = torch.autograd.grad(loss, [leaves[n] for n in names], allow_unused=True)
    out = {n: (None if g is None else g.detach().numpy()) for n, g in zip(names, grads)}
    return img.detach().numpy(), out


_cache = {}


def cached(name, key, make):
    """make()'s tuple of numpy arrays, made read-only.  key: a hashable name under which the result is kept, per yardstick `name`, for the
    other tests of the session that need the same scene and order (None: not kept)."""
    if key is not None and (name, key) in _cache:
        return _cache[name, key]
    out = make()
    for arr in out:
        arr.setflags(write=False)
    if key is not None:
        _cache[name, key] = out
    return out
