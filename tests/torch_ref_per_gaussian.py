"""Float64 yardstick of the per-Gaussian backward ALONE (csrc/stp_backward.hip: preprocess_backward_kernel), Gaussian by Gaussian.

The per-Gaussian half maps a Gaussian's gradient record -- nine sums of the render half, in the record's order (include/stp_raster.h):
colour r g b, mean2D x y in NDC units, conic xx xy yy, opacity -- to its rows of dL_dmeans3D, dL_dscales, dL_drotations, dL_dsh,
dL_dcov3D, dL_dopacity and to its share of the three camera gradients.  Given the records it is a smooth function of one Gaussian, with no
sum across threads but the camera's.  vjp() differentiates the same map with torch.autograd on torch_ref.per_gaussian(), the part of the one
dense renderer that sees one Gaussian at a time: the gradient of sum(records * slots), for records the caller chooses.  No pixel, no
summation order and no threshold of the render half enters.

Conventions of the rasterizer (the reference's backward.cu, which the kernel and the oracle reproduce) that are not plain derivatives, each
behind an argument of vjp() that is off by default -- with all of them off vjp() is plain autograd on per_gaussian(), and fed with the
cotangents of a whole render it returns torch_ref.loss_and_grads (tests/test_per_gaussian_cpu.py):

  conic_xy_half   the record's conic-xy slot is HALF the cotangent of the conic's off-diagonal entry (the render half adds 0.5 * ..., the
                  per-Gaussian half multiplies by 2): the slot that meets the record is 2 * conic_xy.
  inv_det_eps     the derivative of 1 / det is taken as -1 / (det^2 + 1e-7).  backward.cu factors 1 / det^2 out of all three derivatives
                  of the conic (denom2inv), so the whole Jacobian d(conic) / d(a, b, c) is the true one times det^2 / (det^2 + 1e-7): a
                  gradient-scaling torch.autograd.Function of five lines.  For a sub-pixel Gaussian, det about 0.09, that is 1.2e-5 of the
                  gradient: above float32 rounding, so it is modelled here and not absorbed by a tolerance.
  ewa_closed_form under proper_ewa_scaling the gradient of the opacity factor sqrt(det(cov) / det(cov + 0.3 I)) with respect to the 2D
                  covariance is the reference's closed form evaluated with the DILATED diagonal (tests/test_oracle_cpu.py::
                  test_oracle_ewa_scaling_gradient_quirk), restated below in float64.
  scale_modifier_omitted   dL_dscales is the derivative with respect to scale_modifier * scales (tests/test_camera_model_cpu.py::
                  test_dL_dscales_omits_scale_modifier_like_the_reference).
  clamp_constant  a view-space coordinate clamped to the 1.3 tan_fov band is a constant (torch_ref.render_core(camera_leaves=True)).

kernel=True switches all five on.

The measure.  scale() returns per Gaussian and output tensor S = max over the row of sum_k |record_k| |d slot_k / d entry| (nine one-slot
VJPs), and ratio() = max over the row of |got - float64| / S.  Dividing by S makes the measure blind to cancellation BETWEEN slots;
dividing by the row's largest S and not entry by entry is deliberate: cancellation inside one slot's Jacobian (dL_dscales of an anisotropic
Gaussian) makes an entrywise bound thousands of u wide.

The tolerance T[family][tensor] is measured, not chosen: 4 x the worst ratio of THIS module evaluated in float32 on the CPU (dtype=
torch.float32, the same inputs and records; never the kernel), over the family's record kinds, rounded up to two digits, floor
16 * 2^-24.  The factor 4 is tests/test_gpu_upstream_grad.py's margin of the kernel over its CPU model: another legitimate evaluation order
and -ffp-contract=fast.  No entry may exceed 2e-3.  tests/test_per_gaussian_cpu.py re-measures it; tests/test_gpu_per_gaussian.py holds
the kernel to it.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import torch_ref
from diff_gaussian_rasterization import scenes

SLOTS = ("colour r", "colour g", "colour b", "mean2D x", "mean2D y", "conic xx", "conic xy", "conic yy", "opacity")
CAMERA = ("dL_dview", "dL_dproj", "dL_dcam")
MEASURED = ("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dsh", "dL_dcov3D", "dL_dopacity")
FLOOR = 16 * 2.0 ** -24
CAP = 2e-3


class _ScaleGrad(torch.autograd.Function):
    """x, with its gradient multiplied by k"""
    @staticmethod
    def forward(ctx, x, k):
        ctx.save_for_backward(k)
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None


def _conic_hook(cA, cB, cC, det):
    k = (det * det / (det * det + 1e-7)).detach()
    return _ScaleGrad.apply(cA, k), _ScaleGrad.apply(cB, k), _ScaleGrad.apply(cC, k)


class _EwaFactor(torch.autograd.Function):
    """sqrt(max(det(cov) / det(cov + 0.3 I), 0.000025)); backward: the reference's closed form, with x, y the dilated diagonal entries."""
    @staticmethod
    def forward(ctx, a0, b0, c0, a, c):
        ratio = (a0 * c0 - b0 * b0) / (a * c - b0 * b0)
        h = torch.sqrt(torch.clamp(ratio, min=0.000025))
        ctx.save_for_backward(ratio, h, b0, a, c)
        return h

    @staticmethod
    def backward(ctx, g):
        ratio, h, z, x, y = ctx.saved_tensors
        w = 0.3
        qd = w * w + w * (x + y) + x * y - z * z
        f = torch.where(ratio <= 0.000025, torch.zeros_like(g), g / (2 * h)) / (qd * qd)
        return w * (w * y + y * y + z * z) * f, -2.0 * w * z * (w + x + y) * f, w * (w * x + x * x + z * z) * f, None, None


def _switches(kernel, camera_leaves, **given):
    sw = {n: (bool(kernel) if v is None else bool(v)) for n, v in given.items()}
    sw["clamp_constant"] = sw["clamp_constant"] or bool(camera_leaves)
    return sw


def _graph(scene, visible, sw, proper_ewa_scaling, use_cov3D_precomp, dtype, hooks=None):
    """(leaves, slots (P, 9) with the graph, Sigma, boolean mask of the rows that count)"""
    hooks = dict(hooks or {})
    if sw["inv_det_eps"]:
        hooks["conic"] = _conic_hook
    if sw["ewa_closed_form"]:
        hooks["ewa_factor"] = _EwaFactor.apply
    leaves, pg = torch_ref.per_gaussian(scene, proper_ewa_scaling, use_cov3D_precomp, camera_leaves=sw["clamp_constant"], dtype=dtype,
                                        hooks=hooks)
    cA, cB, cC = pg["conic"]
    slots = torch.cat([pg["colour"], pg["ndc"], torch.stack([cA, (2.0 if sw["conic_xy_half"] else 1.0) * cB, cC, pg["opacity"]], 1)], 1)
    vis = torch.ones(slots.shape[0], dtype=torch.bool) if visible is None else torch.as_tensor(np.asarray(visible), dtype=torch.bool)
    return leaves, slots, pg["Sigma"], vis


def _named(scene, leaves, Sigma, grads, sw, camera, use_cov3D_precomp):
    """autograd's gradients (of the leaves in their order, then of Sigma) under the names of the backward's outputs"""
    g = dict(zip(list(leaves) + ["Sigma"], grads))
    z = lambda n: torch.zeros_like(leaves[n]) if g.get(n) is None else g[n]
    out = {"dL_dmeans3D": z("means3D"), "dL_dmeans2D": z("means2D"), "dL_dopacity": z("opacities")}
    if use_cov3D_precomp:
        out["dL_dcov3D"] = z("cov3D_precomp")
    else:
        G = g["Sigma"] if g.get("Sigma") is not None else torch.zeros_like(Sigma)
        out["dL_dcov3D"] = torch.stack([G[..., 0, 0], G[..., 0, 1] + G[..., 1, 0], G[..., 0, 2] + G[..., 2, 0], G[..., 1, 1],
                                        G[..., 1, 2] + G[..., 2, 1], G[..., 2, 2]], -1)
        out["dL_dscales"] = z("scales") / (scene.scale_modifier if sw["scale_modifier_omitted"] else 1.0)
        out["dL_drotations"] = z("rotations")
    if "shs" in leaves:
        out["dL_dsh"] = z("shs")
    else:
        out["dL_dcolors"] = z("colors_precomp")
    if camera:
        out.update(dL_dview=z("viewmatrix"), dL_dproj=z("projmatrix"), dL_dcam=z("campos"))
    return out


def vjp(scene, records, visible=None, *, kernel=False, conic_xy_half=None, inv_det_eps=None, ewa_closed_form=None,
        scale_modifier_omitted=None, clamp_constant=None, proper_ewa_scaling=False, use_cov3D_precomp=False, camera_leaves=False,
        dtype=torch.float64):
    """{output name: gradient of sum(records * slots) over the rows of `visible` (None: all)}, numpy arrays of `dtype`, under the names of
    the backward's outputs: dL_dmeans3D (P,3), dL_dmeans2D (P,2, NDC), dL_dopacity (P,1), dL_dcov3D (P,6: the leaf with
    use_cov3D_precomp, else the gradient of the covariance built from scales and rotations, as the kernel reports it), dL_dscales,
    dL_drotations (without use_cov3D_precomp), dL_dsh (P,M,3) or dL_dcolors (a scene with colors_precomp), and with camera_leaves
    dL_dview, dL_dproj, dL_dcam (camera_leaves implies clamp_constant, torch_ref.render_core's convention).
    records: (P, 9); rows outside `visible` may hold anything (NaN), their gradient rows are zeros."""
    sw = _switches(kernel, camera_leaves, conic_xy_half=conic_xy_half, inv_det_eps=inv_det_eps, ewa_closed_form=ewa_closed_form,
                   scale_modifier_omitted=scale_modifier_omitted, clamp_constant=clamp_constant)
    leaves, slots, Sigma, vis = _graph(scene, visible, sw, proper_ewa_scaling, use_cov3D_precomp, dtype)
    rec = torch.as_tensor(np.asarray(records), dtype=dtype)
    loss = (rec[vis] * slots[vis]).sum()
    targets = list(leaves.values()) + ([] if use_cov3D_precomp else [Sigma])
    grads = torch.autograd.grad(loss, targets, allow_unused=True)
    res = {}
    for n, a in _named(scene, leaves, Sigma, grads, sw, camera_leaves, use_cov3D_precomp).items():
        a = a.detach().clone()
        if n not in CAMERA:
            a[~vis] = 0
        res[n] = a.numpy()
    return res


def scale(scene, records, visible=None, *, kernel=False, conic_xy_half=None, inv_det_eps=None, ewa_closed_form=None,
          scale_modifier_omitted=None, clamp_constant=None, proper_ewa_scaling=False, use_cov3D_precomp=False, camera_leaves=False):
    """{output name: S}: per Gaussian tensor (P,) the largest entry of the row of sum_k |record_k| |d slot_k / d entry|, from nine
    one-slot VJPs in float64 (0 for rows outside `visible`); per camera tensor, in its own shape, the sum of that over the visible
    Gaussians, entry by entry.  The view matrix enters a Gaussian twice, through the view-space mean and through the rotation of its
    covariance, and the two derivatives can cancel exactly (with an identity view, d conic / d view[2][0] is zero for every Gaussian:
    the shear of the mean undoes the shear of the covariance): the scale of an entry of dL_dview is the sum of the absolute values of
    BOTH, or a structural zero would be held to a bound of zero."""
    sw = _switches(kernel, camera_leaves, conic_xy_half=conic_xy_half, inv_det_eps=inv_det_eps, ewa_closed_form=ewa_closed_form,
                   scale_modifier_omitted=scale_modifier_omitted, clamp_constant=clamp_constant)
    second = {}

    def view_in_covariance(V):
        second["viewmatrix"] = V.detach().clone().requires_grad_(True)
        return second["viewmatrix"]
    leaves, slots, Sigma, vis = _graph(scene, visible, sw, proper_ewa_scaling, use_cov3D_precomp, torch.float64,
                                       {"view_in_covariance": view_in_covariance} if camera_leaves else None)
    rec = torch.as_tensor(np.asarray(records), dtype=torch.float64).abs()
    rec = torch.where(vis[:, None], rec, torch.zeros_like(rec))
    P = slots.shape[0]
    targets = list(leaves.values()) + ([] if use_cov3D_precomp else [Sigma])
    acc = {}
    for k in range(9):
        grads = torch.autograd.grad(slots[vis, k].sum(), targets, allow_unused=True, retain_graph=True)
        for n, a in _named(scene, leaves, Sigma, grads, sw, False, use_cov3D_precomp).items():
            term = rec[:, k].reshape((P,) + (1,) * (a.dim() - 1)) * a.detach().abs()
            acc[n] = term if n not in acc else acc[n] + term
    out = {n: torch.where(vis, a.reshape(P, -1).max(1).values, torch.zeros(P, dtype=torch.float64)).numpy() for n, a in acc.items()}
    if camera_leaves:
        names = {"dL_dview": "viewmatrix", "dL_dproj": "projmatrix", "dL_dcam": "campos"}
        eye = torch.eye(P, dtype=torch.float64)[vis]
        cam = {n: torch.zeros_like(leaves[l]) for n, l in names.items()}
        for k in range(9):
            grads = torch.autograd.grad(slots[:, k], [leaves[l] for l in names.values()] + [second["viewmatrix"]], grad_outputs=eye,
                                        is_grads_batched=True, allow_unused=True, retain_graph=True)
            for n, g in zip(list(names) + ["dL_dview"], grads):
                if g is not None:
                    cam[n] = cam[n] + (rec[vis, k].reshape((-1,) + (1,) * (g.dim() - 1)) * g.abs()).sum(0)
        out.update({n: a.detach().numpy() for n, a in cam.items()})
    return out


def ratio(got, ref, S):
    """Per Gaussian tensor (S of shape (P,)): the largest over the rows of max_row |got - ref| / S; per camera tensor (S in the
    tensor's shape): the largest entry of |got - ref| / S.  An error of 0 counts as 0, whatever S."""
    got, ref, S = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(S, np.float64)
    assert got.size == ref.size
    if S.shape == ref.shape and ref.shape in ((4, 4), (3,)):
        err = np.abs(got.reshape(ref.shape) - ref)
    else:
        err = np.abs(got.reshape(len(S), -1) - ref.reshape(len(S), -1)).max(1)
    assert np.all(S[err > 0] > 0), "an error where the scale is zero"
    q = np.divide(err, S, out=np.zeros_like(err), where=err > 0)
    return float(q.max()) if q.size else 0.0


def ratios(got, ref, S, names):
    return {n: ratio(got[n], ref[n], S[n]) for n in names if n in ref and n in got}


# ---- the input families and record kinds, shared by the CPU measurement and the GPU tests ---------------------------------------------------
W, H, BASE_P = 40, 36, 293   # 293: one full 256-row workgroup and a tail of 37
FAMILIES = ("plain", "clamped", "subpixel", "huge", "needles10", "needles24", "offband", "rawquat", "fxfy", "near", "far")
KINDS = ("normal", "oneslot", "wide", "zeros")


def _view(sc):
    V = np.asarray(sc.viewmatrix, np.float64)
    return np.asarray(sc.means3D, np.float64) @ V[:3, :3] + V[3, :3], V


def _set_view(sc, pv, V):
    sc.means3D = np.ascontiguousarray((pv - V[3, :3]) @ np.linalg.inv(V[:3, :3]), dtype=np.float32)


def family(name, P=BASE_P, M=16, D=3, precomp=False):
    """The scene of input family `name` (FAMILIES) with P Gaussians on 40x36 pixels, M stored SH coefficients, active degree D."""
    mk = lambda lo, hi, seed, camera="orbit", **kw: scenes.make_scene(P=P, W=W, H=H, sigma_min=lo, sigma_max=hi, seed=seed, camera=camera, **kw)
    if name == "plain":
        sc = mk(1.0, 8.0, 21)
        pv, V = _view(sc)
        pv[3::7, 2] *= -1.0   # every seventh behind the camera
        _set_view(sc, pv, V)
    elif name == "clamped":   # tests/test_gpu_sh_stash.py: scene()
        sc = mk(1.0, 8.0, 11 + 16 + 3, camera="origin")
        sc.shs[::5, 0, 0] -= 3.0
        sc.shs[2::5, 0, 2] -= 3.0
        sc.means3D[::7, 2] *= -1.0
    elif name == "subpixel":
        sc = mk(0.02, 0.3, 32)
    elif name == "huge":
        sc = mk(30.0, 200.0, 23)
    elif name in ("needles10", "needles24"):
        sc = mk(1.0, 8.0, 24)
        sc.scales[np.arange(P), np.arange(P) % 3] *= 10.0 if name == "needles10" else 24.0
    elif name == "offband":
        sc = mk(10.0, 40.0, 25)
        pv, V = _view(sc)
        i = np.arange(P)
        sign = np.where((i // 3) % 2 == 0, 1.0, -1.0)
        pv[:, 0] = np.where(i % 3 == 0, sign * 1.4 * sc.tanfovx * pv[:, 2], pv[:, 0])
        pv[:, 1] = np.where(i % 3 == 1, sign * 1.45 * sc.tanfovy * pv[:, 2], pv[:, 1])
        _set_view(sc, pv, V)
    elif name == "rawquat":
        sc = mk(1.0, 8.0, 26)
        norm = np.exp(math.log(0.3) + (math.log(3.0) - math.log(0.3)) * scenes.uniform(26, 400, P))
        sc.rotations = np.ascontiguousarray(sc.rotations.astype(np.float64) * norm[:, None], dtype=np.float32)
        sc.scale_modifier = 1.7
    elif name == "fxfy":
        from test_camera_model_cpu import VARIANTS   # fx != fy, an off-centre principal point and a rolled view
        sc = scenes.vary_inputs(mk(1.0, 8.0, 27), **VARIANTS["camera_only"])
    elif name == "near":
        sc = mk(1.0, 8.0, 28, z_range=(0.25, 0.9))
    elif name == "far":
        sc = mk(1.0, 8.0, 29, z_range=(40.0, 90.0))
    else:
        raise KeyError(name)
    sc.shs = np.ascontiguousarray(sc.shs[:, :M])
    sc.sh_degree = D
    if precomp:
        sc.colors_precomp = np.random.default_rng(11).uniform(0.05, 1.0, (P, 3)).astype(np.float32)
        sc.shs = None
    return sc


def records(kind, P, seed=5):
    """(P, 9) float32 records of KINDS"""
    n = scenes.normal(seed, 500, 9 * P).reshape(P, 9)
    if kind == "normal":
        r = n
    elif kind == "oneslot":   # one live slot per Gaussian: a swapped or mis-scaled slot cannot hide behind a larger one
        r = np.where(np.arange(9)[None] == (np.arange(P) % 9)[:, None], n, 0.0)
    elif kind == "wide":
        r = np.sign(n) * 10.0 ** (-6.0 + 9.0 * scenes.uniform(seed, 501, 9 * P).reshape(P, 9))
    elif kind == "zeros":
        r = np.zeros((P, 9))
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(r, dtype=np.float32)


def with_nan_rows(rec, visible):
    """the records with NaN in every row of an invisible Gaussian (the per-Gaussian half must not read them)"""
    r = np.array(rec, np.float32)
    r[~np.asarray(visible, bool)] = np.nan
    return r


def yardstick_visible(scene, proper_ewa_scaling=False):
    """The float64 renderer's own visibility (in front of the near plane, opacity, a tile rectangle that is not empty): the rows the CPU
    measurement runs on.  (The GPU tests use the forward's radii: the product's culling options cull more.)"""
    with torch.no_grad():
        details = torch_ref.render_core(scene, "global", proper_ewa_scaling)[2]
    return details["cand"].any(0).numpy()


def conditions(scene, visible):
    """Asserts, in float64, that no visible Gaussian sits on a decision the kernel takes in float32: |x/z| / (1.3 tan_fov) within 1e-4 of
    1, or a colour channel within 1e-4 of 0 (before the clamp).  Returns (outside the band in x (P,), in y (P,), clamped channels
    (P,3)), each of visible Gaussians only."""
    pv, _ = _view(scene)
    rx, ry = np.abs(pv[:, 0] / pv[:, 2]) / (1.3 * scene.tanfovx), np.abs(pv[:, 1] / pv[:, 2]) / (1.3 * scene.tanfovy)
    v = np.asarray(visible, bool)
    assert np.all(np.abs(rx[v] - 1) > 1e-4) and np.all(np.abs(ry[v] - 1) > 1e-4)
    clamped = np.zeros((scene.P, 3), bool)
    if scene.shs is not None:
        d = torch.tensor(scene.means3D.astype(np.float64) - scene.campos.astype(np.float64))
        col = torch_ref.eval_sh(scene.sh_degree, torch.tensor(scene.shs.astype(np.float64)), d / d.norm(dim=1, keepdim=True)).numpy()
        assert np.all(np.abs(col[v]) > 1e-4)
        clamped = col < 0
    return (rx > 1) & v, (ry > 1) & v, clamped & v[:, None]


def reference(scene, rec, visible, key=None, **kw):
    """({name: float64 gradient}, {name: S}) of vjp(kernel=True) and scale(kernel=True); kept under `key` (torch_ref.cached)."""
    def make():
        g = vjp(scene, rec, visible, kernel=True, **kw)
        s = scale(scene, rec, visible, kernel=True, **kw)
        assert sorted(g) == sorted(s)
        return tuple(g[n] for n in sorted(g)) + tuple(s[n] for n in sorted(g)) + (np.array(sorted(g)),)
    out = torch_ref.cached("per_gaussian", key, make)
    names = [str(n) for n in out[-1]]
    return dict(zip(names, out[:len(names)])), dict(zip(names, out[len(names):-1]))


def measure_float32(name, kinds=KINDS, family_kw=None, **kw):
    """{tensor: worst ratio over `kinds`} of this module evaluated in float32 against itself in float64, on family `name`."""
    sc = family(name, **(family_kw or {}))
    vis = yardstick_visible(sc, kw.get("proper_ewa_scaling", False))
    cond = conditions(sc, vis)
    worst = {}
    for kind in kinds:
        rec = records(kind, sc.P)
        ref, S = reference(sc, rec, vis, **kw)
        got = vjp(sc, rec, vis, kernel=True, dtype=torch.float32, **kw)
        for n, r in ratios(got, ref, S, MEASURED + (CAMERA if kw.get("camera_leaves") else ())).items():
            worst[n] = max(worst.get(n, 0.0), r)
    return worst, int(vis.sum()), cond


def tolerance(worst):
    """4 x the float32 evaluation's worst ratio, rounded up to two significant digits, floor 16 * 2^-24"""
    t = max(4.0 * worst, FLOOR)
    e = 10.0 ** (math.floor(math.log10(t)) - 1)
    return float(f"{math.ceil(t / e - 1e-9) * e:.1e}")


# what the GPU tests run besides the families with their four record kinds, on "plain" and "clamped" with N(0,1) records: (family(...)
# arguments, vjp(...) arguments); proper_ewa_scaling is measured into a table row of its own, the camera tensors into "camera"
VARIANT_MEASUREMENTS = (
    (dict(M=16, D=1), {}), (dict(M=9, D=2), {}), (dict(M=4, D=1), {}), (dict(M=1, D=0), {}), (dict(precomp=True), {}),
    ({}, dict(use_cov3D_precomp=True)), ({}, dict(proper_ewa_scaling=True)), ({}, dict(camera_leaves=True)),
    ({}, dict(camera_leaves=True, proper_ewa_scaling=True)))

# T[family][tensor], measured as the module docstring says (tests/test_per_gaussian_cpu.py repeats the measurement); "<family>_ewa": under
# proper_ewa_scaling; "camera": the three camera tensors, entrywise, over both families, with and without proper_ewa_scaling.
# "needles24": one scale x 24.  At x 30 the float32 evaluation reaches 7.0e-4 (dL_dmeans3D, dL_drotations), which would need 2.8e-3, above
# CAP: the error grows with the square of the anisotropy, and x 24 is the largest factor that fits.
T = {
    "plain": {"dL_dmeans3D": 4.1e-06, "dL_dscales": 4.7e-06, "dL_drotations": 5.2e-06, "dL_dsh": 1.4e-06, "dL_dcov3D": 4.1e-06, "dL_dopacity": 9.6e-07},
    "clamped": {"dL_dmeans3D": 7.1e-06, "dL_dscales": 4.1e-06, "dL_drotations": 6.6e-06, "dL_dsh": 1.4e-06, "dL_dcov3D": 3.3e-06, "dL_dopacity": 9.6e-07},
    "subpixel": {"dL_dmeans3D": 1.8e-05, "dL_dscales": 4.9e-06, "dL_drotations": 4.8e-06, "dL_dsh": 1.6e-06, "dL_dcov3D": 2.9e-06, "dL_dopacity": 9.6e-07},
    "huge": {"dL_dmeans3D": 7.9e-06, "dL_dscales": 5.4e-06, "dL_drotations": 7.9e-06, "dL_dsh": 1.5e-06, "dL_dcov3D": 4.9e-06, "dL_dopacity": 9.6e-07},
    "needles10": {"dL_dmeans3D": 1.9e-04, "dL_dscales": 3.1e-04, "dL_drotations": 3.8e-04, "dL_dsh": 1.5e-06, "dL_dcov3D": 3.1e-04, "dL_dopacity": 9.6e-07},
    "needles24": {"dL_dmeans3D": 1.1e-03, "dL_dscales": 1.8e-03, "dL_drotations": 1.9e-03, "dL_dsh": 1.5e-06, "dL_dcov3D": 1.8e-03, "dL_dopacity": 9.6e-07},
    "offband": {"dL_dmeans3D": 4.5e-06, "dL_dscales": 4.5e-06, "dL_drotations": 9.7e-06, "dL_dsh": 1.3e-06, "dL_dcov3D": 4.4e-06, "dL_dopacity": 9.6e-07},
    "rawquat": {"dL_dmeans3D": 6.2e-05, "dL_dscales": 4.2e-05, "dL_drotations": 2.2e-05, "dL_dsh": 1.6e-06, "dL_dcov3D": 1.8e-05, "dL_dopacity": 9.6e-07},
    "fxfy": {"dL_dmeans3D": 4.8e-06, "dL_dscales": 6.7e-06, "dL_drotations": 1.9e-05, "dL_dsh": 1.3e-06, "dL_dcov3D": 3.9e-06, "dL_dopacity": 9.6e-07},
    "near": {"dL_dmeans3D": 6.3e-06, "dL_dscales": 4.4e-06, "dL_drotations": 9.0e-06, "dL_dsh": 1.5e-06, "dL_dcov3D": 3.8e-06, "dL_dopacity": 9.6e-07},
    "far": {"dL_dmeans3D": 5.8e-06, "dL_dscales": 3.2e-06, "dL_drotations": 3.9e-05, "dL_dsh": 1.6e-06, "dL_dcov3D": 3.2e-06, "dL_dopacity": 9.6e-07},
    "plain_ewa": {"dL_dmeans3D": 4.1e-06, "dL_dscales": 4.2e-06, "dL_drotations": 5.2e-06, "dL_dsh": 1.4e-06, "dL_dcov3D": 4.4e-06, "dL_dopacity": 9.6e-07},
    "clamped_ewa": {"dL_dmeans3D": 7.1e-06, "dL_dscales": 4.1e-06, "dL_drotations": 6.6e-06, "dL_dsh": 1.4e-06, "dL_dcov3D": 3.3e-06, "dL_dopacity": 9.6e-07},
    "camera": {"dL_dview": 9.6e-07, "dL_dproj": 9.6e-07, "dL_dcam": 9.6e-07},
}
