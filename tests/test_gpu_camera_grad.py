"""GPU tests (-m gpu) of the camera gradients: dL/dviewmatrix, dL/dprojmatrix and dL/dcampos (include/stp_raster.h:
stp_set_backward_camera_grads; routed by rasterize_gaussians() through _RasterizeGaussiansCamera when a camera tensor requires grad).

  * tiny scenes against a float64 autograd reference with the camera tensors as leaves (torch_ref_camera.py), every sort mode with a
    backward, both backward modes, SH degrees 0-3, precomputed colours / covariances, Gaussians in the clamped band;
  * the translation gauge at full size (C2-full, C3, one proper_ewa_scaling scene): moving world and camera together changes nothing;
  * nothing else moves: image, radii and the Gaussian gradients are those of a run without the request, bit for bit from the same
    per-Gaussian records; camera gradients are bit-reproducible;
  * frozen Gaussians, P = 0, a fully culled frame, a chunked per-Gaussian half;
  * pose refinement end to end: Adam on a 6-DoF pose recovers a perturbed camera.
"""
import functools
import math

import numpy as np
import pytest
import torch

from helpers import CAMERA, FULL_STP, _direct, _rel, api_render, api_settings, ext_settings, max_abs, settings_dict
from diff_gaussian_rasterization import scenes
import torch_ref_camera

pytestmark = pytest.mark.gpu

render = functools.partial(api_render, camera=CAMERA)   # camera: the camera tensors that require grad


def tiny(seed=7, use_sh=True, degree=3, clamped=True, P=150, W=40, H=36):
    sc = scenes.make_scene(P=P, W=W, H=H, sigma_min=1.0, sigma_max=8.0, seed=seed, use_sh=use_sh, camera="orbit")
    sc.sh_degree = degree
    return torch_ref_camera.with_clamped_gaussians(sc) if clamped else sc


def cov6(sc):
    R = torch_ref_camera.quat_to_rot(torch.tensor(sc.rotations, dtype=torch.float64))
    S = torch.diag_embed((sc.scale_modifier * torch.tensor(sc.scales, dtype=torch.float64)) ** 2)
    Sig = (R @ S @ R.transpose(1, 2)).numpy()
    return np.stack([Sig[:, 0, 0], Sig[:, 0, 1], Sig[:, 0, 2], Sig[:, 1, 1], Sig[:, 1, 2], Sig[:, 2, 2]], 1).astype(np.float32)


MODES = {   # settings, the float64 reference's order
    "global_z": (settings_dict(0, order=0), dict(order="global", depth_key="z")),
    "global_distance": (settings_dict(0, order=1), dict(order="global", depth_key="distance")),
    "kbuffer16": (settings_dict(2, per_pixel=16), dict(order="exact")),
    "hier": (settings_dict(3), dict(order="exact")),
    "hier_full": (settings_dict(**FULL_STP), dict(order="exact")),
}


def _check_against_reference(got, ref, names=CAMERA + ("means3D",), tol=5e-5):
    for n in names:
        assert got[n] is not None, n
        if ref[n] is None or not np.any(ref[n]):   # (campos with colours or SH degree 0: no view-direction dependence)
            assert torch.equal(got[n], torch.zeros_like(got[n])), n
            continue
        assert got[n].shape == ref[n].shape and got[n].dtype == torch.float32, n
        r = _rel(got[n].cpu().numpy(), ref[n])
        assert r < tol, f"{n}: rel {r:.2e}\n got {got[n].cpu().numpy()}\n ref {ref[n]}"


@pytest.mark.parametrize("backward_mode", ["replay", "resort"])
@pytest.mark.parametrize("mode", list(MODES))
def test_camera_grads_match_float64_autograd(mode, backward_mode):
    sd, ref_kw = MODES[mode]
    sc = tiny()
    img, ref = torch_ref_camera.loss_and_grads(sc, **ref_kw)
    got = render(sc, sd, backward_mode=backward_mode)
    assert got["grad_fn"] == "_RasterizeGaussiansCameraBackward"
    assert max_abs(got["color"].cpu().numpy(), img) < 2e-6
    _check_against_reference(got, ref)
    # entries the forward never reads
    assert torch.all(got["viewmatrix"][:, 3] == 0) and torch.all(got["projmatrix"][:, 2] == 0)


@pytest.mark.parametrize("backward_mode", ["replay", "resort"])
@pytest.mark.parametrize("variant", ["sh0", "sh1", "sh2", "colors_precomp", "cov3D_precomp"])
def test_camera_grads_input_variants(variant, backward_mode):
    sd, ref_kw = MODES["global_z" if variant == "cov3D_precomp" else "hier"]   # (the sorted modes need scales and rotations)
    sc = tiny(seed=11, use_sh=variant != "colors_precomp", degree=int(variant[2]) if variant.startswith("sh") else 3)
    cov = cov6(sc) if variant == "cov3D_precomp" else None
    img, ref = torch_ref_camera.loss_and_grads(sc, use_cov3D_precomp=cov is not None, **ref_kw)
    got = render(sc, sd, backward_mode=backward_mode, cov3D=cov)
    assert max_abs(got["color"].cpu().numpy(), img) < 2e-6
    _check_against_reference(got, ref)
    if variant == "colors_precomp":
        assert torch.all(got["campos"] == 0)


@pytest.mark.parametrize("mode", ["global_z", "hier_full"])
def test_camera_grads_proper_ewa_scaling(mode):
    """proper_ewa_scaling: projmatrix and campos match autograd; viewmatrix carries the reference's covariance-gradient quirk exactly as
    dL/dmeans3D does (test_oracle_cpu.py::test_oracle_ewa_scaling_gradient_quirk) and is covered by the gauge test."""
    sd, ref_kw = MODES[mode]
    sd = dict(sd, proper_ewa_scaling=True)
    sc = tiny(seed=5)
    img, ref = torch_ref_camera.loss_and_grads(sc, proper_ewa_scaling=True, **ref_kw)
    got = render(sc, sd)
    assert max_abs(got["color"].cpu().numpy(), img) < 2e-6
    _check_against_reference(got, ref, names=("projmatrix", "campos"))


def _gauge_residual(sc, got):
    f64 = lambda x: x.double().cpu().numpy()
    V, P = np.asarray(sc.viewmatrix, np.float64), np.asarray(sc.projmatrix, np.float64)
    gm, gv, gp, gc = f64(got["means3D"]), f64(got["viewmatrix"]), f64(got["projmatrix"]), f64(got["campos"])
    terms = [gm.sum(0), gc, -V[:3, :] @ gv[3, :], -P[:3, :] @ gp[3, :]]
    scale = np.abs(gm).sum(0) + np.abs(gc) + np.abs(V[:3, :]) @ np.abs(gv[3, :]) + np.abs(P[:3, :]) @ np.abs(gp[3, :])
    return sum(terms), scale


@pytest.mark.parametrize("name", ["C2-full", "C3", "ewa"])
def test_translation_gauge_full_size(name):
    """Shifting world and camera together by delta leaves the image unchanged, so
    sum_i dL/dmu_i + dL/dcampos - V[:3,:] dL/dV[3,:]^T - P[:3,:] dL/dP[3,:]^T = 0 (float64 on the host, from the product's outputs)."""
    if name == "C2-full":
        sc, sd = scenes.config("C2"), settings_dict(**FULL_STP)
    elif name == "C3":
        sc, sd = scenes.config("C3"), settings_dict(2, per_pixel=16)
    else:
        sc, sd = scenes.make_scene(P=20000, W=256, H=256, sigma_min=1.0, sigma_max=10.0, seed=13, camera="orbit"), \
            dict(settings_dict(**FULL_STP), proper_ewa_scaling=True)
    got = render(sc, sd)
    for n in CAMERA + ("means3D",):
        assert torch.isfinite(got[n]).all(), n
    res, scale = _gauge_residual(sc, got)
    print(f"\n{name}: gauge residual {res} / magnitude {scale} = {np.abs(res) / scale}")
    # measured: about 1e-10 of the magnitude at C2-full / C3, 6e-9 with proper_ewa_scaling (20k Gaussians); the issue's guess was 1e-3
    assert np.all(np.abs(res) <= 1e-7 * scale), (res, scale)
    # ... and against the camera side alone: an error in the translation rows or in dL/dcampos is not hidden by the Gaussian sum
    V, P = np.asarray(sc.viewmatrix, np.float64), np.asarray(sc.projmatrix, np.float64)
    f64 = lambda x: x.double().cpu().numpy()
    cam_side = np.abs(f64(got["campos"])) + np.abs(V[:3, :] @ f64(got["viewmatrix"])[3, :]) + np.abs(P[:3, :] @ f64(got["projmatrix"])[3, :])
    print(f"{name}: residual / camera-side magnitude = {np.abs(res) / cam_side}")
    assert np.all(np.abs(res) <= 1e-5 * cam_side), (res, cam_side)


@pytest.mark.parametrize("backward_mode", ["replay", "resort"])
def test_nothing_else_moves(backward_mode):
    """With the request, the image, the radii and the Gaussian gradients are those of a run without it.  End to end the Gaussian gradients
    are compared bit for bit whenever two runs without the request are (the render half's float atomics are the only run-to-run
    variation, and the request does not touch that half); from the same per-Gaussian records they are bit-identical always, and the
    camera gradients are bit-reproducible."""
    sc = scenes.make_scene(P=20000, W=256, H=256, sigma_min=1.0, sigma_max=10.0, seed=3, camera="orbit")
    sd = settings_dict(**FULL_STP)
    gauss = ("means3D", "means2D", "shs", "opacities", "scales", "rotations")
    a, b, a2 = render(sc, sd, backward_mode=backward_mode), render(sc, sd, camera=(), backward_mode=backward_mode), \
        render(sc, sd, backward_mode=backward_mode)
    assert b["grad_fn"] == "_RasterizeGaussiansBackward" and a["grad_fn"] == "_RasterizeGaussiansCameraBackward"
    assert torch.equal(a["color"], b["color"]) and torch.equal(a["radii"], b["radii"])
    b2 = render(sc, sd, camera=(), backward_mode=backward_mode)
    for n in gauss:
        if torch.equal(b[n], b2[n]):
            assert torch.equal(a[n], b[n]), n
        else:   # the render half varies run to run here: the request adds nothing to that spread
            assert (a[n] - b[n]).abs().max().item() <= 4 * (b[n] - b2[n]).abs().max().item(), n
    if all(torch.equal(a[n], a2[n]) for n in gauss):
        for n in CAMERA:
            assert torch.equal(a[n], a2[n]), n


PHASE_CASES = {   # scene variant, settings, phases bits
    "sh3": (dict(), settings_dict(**FULL_STP), 0),
    "sh3_compact_clear": (dict(), settings_dict(**FULL_STP), 4 | 8),
    "sh0": (dict(degree=0), settings_dict(3), 0),
    "sh1": (dict(degree=1), settings_dict(2, per_pixel=16), 0),
    "sh2": (dict(degree=2), settings_dict(3), 0),
    "colors_precomp": (dict(use_sh=False), settings_dict(**FULL_STP), 0),
    "cov3D_precomp": (dict(cov=True), settings_dict(0), 0),
    "proper_ewa_scaling": (dict(), dict(settings_dict(**FULL_STP), proper_ewa_scaling=True), 0),
}


@pytest.mark.parametrize("backward_mode", ["replay", "resort"])
@pytest.mark.parametrize("case", list(PHASE_CASES))
def test_per_gaussian_half_bit_identical_with_request(case, backward_mode):
    """The per-Gaussian half on the same records with and without the camera request: its eight outputs bit for bit, and the camera
    gradients bit-reproducible."""
    from diff_gaussian_rasterization import _C
    kw, sd, bits = PHASE_CASES[case]
    sc = scenes.make_scene(P=20000, W=256, H=256, sigma_min=1.0, sigma_max=10.0, seed=3, camera="orbit", use_sh=kw.get("use_sh", True))
    sc.sh_degree = kw.get("degree", 3)
    cov = cov6(sc) if kw.get("cov") else None
    log = backward_mode == "replay" and sd["sort_settings"]["sort_mode"] in (2, 3)
    args = _direct(sc, {**sd, "_record_blend_log": log, "_backward_mode": backward_mode}, cov3D=cov)
    records = _C.rasterize_gaussians_backward(*args, phases=1 | (bits & 4))
    plain = _C.rasterize_gaussians_backward(*args, phases=2 | bits, partial=records.clone())
    cam1 = _C.rasterize_gaussians_backward(*args, phases=2 | bits, partial=records.clone(), camera_grads=True)
    cam2 = _C.rasterize_gaussians_backward(*args, phases=2 | bits, partial=records.clone(), camera_grads=True)
    assert len(plain) == 8 and len(cam1) == 11
    names = ("means2D", "colors", "opacity", "means3D", "cov3D", "sh", "scales", "rotations")
    for k in range(8):
        assert torch.equal(plain[k], cam1[k]), (names[k], (plain[k] - cam1[k]).abs().max().item())
        assert torch.equal(cam1[k], cam2[k]), names[k]
    for y, z in zip(cam1[8:], cam2[8:]):
        assert torch.equal(y, z)
    assert cam1[8].shape == (4, 4) and cam1[9].shape == (4, 4) and cam1[10].shape == (3,)
    assert any(bool(torch.any(x != 0)) for x in cam1[8:])


def test_frozen_gaussians():
    """Only the camera requires grad: the same camera gradients as the full run, no Gaussian gradient, blend log recorded."""
    sc = tiny(P=400, W=64, H=64)
    sd = settings_dict(**FULL_STP)
    full = render(sc, sd, backward_mode="replay")
    cam = render(sc, sd, gaussians=False, backward_mode="replay")
    assert cam["grad_fn"] == "_RasterizeGaussiansCameraBackward"
    for n in ("means3D", "means2D", "shs", "opacities", "scales", "rotations"):
        assert cam[n] is None, n
    for n in CAMERA:
        assert _rel(cam[n].cpu().numpy(), full[n].cpu().numpy()) < 1e-5, n
    only_view = render(sc, sd, camera=("viewmatrix",), gaussians=False)
    assert only_view["projmatrix"] is None and only_view["campos"] is None
    assert _rel(only_view["viewmatrix"].cpu().numpy(), full["viewmatrix"].cpu().numpy()) < 1e-5


def test_empty_and_culled_frames():
    empty = scenes.make_scene(P=1, W=48, H=40, sigma_min=1.0, sigma_max=2.0, seed=1, camera="orbit")
    for f in ("means3D", "scales", "rotations", "opacities", "shs"):
        setattr(empty, f, getattr(empty, f)[:0])
    got = render(empty, settings_dict(**FULL_STP), gaussians=False)
    for n in CAMERA:
        assert got[n] is not None and torch.equal(got[n], torch.zeros_like(got[n])), n
    behind = scenes.make_scene(P=200, W=48, H=40, sigma_min=1.0, sigma_max=8.0, seed=7)   # camera at the origin looking down +z
    behind.means3D = (behind.means3D * np.array([1, 1, -1], np.float32)).astype(np.float32)
    for sd in (settings_dict(**FULL_STP), settings_dict(0)):
        got = render(behind, sd)
        assert int(got["radii"].max()) == 0
        for n in CAMERA:
            assert torch.equal(got[n], torch.zeros_like(got[n])), n


def test_chunked_half_refuses_camera_grads():
    from diff_gaussian_rasterization import _C
    sc = tiny(clamped=False, P=600)
    sd = {**settings_dict(**FULL_STP), "_backward_mode": "resort"}
    args = _direct(sc, sd)
    records = _C.rasterize_gaussians_backward(*args, phases=1 | 4)
    with pytest.raises(RuntimeError, match="chunked"):
        _C.rasterize_gaussians_backward(*args, phases=2 | 4, partial=records, chunk=(0, 2), camera_grads=True)
    # the refused request was consumed: the next plain call runs as always
    out = _C.rasterize_gaussians_backward(*args, phases=2 | 4, partial=records, chunk=(0, 1))
    assert len(out) == 8


# ---- pose refinement -------------------------------------------------------------------------------------------------------------
def _rodrigues(w):
    th = torch.sqrt((w * w).sum() + 1e-20)
    k = w / th
    K = torch.stack([torch.stack([0 * th, -k[2], k[1]]), torch.stack([k[2], 0 * th, -k[0]]), torch.stack([-k[1], k[0], 0 * th])])
    return torch.eye(3, dtype=w.dtype, device=w.device) + torch.sin(th) * K + (1 - torch.cos(th)) * (K @ K)


def _camera_from_pose(pose, V0, proj):
    """pose = (omega, tau): p_view = R(omega) p_view0 + tau.  Row-vector layout: V = V0 @ [[R^T, 0], [tau, 1]], P = V @ proj,
    campos = the camera centre (p_view = 0)."""
    R = _rodrigues(pose[:3])
    top = torch.cat([R.T, torch.zeros(3, 1, dtype=pose.dtype, device=pose.device)], 1)
    bottom = torch.cat([pose[3:], torch.ones(1, dtype=pose.dtype, device=pose.device)])[None]
    V = V0 @ torch.cat([top, bottom], 0)
    campos = -V[3, :3] @ torch.linalg.inv(V[:3, :3])
    return V, V @ proj, campos


def test_pose_refinement_end_to_end():
    """Adam on a 6-DoF pose vector (axis-angle + translation, through torch ops that build V, P = V @ Proj and campos) recovers a camera
    perturbed by 2 degrees and 2 % of the scene depth from a target rendered at the true pose."""
    import diff_gaussian_rasterization as dgr
    dev = torch.device("cuda:0")
    sc = scenes.make_scene(P=20000, W=256, H=256, sigma_min=1.0, sigma_max=10.0, seed=17, camera="orbit", opacity_range=(0.2, 0.8))
    f = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    V0 = f(sc.viewmatrix)
    proj = torch.linalg.inv(V0.double()).float() @ f(sc.projmatrix)   # the projection-only matrix: P = V @ proj
    means, opac, scales, rots, shs = f(sc.means3D), f(sc.opacities), f(sc.scales), f(sc.rotations), f(sc.shs)
    es = ext_settings(settings_dict(**FULL_STP))

    def draw(pose):
        V, P, cam = _camera_from_pose(pose, V0, proj)
        rs = api_settings(sc, es, dev, viewmatrix=V, projmatrix=P, inv_viewprojmatrix=torch.linalg.inv(P.detach().double()).float(), campos=cam)
        return dgr.GaussianRasterizer(rs)(means, torch.zeros_like(means), opac, shs=shs, scales=scales, rotations=rots)[0]

    with torch.no_grad():
        target = draw(torch.zeros(6, device=dev))
    rng = np.random.default_rng(0)
    axis, tdir = rng.normal(size=3), rng.normal(size=3)
    depth = float(np.median((np.c_[sc.means3D, np.ones(sc.P)] @ sc.viewmatrix)[:, 2]))
    start = np.r_[axis / np.linalg.norm(axis) * math.radians(2.0), tdir / np.linalg.norm(tdir) * 0.02 * depth]
    omega = torch.tensor(start[:3], dtype=torch.float32, device=dev, requires_grad=True)
    tau = torch.tensor(start[3:], dtype=torch.float32, device=dev, requires_grad=True)
    steps = 150
    opt = torch.optim.Adam([{"params": [omega], "lr": 2e-3}, {"params": [tau], "lr": 5e-3}])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 0.5 * (1 + math.cos(math.pi * it / steps)))
    for _ in range(steps):
        opt.zero_grad()
        loss = (draw(torch.cat([omega, tau])) - target).abs().mean()
        loss.backward()
        assert torch.isfinite(omega.grad).all() and torch.isfinite(tau.grad).all()
        opt.step()
        sched.step()
    p = torch.cat([omega, tau]).detach().cpu().numpy()
    rot0, rot1 = np.linalg.norm(start[:3]), np.linalg.norm(p[:3])
    tr0, tr1 = np.linalg.norm(start[3:]), np.linalg.norm(p[3:])
    print(f"\npose refinement: rotation {math.degrees(rot0):.3f} -> {math.degrees(rot1):.4f} deg, translation {tr0:.4f} -> {tr1:.5f} "
          f"(depth {depth:.2f}), final L1 {loss.item():.2e}")
    assert rot1 <= 0.2 * rot0 and tr1 <= 0.2 * tr0


def test_camera_inputs_modified_in_place_raise():
    """The camera Function saves its camera inputs like the Gaussian ones: changing one in place before the backward raises."""
    import diff_gaussian_rasterization as dgr
    sc = tiny(clamped=False)
    dev = torch.device("cuda:0")
    f = lambda a, rg=False: torch.tensor(np.asarray(a, np.float32), device=dev).requires_grad_(rg)
    V = f(sc.viewmatrix) * 1.0
    V.requires_grad_(True)
    Vin = V.clone()   # a non-leaf the caller could modify in place
    rs = api_settings(sc, ext_settings(settings_dict(3)), dev, viewmatrix=Vin)
    m = f(sc.means3D)
    color, _ = dgr.GaussianRasterizer(rs)(m, torch.zeros_like(m), f(sc.opacities), shs=f(sc.shs), scales=f(sc.scales), rotations=f(sc.rotations))
    with torch.no_grad():
        Vin[3, 0] += 1.0
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (color * f(sc.dL_dout)).sum().backward()
