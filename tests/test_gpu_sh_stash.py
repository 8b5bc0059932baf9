"""GPU tests (-m gpu) of the SH stash (include/stp_raster.h: stp_set_forward_sh_stash) and of the optional outputs of the backward.

A forward that can be differentiated keeps, per visible Gaussian, the nine derivatives d(colour channel) / d(unit view direction) its SH
colour kernel can form from what it holds; the per-Gaussian backward reads them in the place of the SH rows.  Here:

  * the same build runs the same frame with the request and without it (settings._no_sh_stash: the legacy path): every output of the
    forward and every gradient, the camera's included, bit for bit -- over P (two workgroups, a partial last one, the unrolled and the
    generic staging), M, an active degree below the stored one, concatenated / split / misaligned split SH, with and without camera
    gradients and the inverse-depth request, on a frame with Gaussians behind the camera and off screen and with clamped colours;
  * dL_dmeans3D, the one gradient the stash enters, of both paths against the float64 yardstick (torch_ref.py), bound 1e-4 of the
    largest entry (tests/test_reference_pin.py's);
  * the stash itself against a float64 evaluation of the nine derivatives written here from the formulas;
  * the outputs nobody receives: autograd's six leaf gradients against a direct _C backward that writes all eight; dL_dcolors /
    dL_dcov3D still arrive where colors_precomp / cov3D_precomp are given;
  * buffers without a stash, and clones of either kind.
"""
import numpy as np
import pytest
import torch

import helpers
import torch_ref
from helpers import FULL_STP, _rel, api_render, settings_dict
from diff_gaussian_rasterization import scenes

pytestmark = pytest.mark.gpu

MD = [(1, 0), (4, 1), (9, 2), (16, 3), (16, 1), (9, 1)]   # (stored coefficients, active degree): the last two are active below stored
EIGHT = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")


def scene(P, M, D, camera="origin", hide=True, plain=False):
    """P Gaussians on 40x36 pixels with M stored coefficients and active degree D.  hide: every seventh Gaussian is put behind the camera
    (with the frame's own margin of 5 % off-screen positions: invisible rows in every workgroup).  plain: the frame of the float64
    comparisons of tests/test_gpu_absgrad.py as it is, but for M and D."""
    sc = scenes.make_scene(P=P, W=40, H=36, sigma_min=1.0, sigma_max=8.0, seed=7 if plain else 11 + M + D, camera=camera)
    sc.shs = np.ascontiguousarray(sc.shs[:, :M])
    sc.sh_degree = D
    if plain:
        return sc
    sc.shs[::5, 0, 0] -= 3.0    # colours driven negative on some channels: 0.5 + C0 * dc < 0, the clamp bytes are set
    sc.shs[2::5, 0, 2] -= 3.0
    if hide:
        assert camera == "origin"
        sc.means3D[::7, 2] *= -1.0
    return sc


def _sd(sd, stash, mode=None):
    d = dict(sd, _record_blend_log=True)
    if not stash:
        d["_no_sh_stash"] = True
    if mode:
        d["_backward_mode"] = mode
    return d


def _split(shs, misaligned):
    dc, rest = shs[:, :1].contiguous(), shs[:, 1:].contiguous()
    if misaligned:
        pad = lambda t: torch.cat((torch.zeros_like(t[:1]), t))[1:]
        dc, rest = pad(dc), pad(rest)
        assert dc.data_ptr() % 16 != 0
    return dc, rest


def lit(sc, frac=0.5):
    """The scene with dL_dout zeroed outside ONE pixel: every Gaussian then receives a single contribution from the render half, whose
    atomic sums are otherwise made in an order that differs from run to run -- two whole backwards of such a frame can be compared bit
    for bit."""
    mask = np.zeros((1, sc.H, sc.W), np.float32)
    mask[0, int(sc.H * frac), int(sc.W * frac)] = 1.0
    sc.dL_dout = sc.dL_dout * mask
    sc.meta["lit"] = mask
    return sc


def run(sc, sd, stash, layout="cat", camera=False, invd=False, mode=None, clone_geom=False, records=None):
    """One forward + backward through _C directly.  Returns (forward outputs, gradients, the gradient records), the first two dicts of
    tensors.  records=None: a whole backward; else the per-Gaussian half alone on these records (the render half sums with atomics in
    an order of its own every run: two paths of the per-Gaussian half are compared on the SAME records) -- "render" runs the render half
    first and hands its records on."""
    from diff_gaussian_rasterization import _C
    d = _sd(sd, stash, mode)
    empty = torch.Tensor([])
    dev = torch.device("cuda:0")
    t = lambda a: empty if a is None else torch.tensor(np.asarray(a, np.float32), device=dev)
    bg, m3, op, sca, rot, shs = t(sc.bg), t(sc.means3D), t(sc.opacities), t(sc.scales), t(sc.rotations), t(sc.shs)
    view, proj, inv, cam, w = t(sc.viewmatrix), t(sc.projmatrix), t(sc.inv_viewprojmatrix), t(sc.campos), t(sc.dL_dout)
    kw = {}
    sh_in = shs
    if layout != "cat":
        kw["dc"], sh_in = _split(shs, layout == "misaligned")
    fkw = dict(kw, invdepth=True) if invd else kw
    out = _C.rasterize_gaussians(bg, m3, empty, op, sca, rot, sc.scale_modifier, empty, view, proj, inv, sc.tanfovx, sc.tanfovy, sc.H, sc.W,
                                 sh_in, sc.sh_degree, cam, False, d, False, False, **fkw)
    R, color, radii, geom, binning, img = out[:6]
    assert _C.has_sh_stash(geom, sc.P, d) == bool(stash)
    L, s = _C._load(), _C.settings_from_dict(d)
    import ctypes
    want = L.stp_geometry_buffer_size_stash(sc.P, ctypes.byref(s)) if stash else L.stp_geometry_buffer_size(sc.P, ctypes.byref(s))
    assert geom.numel() == want, (geom.numel(), want)
    vis = radii > 0
    fwd = {"R": torch.tensor(R), "color": color, "radii": radii, "final_T": _C.image_array(img, sc.W, sc.H, "final_T").clone(),
           "n_contrib": _C.image_array(img, sc.W, sc.H, "n_contrib").clone()}
    for name in ("rgb", "clamped", "means2D", "conic_opacity", "depths", "cov3D"):   # (rows of invisible Gaussians are never written)
        a = _C.geometry_array(geom, sc.P, d, name)
        fwd[name] = a.view(sc.P, -1)[vis].clone()
    if R > 0:
        for name in ("point_list", "keys"):
            fwd[name] = _C.binning_array(binning, R, name).clone()
    if invd:
        fwd["invdepth"] = out[-1]
    if stash:
        fwd["_stash"] = _C.geometry_array(geom, sc.P, d, "sh_stash").view(9, sc.P).clone()
    bkw = dict(kw)
    if camera:
        bkw["camera_grads"] = True
    if invd:
        bkw["invdepth"] = out[-1]
        bkw["dL_dinvdepth"] = torch.linspace(-1.0, 1.0, sc.H * sc.W, device=dev).view(1, sc.H, sc.W) * t(sc.meta["lit"])
    if clone_geom:
        geom = geom.clone()
    args = (bg, m3, radii, op, empty, sca, rot, sc.scale_modifier, empty, view, proj, inv, sc.tanfovx, sc.tanfovy,
            color, w, sh_in, sc.sh_degree, cam, geom, R, binning, img, d, False)
    if records is not None:
        assert not invd   # (the binding wants both halves in one call with the inverse-depth request)
        if isinstance(records, str):
            records = _C.rasterize_gaussians_backward(*args, phases=1)
        bkw.update(phases=2, partial=records.clone())
    g = _C.rasterize_gaussians_backward(*args, **bkw)
    grads = dict(zip(EIGHT, g[:8]))
    rest = list(g[8:])
    if camera:
        grads.update(dL_dview=rest.pop(0), dL_dproj=rest.pop(0), dL_dcam=rest.pop(0))
    if layout != "cat":
        grads["dL_ddc"] = rest.pop(0)
    assert not rest
    return fwd, grads, records


def assert_same(a, b, skip=()):
    assert a.keys() - {"_stash"} == b.keys() - {"_stash"}
    for k in a:
        if k in skip or k == "_stash":
            continue
        assert a[k].shape == b[k].shape and torch.equal(torch.nan_to_num(a[k], nan=-7.0), torch.nan_to_num(b[k], nan=-7.0)), k


def _frame_has_what_it_should(sc, fwd):
    vis = fwd["radii"] > 0
    assert 0 < int((~vis).sum()) and int(vis.sum()) >= sc.P // 2           # invisible rows, and plenty of visible ones
    assert 0 < int(fwd["clamped"].sum()) < fwd["clamped"].numel()          # some colours were clamped at zero


# ---- 1. against the legacy path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("invd", [False, True], ids=["", "invd"])
@pytest.mark.parametrize("camera", [False, True], ids=["", "cam"])
@pytest.mark.parametrize("layout", ["cat", "split", "misaligned"])
@pytest.mark.parametrize("M,D", MD)
@pytest.mark.parametrize("P", [257, 300])
def test_stash_path_equals_legacy_path(P, M, D, layout, camera, invd):
    """Every forward output and every gradient but dL_dmeans3D, bit for bit, the camera's included (with a camera request the kernel
    still stages the coefficients in for its camera-terms pass: dL_dcampos is a function of the nine numbers, and it stays the legacy
    path's).  dL_dmeans3D is bit-equal up to degree 1 and an ulp or so apart above it -- the forward kernel fuses the
    shared expressions (csrc/stp_sh_dir.h) differently from the backward kernel; measured on MI355X: at most 3.5e-8 of the largest
    entry -- and the bound that holds is test_dmeans3D_against_float64_yardstick's.  The figure is printed."""
    sc, sd = scene(P, M, D), settings_dict(**FULL_STP)
    if invd:   # whole backwards: one lit pixel
        f0, g0, _ = run(lit(sc), sd, False, layout, camera, True)
        f1, g1, _ = run(sc, sd, True, layout, camera, True)
        assert int((g0["dL_dmeans2D"].abs().sum(1) > 0).sum()) >= 5
    else:      # the per-Gaussian halves of both paths on the records of one render half
        f0, g0, rec = run(sc, sd, False, layout, camera, records="render")
        f1, g1, _ = run(sc, sd, True, layout, camera, records=rec)
        assert int((g0["dL_dmeans2D"].abs().sum(1) > 0).sum()) >= P // 2
    _frame_has_what_it_should(sc, f1)
    assert_same(f0, f1)
    assert_same(g0, g1, skip=("dL_dmeans3D",))
    a, b = g0["dL_dmeans3D"], g1["dL_dmeans3D"]
    diff = float((a - b).abs().max()) / max(float(a.abs().max()), 1e-30)
    print(f"\nP={P} M={M} D={D} {layout} cam={camera} invd={invd}: dL_dmeans3D legacy vs stash, max diff / max = {diff:.2e}")
    if D <= 1:
        assert torch.equal(a, b)


@pytest.mark.parametrize("name,sd,mode", [("global", settings_dict(0), None), ("kbuffer16-replay", settings_dict(2, per_pixel=16), "replay"),
                                          ("hier-resort", settings_dict(3), "resort"), ("full-ewa", settings_dict(**FULL_STP, ewa=True), None)])
def test_stash_path_equals_legacy_path_in_other_modes(name, sd, mode):
    sc = scene(300, 16, 3)
    for camera in (False, True):
        f0, g0, rec = run(sc, sd, False, camera=camera, mode=mode, records="render")
        f1, g1, _ = run(sc, sd, True, camera=camera, mode=mode, records=rec)
        # (n_contrib of a forward that records no log is not part of what the backward reads in these modes: left out under "resort")
        assert_same(f0, f1, skip=("n_contrib",) if mode == "resort" else ())
        assert_same(g0, g1, skip=("dL_dmeans3D",))


# ---- 2. dL_dmeans3D against the float64 yardstick ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D", MD)
def test_dmeans3D_against_float64_yardstick(M, D):
    """Both paths against torch_ref.loss_and_grads (float64), relative to the largest entry; the stash path meets the project's bound of
    1e-4 and is not worse than twice the legacy path's error.  Measured on MI355X: both paths 4.7e-6 .. 6.7e-6, equal to the four
    digits printed."""
    sc = scene(150, M, D, camera="orbit", plain=True)
    ref = torch_ref.cached("sh_stash", (M, D), lambda: (torch_ref.loss_and_grads(sc, order="exact")[1]["means3D"],))[0]
    sd = settings_dict(3)
    err = {}
    for stash in (True, False):
        _, g, _ = run(sc, sd, stash)
        err[stash] = _rel(g["dL_dmeans3D"].cpu().numpy(), ref)
    print(f"\nM={M} D={D}: dL_dmeans3D rel err vs float64: stash {err[True]:.3e}, legacy {err[False]:.3e}")
    assert err[True] < 1e-4
    assert err[True] <= 2.0 * err[False]


# ---- 3. the stash itself ----------------------------------------------------------------------------------------------------------------
def _dir_derivatives_f64(sc):
    """(9, P) float64: plane 3 c + {0, 1, 2} = d(colour channel c) / d(x, y, z) at the unit view direction, and the sum of the absolute
    values of the summands of each entry (9, P).  From the real SH basis of degree <= 3, differentiated by hand."""
    C1, C2, C3 = torch_ref.SH_C1, torch_ref.SH_C2, torch_ref.SH_C3
    v = sc.means3D.astype(np.float64) - sc.campos.astype(np.float64)
    n = v / np.linalg.norm(v, axis=1, keepdims=True)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    sh = np.zeros((sc.P, 16, 3))
    k = min(sc.shs.shape[1], (sc.sh_degree + 1) ** 2)
    sh[:, :k] = sc.shs[:, :k]
    val, mag = np.zeros((9, sc.P)), np.zeros((9, sc.P))
    for c in range(3):
        s = lambda i: sh[:, i, c]
        terms = [[], [], []]
        if sc.sh_degree > 0:
            terms[0] += [-C1 * s(3)]; terms[1] += [-C1 * s(1)]; terms[2] += [C1 * s(2)]
        if sc.sh_degree > 1:
            terms[0] += [C2[0] * y * s(4), -2 * C2[2] * x * s(6), C2[3] * z * s(7), 2 * C2[4] * x * s(8)]
            terms[1] += [C2[0] * x * s(4), C2[1] * z * s(5), -2 * C2[2] * y * s(6), -2 * C2[4] * y * s(8)]
            terms[2] += [C2[1] * y * s(5), 4 * C2[2] * z * s(6), C2[3] * x * s(7)]
        if sc.sh_degree > 2:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            terms[0] += [C3[0] * s(9) * 6 * xy, C3[1] * s(10) * yz, C3[2] * s(11) * -2 * xy, C3[3] * s(12) * -6 * xz,
                         C3[4] * s(13) * -3 * xx, C3[4] * s(13) * 4 * zz, C3[4] * s(13) * -yy, C3[5] * s(14) * 2 * xz,
                         C3[6] * s(15) * 3 * xx, C3[6] * s(15) * -3 * yy]
            terms[1] += [C3[0] * s(9) * 3 * xx, C3[0] * s(9) * -3 * yy, C3[1] * s(10) * xz, C3[2] * s(11) * -3 * yy, C3[2] * s(11) * 4 * zz,
                         C3[2] * s(11) * -xx, C3[3] * s(12) * -6 * yz, C3[4] * s(13) * -2 * xy, C3[5] * s(14) * -2 * yz, C3[6] * s(15) * -6 * xy]
            terms[2] += [C3[1] * s(10) * xy, C3[2] * s(11) * 8 * yz, C3[3] * s(12) * 6 * zz, C3[3] * s(12) * -3 * xx, C3[3] * s(12) * -3 * yy,
                         C3[4] * s(13) * 8 * xz, C3[5] * s(14) * xx, C3[5] * s(14) * -yy]
        for a in range(3):
            for tm in terms[a]:
                val[3 * c + a] += tm
                mag[3 * c + a] += np.abs(tm)
    return val, mag


@pytest.mark.parametrize("layout", ["cat", "misaligned"])
@pytest.mark.parametrize("M,D", MD)
@pytest.mark.parametrize("P", [257, 300])
def test_stash_holds_the_nine_derivatives(P, M, D, layout):
    """Bound per entry: 24 float32 unit roundoffs (2^-24) of the sum of the absolute values of its summands.  Each summand is a product
    of a constant, a coefficient and at most two direction components, each of which carries the three roundings of its normalisation
    (sum of squares, root, quotient: <= 4 u with the sum's own), so a summand is within (2 * 4 + 3) u of its value, and the float32 sum of
    up to 11 summands adds at most 10 u of their absolute sum: 21 u, rounded up.  Measured on MI355X: at most 4.2 u."""
    sc = scene(P, M, D)
    fwd, _, _ = run(sc, settings_dict(**FULL_STP), True, layout, records="render")
    vis = (fwd["radii"] > 0).cpu().numpy()
    got = fwd["_stash"].cpu().numpy().astype(np.float64)[:, vis]
    val, mag = _dir_derivatives_f64(sc)
    val, mag = val[:, vis], mag[:, vis]
    u = 2.0 ** -24
    if D == 0:
        assert np.all(got == 0)
        return
    ratio = float(np.max(np.abs(got - val) / (u * np.maximum(mag, 1e-300))))
    print(f"\nP={P} M={M} D={D} {layout}: stash vs float64, largest error = {ratio:.2f} u of the summands' absolute sum")
    assert np.max(mag) > 0 and ratio <= 24.0


# ---- 4. outputs nobody receives -----------------------------------------------------------------------------------------------------------
def _direct_eight(sc, sd, cov3D=None):
    from diff_gaussian_rasterization import _C
    d = dict(sd, _sh_stash=True, _backward_mode="resort")   # (the frame autograd renders with backward_mode="resort": stash, no blend log)
    return _C.rasterize_gaussians_backward(*helpers._direct(sc, d, cov3D=cov3D))


def test_autograd_omits_what_nobody_receives_and_matches_the_direct_call():
    from diff_gaussian_rasterization import _C
    sc, sd = lit(scene(300, 16, 3)), settings_dict(**FULL_STP)   # (two whole backwards: one lit pixel)
    got = api_render(sc, sd, backward_mode="resort")
    ref = _direct_eight(sc, sd)
    assert int((ref[0].abs().sum(1) > 0).sum()) >= 5
    assert len(ref) == 8 and all(t is not None and torch.isfinite(t).all() for t in ref)   # a direct caller: all eight, written in full
    for name, k in (("means2D", 0), ("opacities", 2), ("means3D", 3), ("shs", 5), ("scales", 6), ("rotations", 7)):
        assert torch.equal(got[name], ref[k].view(got[name].shape)), name
    # the private keys themselves: the two slots of the result are None, the other six the same tensors
    args = helpers._direct(sc, dict(sd, _sh_stash=True, _backward_mode="resort", _no_grad_colors=True, _no_grad_cov3D=True))
    lean = _C.rasterize_gaussians_backward(*args)
    assert lean[1] is None and lean[4] is None
    for k in (0, 2, 3, 5, 6, 7):
        assert torch.equal(lean[k], ref[k]), k


def test_colour_gradient_still_arrives_with_colors_precomp():
    sc, sd = helpers._precomp(lit(scene(300, 16, 3))), settings_dict(**FULL_STP)
    got = api_render(sc, sd, backward_mode="resort")
    ref = _direct_eight(sc, sd)
    assert got["colors_precomp"] is not None and float(got["colors_precomp"].abs().max()) > 0
    assert torch.equal(got["colors_precomp"], ref[1])
    for name, k in (("means3D", 3), ("scales", 6), ("rotations", 7)):
        assert torch.equal(got[name], ref[k]), name


def test_cov3D_gradient_still_arrives_with_cov3D_precomp():
    sc, sd = lit(scene(300, 16, 3)), settings_dict(0)   # (a precomputed covariance: GLOBAL mode, the sorted modes need scales and rotations)
    cov = scenes.covariance_from_scale_rotation(sc)
    got = api_render(sc, sd, cov3D=cov)
    ref = _direct_eight(sc, sd, cov3D=cov)
    assert got["cov3D_precomp"] is not None and float(got["cov3D_precomp"].abs().max()) > 0
    assert torch.equal(got["cov3D_precomp"], ref[4])
    for name, k in (("means3D", 3), ("shs", 5)):
        assert torch.equal(got[name], ref[k].view(got[name].shape)), name


# ---- 5. buffers without a stash, and clones ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stash", [False, True], ids=["legacy", "stash"])
def test_cloned_geometry_buffer_is_handled_like_the_original(stash):
    """A clone is described by what it carries: the clone of a stash-carrying buffer is read through its stash, the clone of a buffer
    without one takes the legacy path; either gives the gradients of its original, bit for bit.  (run() itself asserts that a forward
    without the request allocates the plain size and leaves no mark.)"""
    sc, sd = scene(300, 16, 3), settings_dict(**FULL_STP)
    _, g_orig, rec = run(sc, sd, stash, camera=True, records="render")
    _, g_clone, _ = run(sc, sd, stash, camera=True, clone_geom=True, records=rec)
    assert_same(g_orig, g_clone)


def test_inference_forward_writes_no_stash():
    from diff_gaussian_rasterization import _C
    sc, sd = scene(300, 16, 3), settings_dict(**FULL_STP)
    args = helpers._direct(sc, sd)          # no _record_blend_log, no _sh_stash: what a forward under no_grad passes
    assert not _C.has_sh_stash(args[19], sc.P, sd)
    import ctypes
    s = _C.settings_from_dict(sd)
    assert args[19].numel() == _C._load().stp_geometry_buffer_size(sc.P, ctypes.byref(s))
    with torch.no_grad():                    # ... and the public API under no_grad
        got = api_render(sc, sd, gaussians=False, means2D_grad=False, forward_only=True)
    assert got["grad_fn"] is None
