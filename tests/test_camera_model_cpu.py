"""CPU tests (-m "not gpu") of the camera model and the per-Gaussian inputs that scenes.make_scene holds constant: focal_x != focal_y,
an off-centre principal point, a rolled view, scale_modifier != 1, raw (not normalised) quaternions, Gaussians in the clamp band of y.

scenes.vary_inputs varies them; the fp32 oracle is held to the float64 yardstick with the camera as leaves (torch_ref.render_core(
camera_leaves=True): a clamped coordinate is a constant, as in the rasterizer) at the bounds of tests/test_oracle_cpu.py: image 2e-6,
every gradient tensor 5e-5 of its largest entry.  VARIANTS is also the written condition of tests/test_gpu_camera_model.py: the product
is compared with the yardstick on a variant only if the variant is listed here and the oracle passes on it here, in every mode.  The
yardstick's exact per-pixel order is the order of the hierarchical and k-buffer modes only at low density (test_oracle_cpu.py::
test_sorted_modes_agree_at_low_density); the base scene is that sparse, denser frames are compared with the oracle (GPU module, part b).

The reference's quirk, kept and pinned here: dL_dscales carries no factor scale_modifier (its computeCov3D backward scales by
s = mod * scale but returns dot(Rt[i], dL_dMt[i]) without the inner derivative); the true derivative, the yardstick's, is mod times it.
Every comparison below multiplies the oracle's (and the product's) dL_dscales by scale_modifier.

Measured, oracle against yardstick, largest over global_z, global_distance, kbuffer16, hier and hier_full (image max-abs; gradient
tensors relative to the largest entry, the largest over means3D, means2D, opacities, scales * mod, rotations, shs):
    narrow_x     image 6.0e-07   gradients 3.8e-06
    wide_x       image 2.2e-07   gradients 4.7e-06
    narrow_y     image 2.3e-07   gradients 1.5e-06
    off_centre   image 5.1e-07   gradients 2.6e-06
    camera_only  image 4.7e-07   gradients 4.0e-06
    mod06        image 3.9e-07   gradients 3.1e-06
    mod17        image 2.8e-07   gradients 2.6e-06
    raw_quat     image 2.9e-07   gradients 3.3e-06
    combo_a      image 4.2e-07   gradients 2.6e-06
    combo_b      image 5.6e-07   gradients 3.1e-06
    y_band_pair  image 4.0e-07   gradients 7.1e-06
A third of the image bound and a seventh of the gradient bound at the most.  The tests here assert HALF of each bound: a variant on
which the oracle came within a factor 2 of a bound is replaced by a sparser one (a smaller sigma_max or scale_modifier), not kept and
not given a wider bound.  The three input cases' figures are in the docstring of their test.
"""
import numpy as np
import pytest

from helpers import _rel, max_abs, settings_dict
from diff_gaussian_rasterization import scenes
from oracle import oracle as orc
# name -> (settings, the yardstick's order): global_z, global_distance, kbuffer16, hier, hier_full.  One table for the camera tests: the
# module it lives in is marked gpu as a whole, but importing it touches no GPU (its mark applies to its own tests only)
from test_gpu_camera_grad import MODES
import torch_ref
import torch_ref_camera

BASE = dict(P=150, W=40, H=36, sigma_min=1.0, sigma_max=4.0, seed=7, camera="orbit")
OFF, ROLL, RAW = (0.3, -0.2), 0.6, (0.7, 1.4)

VARIANTS = {   # scenes.vary_inputs arguments; "y_band_pair": torch_ref_camera.with_clamped_gaussians(y_band=True) on the plain base scene
    "narrow_x": dict(tanfov_scale=(0.75, 1.0)),
    "wide_x": dict(tanfov_scale=(1.3, 1.0)),
    "narrow_y": dict(tanfov_scale=(1.0, 0.75)),
    "off_centre": dict(principal=OFF),
    "camera_only": dict(tanfov_scale=(1.3, 1.0), principal=OFF, roll=ROLL),
    "mod06": dict(scale_modifier=0.6),
    "mod17": dict(scale_modifier=1.7),
    "raw_quat": dict(quat_norm=RAW),
    "combo_a": dict(tanfov_scale=(1.2, 0.75), principal=OFF, roll=ROLL, scale_modifier=0.8, quat_norm=RAW),
    "combo_b": dict(tanfov_scale=(1.3, 1.0), principal=OFF, roll=ROLL, scale_modifier=0.6, quat_norm=RAW),
    "y_band_pair": None,
}
OFF_CENTRE = tuple(n for n, kw in VARIANTS.items() if kw and "principal" in kw)

IMG_TOL, GRAD_TOL = 2e-6, 5e-5   # tests/test_oracle_cpu.py::test_oracle_matches_float64_autograd


def variant_scene(name, use_sh=True, degree=3):
    sc = scenes.make_scene(**BASE, use_sh=use_sh)
    sc.sh_degree = degree if use_sh else 0
    if VARIANTS[name] is None:
        return torch_ref_camera.with_clamped_gaussians(sc, y_band=True)
    return scenes.vary_inputs(sc, **VARIANTS[name])


def yardstick(name, mode, use_sh=True, degree=3, cov3D=False):
    """(image, {leaf: gradient}) of the float64 yardstick with the camera as leaves; computed once per (variant, order) and shared."""
    kw = MODES[mode][1]
    names = ("viewmatrix", "projmatrix", "campos", "means3D", "means2D", "opacities", "scales", "rotations", "shs", "colors_precomp",
             "cov3D_precomp")

    def make():
        image, g = torch_ref.loss_and_grads(variant_scene(name, use_sh, degree), camera_leaves=True, use_cov3D_precomp=cov3D, **kw)
        return (image,) + tuple(np.zeros(()) if g.get(n) is None else g[n] for n in names)
    out = torch_ref.cached("camera_model", (name, tuple(sorted(kw.items())), use_sh, degree, cov3D), make)
    return out[0], {n: (None if a.ndim == 0 else a) for n, a in zip(names, out[1:])}


def view_ratios(sc):
    """(x / z, y / z, z) of the view-space means, float64"""
    V = np.asarray(sc.viewmatrix, np.float64)
    pv = np.asarray(sc.means3D, np.float64) @ V[:3, :3] + V[3, :3]
    return pv[:, 0] / pv[:, 2], pv[:, 1] / pv[:, 2], pv[:, 2]


def oracle_errors(name, mode):
    """(image error, {leaf: relative error}) of the oracle against the yardstick; dL_dscales times scale_modifier"""
    sc = variant_scene(name)
    f = orc.forward_scene(sc, MODES[mode][0])
    g = f.backward(sc.dL_dout)
    img, tg = yardstick(name, mode)
    errs = {"means3D": _rel(g["dL_dmeans3D"], tg["means3D"]), "means2D": _rel(g["dL_dmeans2D"][:, :2], tg["means2D"]),
            "opacities": _rel(g["dL_dopacity"], tg["opacities"]), "scales": _rel(g["dL_dscales"] * sc.scale_modifier, tg["scales"]),
            "rotations": _rel(g["dL_drotations"], tg["rotations"]), "shs": _rel(g["dL_dsh"], tg["shs"])}
    return max_abs(f.color, img), errs


def _assert_within_half_the_bounds(e_img, errs):
    """The oracle uses at most half of each bound: the product, held to the same bounds on the GPU, keeps the other half for its own
    rounding.  A case that comes closer is replaced by a sparser one, not kept."""
    assert e_img < IMG_TOL / 2, e_img
    for k, v in errs.items():
        assert v < GRAD_TOL / 2, (k, v)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(VARIANTS))
def test_oracle_matches_the_yardstick_on_every_variant(name, mode):
    e_img, errs = oracle_errors(name, mode)
    print(f"\n{name} {mode}: image {e_img:.2e} " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    _assert_within_half_the_bounds(e_img, errs)


INPUT_CASES = {   # variant, mode, use_sh, SH degree, cov3D_precomp: the input kinds tests/test_gpu_camera_model.py adds to the variants
    # (colours on combo_a, not combo_b: there the oracle's image error with precomputed colours is 1.06e-6, more than half the bound)
    "colors_precomp": ("combo_a", "hier_full", False, 0, False),
    "cov3D_precomp": ("combo_a", "global_z", True, 3, True),   # (the sorted modes need scales and rotations)
    "sh1": ("combo_a", "kbuffer16", True, 1, False),
}


@pytest.mark.parametrize("case", list(INPUT_CASES))
def test_oracle_matches_the_yardstick_on_the_input_cases(case):
    """Measured, oracle against yardstick (image max-abs; the largest gradient tensor, relative to its largest entry):
        colors_precomp  image 5.9e-07   gradients 2.1e-06 (scales)
        cov3D_precomp   image 4.2e-07   gradients 6.0e-06 (cov3D_precomp)
        sh1             image 3.9e-07   gradients 1.9e-06 (means3D)"""
    name, mode, use_sh, degree, precomp = INPUT_CASES[case]
    sc = variant_scene(name, use_sh, degree)
    c3 = scenes.covariance_from_scale_rotation(sc) if precomp else None
    f = orc.forward_scene(sc, MODES[mode][0], cov3D_precomp=c3)
    g = f.backward(sc.dL_dout)
    img, tg = yardstick(name, mode, use_sh, degree, precomp)
    pairs = [("dL_dmeans3D", "means3D"), ("dL_dopacity", "opacities"), ("dL_dsh" if use_sh else "dL_dcolors", "shs" if use_sh else "colors_precomp")]
    pairs += [("dL_dcov3D", "cov3D_precomp")] if precomp else [("dL_drotations", "rotations")]
    errs = {b: _rel(g[a], tg[b]) for a, b in pairs}
    if not precomp:
        errs["scales"] = _rel(g["dL_dscales"] * sc.scale_modifier, tg["scales"])
    print(f"\n{case}: image {max_abs(f.color, img):.2e} " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    _assert_within_half_the_bounds(max_abs(f.color, img), errs)


def test_variants_vary_what_they_say():
    """focal_x != focal_y, projmatrix[2, 0:2] != 0, a rolled view with the camera centre in place, quaternion norms over the whole range;
    vary_inputs with its defaults changes nothing but the rounding of inv(viewmatrix @ P)."""
    base = scenes.make_scene(**BASE)
    same = scenes.vary_inputs(base)
    for n in ("viewmatrix", "means3D", "scales", "rotations", "opacities", "shs", "campos", "dL_dout"):
        assert np.array_equal(getattr(same, n), getattr(base, n)), n
    assert max_abs(same.projmatrix, base.projmatrix) < 1e-6 and same.tanfovx == base.tanfovx and same.scale_modifier == 1.0
    sc = variant_scene("combo_a")
    fx, fy = sc.W / (2 * sc.tanfovx), sc.H / (2 * sc.tanfovy)
    assert abs(fx / fy - 0.75 / 1.2) < 1e-6
    V, PM = sc.viewmatrix.astype(np.float64), sc.projmatrix.astype(np.float64)
    proj = np.linalg.inv(V) @ PM
    assert abs(proj[2, 0] - OFF[0]) < 1e-5 and abs(proj[2, 1] - OFF[1]) < 1e-5 and abs(proj[0, 0] - 1 / sc.tanfovx) < 1e-5
    assert max_abs(PM @ sc.inv_viewprojmatrix.astype(np.float64), np.eye(4)) < 1e-4
    R0, R1 = base.viewmatrix[:3, :3].astype(np.float64), V[:3, :3]
    rel = R0.T @ R1   # = Rz(roll)
    assert abs(rel[0, 0] - np.cos(ROLL)) < 1e-6 and abs(rel[0, 1] - np.sin(ROLL)) < 1e-6 and abs(rel[2, 2] - 1) < 1e-6
    assert max_abs(-V[3, :3] @ np.linalg.inv(R1), sc.campos) < 1e-5   # the camera centre did not move
    norms = np.linalg.norm(sc.rotations.astype(np.float64), axis=1)
    assert norms.min() < 0.75 and norms.max() > 1.35 and norms.min() >= 0.7 - 1e-6 and norms.max() <= 1.4 + 1e-6
    assert sc.scale_modifier == 0.8


@pytest.mark.parametrize("mod", [0.6, 1.7])
def test_dL_dscales_omits_scale_modifier_like_the_reference(mod):
    """The quirk as a test: the oracle's dL_dscales is the true derivative divided by scale_modifier."""
    name = "mod06" if mod == 0.6 else "mod17"
    sc = variant_scene(name)
    assert sc.scale_modifier == mod
    for mode in ("global_z", "hier_full"):
        g = orc.forward_scene(sc, MODES[mode][0]).backward(sc.dL_dout)
        true = yardstick(name, mode)[1]["scales"]
        assert _rel(g["dL_dscales"], true) > 1e-1
        assert _rel(g["dL_dscales"], true / mod) < GRAD_TOL


def _visible_in_y_band(sc):
    _, ry, _ = view_ratios(sc)
    radii = orc.forward_scene(sc, settings_dict(0)).radii
    return (np.abs(ry) > 1.3 * sc.tanfovy) & (radii > 0)


@pytest.mark.parametrize("name", ["narrow_y", "y_band_pair"])
def test_the_y_band_is_populated_and_matters(name):
    """At least two visible Gaussians with |y / z| > 1.3 tan_fovy, on both sides; the oracle's dL_dmeans3D is the yardstick's that treats
    the clamped coordinate as a constant, and it is NOT the derivative of clamp(y / z) * z, which differs visibly on these Gaussians."""
    sc = variant_scene(name)
    band = _visible_in_y_band(sc)
    _, ry, _ = view_ratios(sc)
    assert int(band.sum()) >= 2 and (ry[band] > 0).any() and (ry[band] < 0).any(), (int(band.sum()), ry[band])
    if name == "y_band_pair":
        rx = view_ratios(sc)[0]
        assert band[-2:].all() and np.all(np.abs(rx[-2:]) < sc.tanfovx)   # the appended y pair: in the y band alone
    g = orc.forward_scene(sc, MODES["global_z"][0]).backward(sc.dL_dout)
    leaf = yardstick(name, "global_z")[1]["means3D"]
    _, through = torch_ref.loss_and_grads(sc, order="global", depth_key="z")   # differentiates clamp(y / z) * z
    scale = float(np.max(np.abs(leaf)))
    e_leaf, e_through = max_abs(g["dL_dmeans3D"][band], leaf[band]) / scale, max_abs(g["dL_dmeans3D"][band], through["means3D"][band]) / scale
    print(f"\n{name}: {int(band.sum())} visible in the y band; dL_dmeans3D there against the camera-leaf yardstick {e_leaf:.2e}, against clamp * z {e_through:.2e}")
    assert e_leaf < GRAD_TOL
    assert e_through > 10 * GRAD_TOL   # no match by an order of magnitude (measured: 4.5e-3 and 1.4e-3)


def test_existing_clamped_scenes_are_unchanged():
    """with_clamped_gaussians without the new argument appends the x pair alone, and the y pair comes behind it."""
    base = scenes.make_scene(**BASE)
    a, b = torch_ref_camera.with_clamped_gaussians(base), torch_ref_camera.with_clamped_gaussians(base, y_band=True)
    assert a.P == base.P + 2 and b.P == base.P + 4
    for n in ("means3D", "scales", "rotations", "opacities", "shs"):
        assert np.array_equal(getattr(b, n)[:a.P], getattr(a, n)), n
