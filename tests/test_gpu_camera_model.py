"""GPU tests (-m gpu) of the camera model and the per-Gaussian inputs that scenes.make_scene holds constant (scenes.vary_inputs):
focal_x != focal_y, an off-centre principal point, a rolled view, scale_modifier != 1, raw quaternions, Gaussians in the clamp band of y.

  a. the product against the float64 yardstick with the camera as leaves, on the tiny variants of tests/test_camera_model_cpu.py (the
     oracle meets the same bounds on each of them there: that is the condition for a yardstick comparison in a sorted mode), in every
     mode with a backward and both backward modes; image 2e-6, every gradient tensor 5e-5 of its largest entry -- the Gaussian ones and
     dL/dviewmatrix, dL/dprojmatrix, dL/dcampos.  dL_dscales is compared after multiplying by scale_modifier (the reference's quirk,
     INTEGRATION.md section 4; pinned in the CPU module);
  b. the product against the oracle on dense frames, where the yardstick's exact order is not the modes' order: check_against_oracle
     as it is (state, keys, lists and ranges bit for bit, gradients 1e-4);
  c. the opt-in outputs that read the camera: inverse depth against its yardstick, the translation gauge on a 20 000-Gaussian frame;
  d. a tile-row window of an off-centre frame is the full frame's rows, bit for bit.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import CAMERA, FULL_STP, GpuRun, _rel, api_render, max_abs, settings_dict
from diff_gaussian_rasterization import scenes
from golden.make_ref_golden import GOLD   # the fixtures' scene, one definition (the generator only adds tests/ to sys.path on import, as conftest.py has already)
from test_camera_model_cpu import INPUT_CASES, OFF, OFF_CENTRE, RAW, ROLL, VARIANTS, variant_scene, yardstick
from test_gpu_camera_grad import MODES, _check_against_reference, _gauge_residual, cov6
from test_gpu_parity import DENSE, check_against_oracle
import test_gpu_invdepth as tgi
import torch_ref_invdepth as tri

pytestmark = pytest.mark.gpu

render = functools.partial(api_render, camera=CAMERA)
CAMERA_ONLY = VARIANTS["camera_only"]


def _against_yardstick(sc, sd, img, ref, backward_mode, names, cov=None):
    got = render(sc, sd, backward_mode=backward_mode, cov3D=cov)
    assert got["grad_fn"] == "_RasterizeGaussiansCameraBackward"
    e_img = max_abs(got["color"].cpu().numpy(), img)
    if got["scales"] is not None:
        got["scales"] = got["scales"] * sc.scale_modifier
    print(f"\nimage {e_img:.2e} " + " ".join(f"{n} {_rel(got[n].cpu().numpy(), ref[n]):.2e}" for n in names if ref[n] is not None))
    assert e_img < 2e-6
    _check_against_reference(got, ref, names=names)
    assert torch.all(got["viewmatrix"][:, 3] == 0) and torch.all(got["projmatrix"][:, 2] == 0)   # entries the forward never reads
    return got


# ---- a. against the float64 yardstick ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backward_mode", ["replay", "resort"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(VARIANTS))
def test_product_matches_the_yardstick_on_every_variant(name, mode, backward_mode):
    sc = variant_scene(name)
    img, ref = yardstick(name, mode)
    got = _against_yardstick(sc, MODES[mode][0], img, ref, backward_mode, ("means3D", "opacities", "scales", "rotations", "shs") + CAMERA)
    if name in OFF_CENTRE:
        # the row of the principal point: finite, a visible part of the yardstick's gradient, and the yardstick's
        gp, rp = got["projmatrix"].cpu().numpy(), ref["projmatrix"]
        assert np.isfinite(gp[2, 0:2]).all()
        assert np.min(np.abs(rp[2, 0:2])) > 1e-3 * np.max(np.abs(rp))
        assert max_abs(gp[2, 0:2], rp[2, 0:2]) < 5e-5 * np.max(np.abs(rp))


@pytest.mark.parametrize("case,backward_mode", [("colors_precomp", "replay"), ("cov3D_precomp", "replay"), ("sh1", "resort")])
def test_product_matches_the_yardstick_on_the_input_cases(case, backward_mode):
    name, mode, use_sh, degree, precomp = INPUT_CASES[case]
    sc = variant_scene(name, use_sh, degree)
    img, ref = yardstick(name, mode, use_sh, degree, precomp)
    names = ("means3D", "opacities") + (("cov3D_precomp",) if precomp else ("scales", "rotations")) + (("shs",) if use_sh else ("colors_precomp",))
    got = _against_yardstick(sc, MODES[mode][0], img, ref, backward_mode, names + CAMERA, cov=cov6(sc) if precomp else None)
    if not use_sh:
        assert torch.all(got["campos"] == 0)   # no view-direction dependence


# ---- b. against the oracle at density ---------------------------------------------------------------------------------------------
# Raw quaternions down to |q| = 0.7 reach |q|^2 = 1/2, where the matrix built from them, (1 - |q|^2) I + |q|^2 R, is near singular for
# half-turns and a LARGE splat's covariance gradients are ill-conditioned in fp32.  The two fixed frames were
# checked for it: the worst visible Gaussians have a singular-value ratio of 0.033 (GOLD, radius 16 px) and 0.012 (DENSE, radius 10 px),
# small splats whose gradients are small against the tensor's largest entry; product against oracle, the largest of two replay and one
# re-sorting backward over every case below: 2.3e-5 on the raw_quat and combo_mod17 frames, a quarter of the bound.  Another seed or P
# needs that check again.
DENSE_VARIANTS = {
    "camera_only": CAMERA_ONLY,
    "mod17": dict(scale_modifier=1.7),
    "raw_quat": dict(quat_norm=RAW),
    "combo_mod17": dict(CAMERA_ONLY, scale_modifier=1.7, quat_norm=RAW),
}
DENSE_SETTINGS = {
    "global_ptd_max_rect_tbc": settings_dict(0, order=3, rect=True, tbc=True),
    "kbuffer16_tbc": settings_dict(2, per_pixel=16, tbc=True),
    "hier_cull": settings_dict(3, h44=True),
    "full_stp": settings_dict(**FULL_STP),
}


@pytest.mark.parametrize("sd", list(DENSE_SETTINGS))
@pytest.mark.parametrize("variant", list(DENSE_VARIANTS))
@pytest.mark.parametrize("scene", ["gold", "dense"])
def test_dense_frames_against_the_oracle(scene, variant, sd):
    """view_ray, Sigma^-1 with the modifier, the culling paths and the replay backward on an asymmetric frustum with long lists."""
    sc = scenes.vary_inputs(scenes.make_scene(**(GOLD if scene == "gold" else DENSE)), **DENSE_VARIANTS[variant])
    check_against_oracle(sc, DENSE_SETTINGS[sd])


def test_dense_frame_proper_ewa_scaling_against_the_oracle():
    sc = scenes.vary_inputs(scenes.make_scene(**GOLD), **DENSE_VARIANTS["combo_mod17"])
    check_against_oracle(sc, settings_dict(**{**FULL_STP, "ewa": True}))


# ---- c. the opt-in outputs that read the camera -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,backward_mode", [("hier_full", "replay"), ("kbuffer16", "resort")])
def test_inverse_depth_on_the_camera_only_variant(mode, backward_mode):
    """The comparison of tests/test_gpu_invdepth.py::test_against_the_float64_yardstick (image and invdepth 2e-6, gradients 5e-5), camera
    leaves included: the output depends on view-space z, which a rolled, off-centre, fx != fy camera must leave alone."""
    sc = variant_scene("camera_only")
    w, wD = tri.weights(sc)
    ref = tri.reference(sc, w, wD, camera_leaves=True, **tgi.MODES[mode][1])
    got = tgi.run(sc, tgi.MODES[mode][0], invdepth=True, alpha=True, wD=wD, backward_mode=backward_mode, camera=CAMERA)
    e_img, e_inv = max_abs(got["color"].cpu().numpy(), ref["image"]), max_abs(got["invdepth"][0].cpu().numpy(), ref["invdepth"])
    print(f"\n{mode} {backward_mode}: image {e_img:.2e} invdepth {e_inv:.2e}")
    assert e_img < 2e-6 and e_inv < 2e-6
    assert torch.equal(got["alpha"][0], 1.0 - got["final_T"].view(sc.H, sc.W))
    tgi.check_grads(got, ref["grads"], 5e-5, names=tgi.GAUSS + CAMERA)


def test_translation_gauge_with_a_varied_camera():
    """tests/test_gpu_camera_grad.py::test_translation_gauge_full_size's identity and bound (1e-7 of the magnitude) with fx != fy, an
    off-centre principal point, a roll and scale_modifier = 0.6."""
    sc = scenes.vary_inputs(scenes.make_scene(P=20000, W=256, H=256, sigma_min=1.0, sigma_max=10.0, seed=13, camera="orbit"),
                            **CAMERA_ONLY, scale_modifier=0.6)
    got = render(sc, settings_dict(**FULL_STP))
    for n in CAMERA + ("means3D",):
        assert torch.isfinite(got[n]).all(), n
    res, scale = _gauge_residual(sc, got)
    print(f"\ngauge residual {res} / magnitude {scale} = {np.abs(res) / scale}")
    assert np.all(scale > 0) and np.all(np.abs(res) <= 1e-7 * scale), (res, scale)


# ---- d. a tile-row window ---------------------------------------------------------------------------------------------------------
def test_tile_row_windows_of_an_off_centre_frame_paste_to_the_full_frame():
    """tests/test_gpu_parity.py::test_tile_row_windows_paste_to_the_full_frame with the principal point off the centre: the rows' view
    rays come from the same inv_viewprojmatrix whichever window renders them."""
    sc = scenes.vary_inputs(scenes.make_scene(P=8000, W=176, H=144, sigma_min=1.0, sigma_max=10.0, seed=8, camera="orbit"),
                            tanfov_scale=(1.3, 1.0), principal=OFF, roll=ROLL)
    sd = settings_dict(**FULL_STP)
    full = GpuRun(sc, sd, backward=False)
    assert full.num_rendered > 0
    img = np.zeros_like(full.color)
    for rows in ((0, 2), (2, 5), (5, 9)):
        part = GpuRun(sc, sd, backward=False, tile_rows=rows)
        assert np.array_equal(part.radii, full.radii)
        img[:, rows[0] * 16:rows[1] * 16] = part.color[:, rows[0] * 16:rows[1] * 16]
    assert np.array_equal(img, full.color)
