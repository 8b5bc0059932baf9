"""CPU tests (-m "not gpu"): the oracle against OUTPUTS OF THE REFERENCE ITSELF.

tests/golden/ref/*.npz were produced on an MI355X by the reference's own cuda_rasterizer sources -- translated by the
ROCm image's hipify-perl, compiled by hipcc with -ffp-contract=off (oracle/ref_build/build_ref.sh; generator:
tests/golden/make_ref_golden.py).  That build gives every +,-,*,/ and sqrt of the reference one IEEE meaning, so a
faithful CPU restatement has to reproduce, BIT FOR BIT:
    num_rendered, radii, tiles_touched, point_offsets, every per-Gaussian state array, the 64-bit sort keys, the
    sorted Gaussian list, the tile ranges, n_contrib, markVisible,
in every sort mode / order / culling / queue-size combination the fixtures hold.  Two documented exceptions:
  * rects2D under tight_opacity_bounding: <= 2 ulp (one logf: the device library's vs the oracle's rounded double log);
  * depthAlongRay: the oracle's default evaluation (like the default product library's since round 4) is the reference's
    uncontracted expression, which is what this build of the reference computes: checked exactly.  The switch
    "ieee_depth"=0 selects the fused multiply-add order of the second product library (libstp_raster_fma.so; the CUDA
    reference leaves contraction to nvcc): checked at tolerance.
Blend results (libm expf on one side, the device's on the other): image <= 2e-6, gradients <= 2e-5 of the largest entry.
"""
import glob
import hashlib
import json
import os

import numpy as np
import pytest

from diff_gaussian_rasterization import scenes
from oracle import oracle as orc

REF_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref")
FIXTURES = sorted(glob.glob(os.path.join(REF_DIR, "*.npz")))
GRADS = ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")


def _ulps(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return int(np.max(np.abs(a - b))) if a.size else 0


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)) if a.size else 0.0


def _scene_hash(sc, scalars=False):
    """scalars: with tanfovx, tanfovy and scale_modifier, as the generator hashes the fixtures that carry inputs_json"""
    h = hashlib.sha256()
    for a in (sc.means3D, sc.scales, sc.rotations, sc.opacities, sc.shs, sc.colors_precomp, sc.viewmatrix, sc.projmatrix,
              sc.inv_viewprojmatrix, sc.campos, sc.bg, sc.dL_dout):
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    if scalars:
        h.update(np.array([sc.tanfovx, sc.tanfovy, sc.scale_modifier], np.float64).tobytes())
    return h.hexdigest()


def load_case(path):
    z = np.load(path)
    sc = scenes.make_scene(**json.loads(str(z["scene_json"])))
    if "inputs_json" in z.files:   # scenes.vary_inputs arguments (tests/golden/make_ref_golden.py: a case's `inputs`)
        sc = scenes.vary_inputs(sc, **json.loads(str(z["inputs_json"])))
    assert _scene_hash(sc, scalars="inputs_json" in z.files) == str(z["scene_sha256"]), "the seeded scene generator no longer reproduces the fixture's inputs"
    sd = json.loads(str(z["settings_json"]))
    c3 = z["cov3D_precomp"] if "cov3D_precomp" in z.files else None
    return z, sc, sd, c3


def test_fixtures_present_and_from_the_reference():
    assert len(FIXTURES) >= 20
    for p in FIXTURES:
        assert "hipify-perl + hipcc" in str(np.load(p)["reference_build"]) and "-ffp-contract=off" in str(np.load(p)["reference_build"])


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_oracle_reproduces_the_reference(path):
    z, sc, sd, c3 = load_case(path)
    depth = bool(z["render_depth"])
    f = orc.forward_scene(sc, sd, cov3D_precomp=c3, render_depth=depth)
    g = None if depth else f.backward(sc.dL_dout)
    # ---- integer / index results: exact
    assert f.num_rendered == int(z["num_rendered"])
    assert np.array_equal(f.radii, z["radii"])
    assert np.array_equal(f.array("tiles_touched"), z["state_tiles_touched"])
    assert np.array_equal(f.array("point_offsets"), z["state_point_offsets"])
    assert np.array_equal(orc.mark_visible(sc.means3D, sc.viewmatrix, sc.projmatrix), z["mark_visible"])
    # ---- per-Gaussian state: bit-exact (visible Gaussians; the reference never writes the others)
    vis = z["radii"] > 0
    tight = sd["culling_settings"]["tight_opacity_bounding"]
    for k in z.files:
        if not k.startswith("state_") or k in ("state_tiles_touched", "state_point_offsets"):
            continue
        nm = k[6:]
        if nm in ("rgb", "clamped") and sc.shs is None:
            continue      # precomputed colours: the reference does not touch geom.rgb / clamped
        if nm == "cov3D" and c3 is not None:
            continue      # precomputed covariance: the reference does not touch geom.cov3D
        a, b = f.array(nm).reshape(sc.P, -1)[vis], z[k][vis]
        if nm == "clamped":
            assert np.array_equal(a, b)
        elif nm == "rects2D" and tight:
            assert _ulps(a, b) <= 2
        else:
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), nm
    # ---- binning: 64-bit keys, sorted list, ranges: exact
    if f.num_rendered:
        assert np.array_equal(f.array("keys"), z["keys"])
        assert np.array_equal(f.array("point_list"), z["point_list"])
        assert np.array_equal(f.array("ranges"), z["ranges"])
    # ---- blend results
    assert float(np.max(np.abs(f.color.astype(np.float64) - z["color"].astype(np.float64)))) <= 2e-6
    if not depth:   # (the reference's debug-visualisation kernels do not maintain final_T / n_contrib)
        assert float(np.max(np.abs(f.array("final_T") - z["final_T"]))) <= 2e-6
        if "n_contrib" in z.files:
            assert np.array_equal(f.array("n_contrib"), z["n_contrib"])
        for k in GRADS:
            a, b = g[k], z["grad_" + k]
            if k == "dL_dmeans2D":
                a, b = a[:, :2], b[:, :2]                       # .z is unused (ref: backward.cu:498-499)
            if k == "dL_dconic":
                a, b = a.reshape(-1, 4)[:, [0, 1, 3]], b.reshape(-1, 4)[:, [0, 1, 3]]   # (xx, xy, ., yy)
            assert _rel(a, b) <= 2e-5, k


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_fma_depth_keys_stay_within_rounding_of_the_reference(path):
    """The oracle's fused-multiply-add depthAlongRay (switch ieee_depth=0, the order libstp_raster_fma.so shares) against the
    same fixtures: depth keys within a few ulp, the sorted list equal up to a handful of neighbour swaps, image >= 60 dB."""
    z, sc, sd, c3 = load_case(path)
    depth = bool(z["render_depth"])
    orc.set_flag("ieee_depth", 0)
    try:
        f = orc.forward_scene(sc, sd, cov3D_precomp=c3, render_depth=depth)
    finally:
        orc.set_flag("ieee_depth", 1)
    assert f.num_rendered == int(z["num_rendered"]) and np.array_equal(f.radii, z["radii"])
    if f.num_rendered:
        ka, kb = f.array("keys"), z["keys"]
        assert np.array_equal(ka >> np.uint64(32), kb >> np.uint64(32))                     # tile ids
        da = (ka & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)
        db = (kb & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)
        swapped = f.array("point_list") != z["point_list"]
        assert int(swapped.sum()) <= max(4, int(2e-3 * swapped.size))
        assert _ulps(np.sort(da), np.sort(db)) <= 64
        assert np.array_equal(f.array("ranges"), z["ranges"])
    d = f.color.astype(np.float64) - z["color"].astype(np.float64)
    mse = float(np.mean(d ** 2))
    assert mse == 0 or 10 * np.log10(1.0 / mse) >= 60.0
