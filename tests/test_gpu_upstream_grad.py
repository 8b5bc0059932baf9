"""GPU tests (-m gpu) of the render backwards under structured upstream gradients (upstream_patterns.py).

Every other gradient test feeds a dense N(0,1) image and compares with the largest difference relative to the tensor's largest entry.
The on-chip sums of three of the five backward paths are a per-tile fixed point whose scale comes from the tile's largest |dL/dpixel|
(stp_render_hier.inc: "on-chip gradient window"), so the paths for a tile of zeros, for exponents away from 2 and for a large dynamic range
inside a tile or between tiles never ran, and a Gaussian with a small gradient could be wrong unseen.  Here:

  (a) the colour gradient Gaussian by Gaussian against the float64 yardstick's bound B = K u A + Q (torch_ref_colour_bound.py), K four
      times the CPU oracle's own constant, on all five paths under all seven patterns;
  (b) every gradient tensor against the oracle at density (the sliding window, the long lists), once more restricted to the Gaussians
      outside the hot tile; exact zeros where the upstream gradient is zero;
  (c) a non-finite pixel, in all channels or in one, reaches every Gaussian blended there and stays inside its tile.
"""
import numpy as np
import pytest
import torch

from helpers import FULL_STP, _scene_a, _scene_b, api_render, max_abs, settings_dict
from test_gpu_absgrad import YARD_CASES
from test_gpu_parity import FLIP_STATS, GRAD_KEYS, _rel, check_against_oracle
import torch_ref_colour_bound as cb
import upstream_patterns as up

pytestmark = pytest.mark.gpu

IDS = [f"{m}-{bm or 'own'}" for m, bm in YARD_CASES]


def _yard(mode, camera, name):
    """(scene, image, w, pattern, terms) of the yardstick: cached per (camera, order)."""
    order = up.MODES[mode][1]
    sc = up.yard_scene(camera)
    img, w = cb.weights(sc, order=order, key=(camera, order))
    dL = up.patterns(sc)[name]
    return sc, img, w, dL, cb.bound_terms(w, dL, sc.W, sc.H)


# ---- (a) the yardstick, Gaussian by Gaussian -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", up.PATTERNS)
@pytest.mark.parametrize("camera", up.CAMERAS)
@pytest.mark.parametrize("mode,backward_mode", YARD_CASES, ids=IDS)
def test_colour_gradient_inside_its_bound(mode, backward_mode, camera, name):
    """|colors_precomp.grad - grad| <= B for every Gaussian and channel (B = 0 where A = 0: exact zeros); the image to 2e-6.
    Largest share of B used on MI355X: 0.11 under n01 and its powers of two on every path; 0.81 under hot_pixel and 0.34 under hot_tile /
    one_tile on the three fixed-point paths (the figures of the CPU model of that fixed point), 0.14 .. 0.17 on the other two; 0.25 under
    trainer.  Per path and pattern: DESIGN.md section 4, profiles/EXPERIMENTS.md."""
    sd, _, fixed = up.MODES[mode]
    sc, img, w, dL, t = _yard(mode, camera, name)
    got = api_render(sc, sd, w=dL, backward_mode=backward_mode)
    B = cb.bound(t, up.K_of(mode), fixed[backward_mode])
    g = got["colors_precomp"].cpu().numpy()
    use = cb.use_of_bound(g, t, B)
    err_img = max_abs(got["color"].cpu().numpy(), img)
    hot = up.hot_tile_mask(sc)
    cold = (t["A"] > 0).any(1) & ~(w[hot] > 0).any(0)
    zero = (t["A"] == 0).all(1) & (got["radii"].cpu().numpy() > 0)
    print(f"\n{mode} {backward_mode} {camera} {name}: K {up.K_of(mode):.0f}, share of B used {use:.3g}, image {err_img:.2e}, "
          f"{int(cold.sum())} cold, {int(zero.sum())} visible with A = 0, nonzero where zero is due: {int((g[t['A'] == 0] != 0).sum())}")
    if backward_mode == "replay":
        assert got["tile_flags"] is not None and not got["tile_flags"].any(), "the replay kernel did not run"
    if name in up.HOT_PATTERNS:
        assert int(cold.sum()) >= 50
    if name == "one_tile":
        assert int(zero.sum()) >= 40
    assert err_img < 2e-6
    assert np.isfinite(g).all()
    assert use <= 1.0


# ---- (b) the oracle at density, every output ---------------------------------------------------------------------------------------
DENSE = {
    "a-hier_full": (_scene_a, settings_dict(**FULL_STP)),
    "b-hier": (_scene_b, settings_dict(3)),
    "b-hier_full": (_scene_b, settings_dict(**FULL_STP)),
    "b-kbuffer16": (_scene_b, settings_dict(2, per_pixel=16)),
}


@pytest.mark.parametrize("name", ["hot_tile", "trainer", "one_tile"])
@pytest.mark.parametrize("backward_mode", ["replay", "resort"])
@pytest.mark.parametrize("case", list(DENSE))
def test_dense_frames_against_the_oracle(case, backward_mode, name):
    """check_against_oracle as it is, with the pattern as the scene's upstream gradient; then its gradient measure again over the COLD
    Gaussians alone -- visible, without an entry in tile 0's list -- whose largest entry the hot tile's Gaussians no longer set; under
    one_tile every Gaussian without an entry in tile 0 has all-zero gradients, exactly."""
    make, sd = DENSE[case]
    sc = make()
    up.with_upstream(sc, up.patterns(sc)[name])
    before = FLIP_STATS["flipped_frames"]
    g, f = check_against_oracle(sc, {**sd, "_backward_mode": backward_mode})
    tol = 1e-4 if FLIP_STATS["flipped_frames"] == before else 2e-3
    og = f.backward(sc.dL_dout)
    r0, r1 = f.array("ranges").reshape(-1, 2)[0]
    in_tile0 = np.zeros(sc.P, bool)
    in_tile0[f.array("point_list")[int(r0):int(r1)]] = True
    cold = (f.radii > 0) & ~in_tile0
    assert in_tile0.any() and int(cold.sum()) >= 150
    moving = np.zeros(sc.P, bool)
    for k in GRAD_KEYS:
        if g.grads.get(k) is None or og[k].size == 0:
            continue
        a, b = g.grads[k][cold], og[k][cold]
        if k == "dL_dmeans2D":
            a, b = a[:, :2], b[:, :2]
        r = _rel(a, b)
        moving |= (og[k].reshape(sc.P, -1) != 0).any(1)
        print(f"\n{case} {backward_mode} {name} {k}: cold {int(cold.sum())}, rel err over them {r:.2e} (tolerance {tol:g})")
        assert r < tol, k
        if name == "one_tile":
            assert not og[k][~in_tile0].any() and not g.grads[k][~in_tile0].any(), k
    if name != "one_tile":   # (the cold Gaussians do have gradients: 178 .. 221 of scene a's 300, more than 1000 of scene b's 2500 are cold)
        assert int((moving & cold).sum()) > (300 if sc.P > 300 else 100)


# ---- (c) non-finite containment ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [(0, 1, 2), (1,)], ids=["rgb", "g"])
@pytest.mark.parametrize("poison", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("camera", up.CAMERAS)
@pytest.mark.parametrize("mode,backward_mode", YARD_CASES, ids=IDS)
def test_non_finite_pixel_stays_in_its_tile(mode, backward_mode, camera, poison, channels):
    """hot_tile with pixel (5, 9) of tile (0, 0) set to inf / nan, in all channels or in one.  Every Gaussian blended at that pixel has a
    non-finite colour gradient in every poisoned channel; every Gaussian with no blended pixel in that tile is finite and inside its B of
    the run without the poison.  With one channel poisoned only some of a pair's terms are non-finite (that channel's colour term and the
    geometric ones): a range check that takes the terms' maximum with fmaxf loses the NaN and sends it through the fixed point's integer
    conversion, from which it comes back finite -- the re-sorting hierarchical backward did, until its check summed the magnitudes.
    Nothing is asserted for the other channels at that pixel, nor for the Gaussians in between -- blended in the tile, not at the pixel:
    the replay kernel switches a lane off through its factors, and a switched-off lane's 0 * nan can reach the lanes it is merged with."""
    sd, _, fixed = up.MODES[mode]
    sc, img, w, dL, t = _yard(mode, camera, "hot_tile")
    py, px = 9, 5
    bad = dL.copy()
    bad[list(channels), py, px] = poison
    got = api_render(sc, sd, w=bad, backward_mode=backward_mode)
    g = got["colors_precomp"].cpu().numpy()
    at_pixel = w[py * sc.W + px] > 0
    outside = ~(w[up.hot_tile_mask(sc)] > 0).any(0)
    assert int(at_pixel.sum()) >= 3 and int((outside & (t["A"] > 0).any(1)).sum()) >= 50
    hit = g[at_pixel][:, list(channels)]
    assert not np.isfinite(hit).any(), hit
    assert np.isfinite(g[outside]).all()
    B = cb.bound(t, up.K_of(mode), fixed[backward_mode])
    err = np.abs(g[outside].astype(np.float64) - t["grad"][outside])
    assert np.all(err <= B[outside]), float(np.max(err / np.maximum(B[outside], 1e-300)))
    assert max_abs(got["color"].cpu().numpy(), img) < 2e-6
