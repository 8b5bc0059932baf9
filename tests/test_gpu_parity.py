"""GPU parity tests (-m gpu): the HIP path, called through the public drop-in API (GaussianRasterizer ->
autograd -> _C -> C ABI of libstp_raster.so), against the CPU oracle on the same seeded inputs.

Tolerances (north_star: "within a stated fp32 tolerance, PSNR >= 60 dB"):
  * integer / index work (radii, tile counts, offsets, 64-bit sort keys, sorted lists, tile ranges): bit-exact;
  * per-Gaussian fp32 state (means2D, conics, depths, Sigma^-1 ...): bit-exact (the one logarithm on the path,
    tight_opacity_bounding's extent, is rounded from double precision on both sides);
  * image: max-abs <= 2e-6 and PSNR >= 100 dB (the blend loops may contract a*b+c, expf differs by an ulp);
  * gradients: max-abs error <= 1e-4 of the largest entry (atomic / LDS-atomic summation order).
"""
import os

import numpy as np
import pytest
import torch

from helpers import FULL_STP, GpuRun, ext_settings, max_abs, oracle_run, psnr, settings_dict
from diff_gaussian_rasterization import scenes

pytestmark = pytest.mark.gpu

GRAD_KEYS = ("dL_dmeans2D", "dL_dopacity", "dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dsh", "dL_dcolors")


def _rel(a, b):
    return max_abs(a, b) / max(float(np.max(np.abs(b))), 1e-30) if np.size(b) else 0.0


FLIP_STATS = {"flipped_frames": 0, "closed_by_nudge": 0}  # (tools/fuzz_parity.py prints them: how many frames with a decision on its threshold, how many the nudged oracle closed)


def _matches_a_nudged_oracle(scene, sd, g, backward, img_tol, grad_tol, ex, tile_rows=None, max_tries=25):
    """A frame with an explained threshold decision: is the product's WHOLE output -- image to img_tol, every gradient tensor to grad_tol, the tolerances of a
    frame without any such decision -- the oracle's with that decision taken the other way?  The oracle is re-run (a) with exactly the alpha tests the
    explanation names inverted (oracle.forced_alpha_flips), then (b) with one of its per-pixel thresholds moved inside the explanation's own band
    (oracle.blend_nudge: 1/255 (1 +- 6e-7), 1e-4 (1 +- 1e-6), the sub-tile culling's alpha; both directions, smallest first).  True = yes, and the frame
    needs no looser tolerance at all; False = fall back to the flipped-frame tolerances (decisions of several kinds, or a pixel with two alphas in the band)."""
    import contextlib
    from oracle import oracle as orc
    tries = []
    if ex and (ex.get("decisions") or ex.get("T_pixels")):
        tries.append(lambda: orc.forced_alpha_flips(ex.get("decisions", []), scene.W, T_pixels=ex.get("T_pixels", [])))
    for frac in (0.1, 0.25, 0.5, 1.0):
        for sign in (1.0, -1.0):
            tries.append(lambda v=sign * frac * 6e-7 / 255.0: orc.blend_nudge(alpha=v))
            tries.append(lambda v=sign * frac * 6e-7 / 255.0: orc.blend_nudge(cull_alpha=v))
            tries.append(lambda v=sign * frac * 1e-6 * 1e-4: orc.blend_nudge(T=v))
    sl = slice(None) if tile_rows is None else slice(16 * tile_rows[0], min(16 * tile_rows[1], scene.H))  # (a window of tile rows of a full-size frame: tests/test_gpu_fullsize.py)
    for ctx in tries[:max_tries]:
        with ctx():
            f2, og2 = oracle_run(scene, sd, backward=backward, tile_rows=tile_rows)
        if np.abs(g.color[:, sl].astype(np.float64) - f2.color[:, sl].astype(np.float64)).max() > img_tol:
            continue
        ok = True
        if backward:
            for k in GRAD_KEYS:
                if g.grads.get(k) is None or og2.get(k) is None or og2[k].size == 0:
                    continue
                a, b = g.grads[k], og2[k]
                if k == "dL_dmeans2D":
                    a, b = a[:, :2], b[:, :2]
                if not _rel(a, b) < grad_tol:
                    ok = False
                    break
        if ok:
            return True
    return False


def check_against_oracle(scene, sd, backward=True, exact_state=True, img_tol=2e-6, grad_tol=1e-4, flip_grad_tol=2e-3):
    """img_tol / grad_tol: the fixed test scenes blend tens of entries per pixel; tools/fuzz_parity.py --heavy (hundreds to
    a thousand blends per pixel, opacities at the 1/255 threshold) passes looser ones -- fp32 rounding accumulates with
    the number of blends, and a faint Gaussian's whole gradient can hang on one threshold decision."""
    g = GpuRun(scene, sd, backward=backward)
    f, og = oracle_run(scene, sd, backward=backward)
    assert g.num_rendered == f.num_rendered
    assert np.array_equal(g.radii, f.radii)
    assert np.array_equal(g.geom_array("tiles_touched").view(np.uint32), f.array("tiles_touched"))
    assert np.array_equal(g.geom_array("point_offsets").view(np.uint32), f.array("point_offsets"))
    vis = f.radii > 0
    for nm, per in (("depths", 1), ("means2D", 2), ("conic_opacity", 4), ("cov3D", 6)):
        a, b = g.geom_array(nm).reshape(-1, per)[vis], f.array(nm).reshape(-1, per)[vis]
        if exact_state:
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), nm
        else:
            assert _rel(a, b) < 1e-6, nm
    if f.num_rendered:
        assert np.array_equal(g.binning_array("keys"), f.array("keys"))
        assert np.array_equal(g.binning_array("point_list"), f.array("point_list"))
        assert np.array_equal(g.image_array("ranges").view(np.uint32), f.array("ranges"))
    # Image: 2e-6 everywhere, except where a DISCRETE decision of the blend loop sits on its threshold and the two sides' exponentials (the
    # device's exp_blend, <= 2 ulp; libm's expf, <= 1 ulp) land on different sides of it -- which moves a pixel by up to 1/255.  Such a pixel is
    # accepted ONLY if it is explained (oracle/explain.py, from state both sides share bit for bit): an entry of its tile list whose alpha --
    # fp32 exponent, exponential in double -- lies within 6e-7 of 1/255 at the pixel; with hierarchical_4x4_culling the same at its 4x4
    # sub-tile's point of maximum contribution (ONE decision there removes an entry from 16 pixels, ref: hierarchical_render.cuh:722-743); or a
    # final transmittance within 1e-6 of the 1e-4 threshold on either side.  No blanket allowance.
    explained_by = None
    diff = np.abs(g.color.astype(np.float64) - f.color.astype(np.float64))
    assert diff.max() <= 1.0 / 255.0 + 1e-6
    moved = diff > img_tol
    flipped = int(moved.sum())
    if flipped or diff.max() > 2e-6:
        from oracle import explain
        probe = lambda mask: explain.explain_moved_pixels(mask, W=scene.W, H=scene.H, ranges=f.array("ranges").reshape(-1), point_list=f.array("point_list"),
                                                          conic_opacity=f.array("conic_opacity").reshape(-1), means2D=f.array("means2D").reshape(-1),
                                                          final_T_a=g.image_array("final_T").reshape(-1), final_T_b=f.array("final_T").reshape(-1),
                                                          cull_4x4=bool(sd["culling_settings"]["hierarchical_4x4_culling"]) and sd["sort_settings"]["sort_mode"] == 3)
        if flipped:
            ex = probe(moved.any(axis=0))
            assert not ex["unexplained"], (flipped, ex["by"], ex["unexplained"][:5])
            explained_by = ex
        elif (ex2 := probe((diff > 2e-6).any(axis=0)))["explained"]:
            explained_by = ex2
            # a decision on its threshold that moved its pixel by less than img_tol (a faint Gaussian deep in a dense scene): the pixel passes as it is,
            # but that Gaussian's gradient still carries the whole blend -- the gradient tolerance of a flipped frame applies
            flipped = 1
    if flipped:
        FLIP_STATS["flipped_frames"] += 1
        if _matches_a_nudged_oracle(scene, sd, g, backward, img_tol, grad_tol, explained_by):
            FLIP_STATS["closed_by_nudge"] += 1
            return g, f
    assert psnr(g.color, f.color) >= (100.0 if flipped == 0 else 75.0)  # (one flipped pixel of a 1600-pixel image: 80 dB)
    # a flipped blend also changes that Gaussian's (and, through the transmittance, its pixel's later Gaussians') gradient
    # terms by the weight of one pixel: 1e-4 of the largest entry when no blend flipped, 2e-3 otherwise
    # (tools/fuzz_parity.py: 2 such scenes in 4000)
    grad_tol = grad_tol if flipped == 0 else flip_grad_tol
    if backward:
        for k in GRAD_KEYS:
            if g.grads.get(k) is None or og.get(k) is None or og[k].size == 0:
                continue
            a, b = g.grads[k], og[k]
            if k == "dL_dmeans2D":
                a, b = a[:, :2], b[:, :2]
            assert _rel(a, b) < grad_tol, k
    return g, f


C1 = dict(P=1000, W=256, H=256, sigma_min=1.0, sigma_max=12.0, seed=1)
DENSE = dict(P=6000, W=96, H=80, sigma_min=2.0, sigma_max=14.0, seed=11, camera="orbit")


@pytest.mark.parametrize("sd", [
    settings_dict(0), settings_dict(0, order=1), settings_dict(0, order=2), settings_dict(0, order=3),
    settings_dict(2, per_pixel=16), settings_dict(3), settings_dict(3, h44=True), settings_dict(**FULL_STP)],
    ids=["global_z", "global_dist", "ptd_center", "ptd_max", "kbuffer16", "hier", "hier_cull", "full_stp"])
def test_c1_all_modes(sd):
    """BASELINE config C1 (1k Gaussians, 256x256) in every sort mode / order, forward + backward."""
    check_against_oracle(scenes.make_scene(**C1), sd)


@pytest.mark.parametrize("sd", [
    settings_dict(0), settings_dict(2, per_pixel=16), settings_dict(2, per_pixel=4, ewa=True), settings_dict(3),
    settings_dict(3, h44=True), settings_dict(**FULL_STP), settings_dict(0, rect=True, tight=True, tbc=True),
    settings_dict(**{**FULL_STP, "ewa": True})],
    ids=["global", "kbuffer16", "kbuffer4_ewa", "hier", "hier_cull", "full_stp", "global_all_culling", "full_stp_ewa"])
def test_dense_scene(sd):
    """~700 Gaussians per tile, off-axis rotated camera: the regime where the resorting queues actually
    reorder and hierarchical != exact sort."""
    check_against_oracle(scenes.make_scene(**DENSE), sd)


@pytest.mark.parametrize("head,mid", [(8, 8), (16, 8), (4, 12), (8, 12), (16, 20), (4, 20)])
def test_hier_queue_sizes(head, mid):
    check_against_oracle(scenes.make_scene(**DENSE), settings_dict(3, per_pixel=head, tile_2x2=mid, h44=True))


@pytest.mark.parametrize("window", [1, 2, 4, 8, 12, 20, 24])
def test_kbuffer_windows(window):
    check_against_oracle(scenes.make_scene(P=3000, W=80, H=64, sigma_min=2.0, sigma_max=12.0, seed=5), settings_dict(2, per_pixel=window))


def test_kbuffer_tile_kernel_forward_passes():
    """STP_KBUFFER=tile (read once per process: a child) sends the k-buffer forwards to the one-entry-per-wave kernel of stp_render_tile.hip
    instead of the wave64 kernels: its recording forward (with the replay as its backward), its plain forward and its depth visualisation,
    each against the oracle with the yardstick of the test that covers the same pass on the default path (test_kbuffer_windows and its scene,
    test_n_contrib_of_the_plain_forward's image bound, test_render_depth_visualisation and its scene)."""
    import os, subprocess, sys
    code = ("import sys, numpy as np; sys.path[:0] = ['tests', 'stopthepop-rasterization_amd', '.']; import conftest;"
            "from helpers import *; from diff_gaussian_rasterization import scenes; import test_gpu_parity as t;"
            "sc = scenes.make_scene(P=3000, W=80, H=64, sigma_min=2.0, sigma_max=12.0, seed=5); sd = settings_dict(2, per_pixel=16);"
            "g, f = t.check_against_oracle(sc, sd);"   # (backward mode 'replay', the default: the forward records the blend log)
            "g = GpuRun(sc, sd, backward=False); f, _ = oracle_run(sc, sd, backward=False);"
            "assert max_abs(g.color, f.color) <= 2e-6;"
            "sc = scenes.make_scene(P=800, W=80, H=64, sigma_min=2.0, sigma_max=8.0, seed=9, camera='orbit', opacity_range=(0.5, 0.95));"
            "g = GpuRun(sc, sd, backward=False, render_depth=True); f, _ = oracle_run(sc, sd, backward=False, render_depth=True);"
            "assert np.ptp(f.color) > 0.5 and max_abs(g.color, f.color) <= 2e-4;"
            "print('tile ok')")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, STP_KBUFFER="tile"), cwd=root)
    assert r.returncode == 0 and r.stdout.endswith("tile ok\n"), r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("mode,window", [(0, 4), (2, 1), (2, 4), (2, 8), (2, 12), (2, 16), (2, 24)])
def test_n_contrib_of_the_plain_forward(mode, window):
    """n_contrib of a forward that records no blend log (inference): GLOBAL = the last contributing list entry + 1
    (ref: forward.cu:352-361), PPX_KBUFFER = the entries a pixel looked at before it saturated (ref: resorted_render.cuh:
    17-221) -- which the wave64 k-buffer kernel does not count but derives from the insertion that filled the window
    (stp_render_kbuf.hip).  Dense scene: most pixels saturate, inside the list and in the final drain."""
    sc = scenes.make_scene(**DENSE)
    sd = settings_dict(mode, per_pixel=window)
    g = GpuRun(sc, sd, backward=False)
    f, _ = oracle_run(sc, sd, backward=False)
    a, b = g.image_array("n_contrib").view(np.uint32).reshape(-1)[:sc.W * sc.H], f.array("n_contrib").reshape(-1)
    assert (b < b.max()).any() and (b == b.max()).any()  # both kinds of pixel occur
    assert np.array_equal(a, b)
    assert max_abs(g.color, f.color) <= 2e-6


def test_ppx_full_forward_and_no_backward():
    sc = scenes.make_scene(P=2500, W=48, H=32, sigma_min=2.0, sigma_max=12.0, seed=5, camera="orbit")  # > 1024 per tile
    check_against_oracle(sc, settings_dict(1), backward=False)
    with pytest.raises(RuntimeError, match="Backward not supported for full per-pixel sort"):
        GpuRun(sc, settings_dict(1), backward=True)


def test_unsupported_queue_sizes_raise():
    sc = scenes.make_scene(P=100, W=32, H=32, sigma_min=1.0, sigma_max=4.0, seed=2)
    with pytest.raises(RuntimeError, match="Not supported head queue size"):
        GpuRun(sc, settings_dict(3, per_pixel=5), backward=False)
    with pytest.raises(RuntimeError, match="Not supported mid queue size"):
        GpuRun(sc, settings_dict(3, tile_2x2=16), backward=False)
    with pytest.raises(RuntimeError, match="Not supported head queue size"):  # 12 exists only in the backward ladder
        GpuRun(sc, settings_dict(3, per_pixel=12), backward=False)


def test_precomputed_colors_and_rgb_gradient():
    check_against_oracle(scenes.make_scene(**{**C1, "use_sh": False, "camera": "orbit"}), settings_dict(3, h44=True))


def test_odd_image_size_and_tiny_inputs():
    check_against_oracle(scenes.make_scene(P=1, W=37, H=19, sigma_min=3.0, sigma_max=3.1, seed=4), settings_dict(3))
    check_against_oracle(scenes.make_scene(P=300, W=1063 // 8, H=97, sigma_min=1.0, sigma_max=9.0, seed=4), settings_dict(**FULL_STP))


def test_everything_culled_and_empty_input():
    import diff_gaussian_rasterization as dgr
    sc = scenes.make_scene(P=64, W=48, H=32, sigma_min=1.0, sigma_max=4.0, seed=2)
    sc.means3D[:, 2] = 0.1  # behind the near plane
    g = GpuRun(sc, settings_dict(3), backward=True)
    assert g.num_rendered == 0 and not g.radii.any()
    assert np.allclose(g.color, np.asarray(sc.bg).reshape(3, 1, 1))
    assert all(v is None or not np.any(v) for v in g.grads.values())
    # P == 0 (reference rasterize_points.cu:93): zero image, no launch
    dev = torch.device("cuda:0")
    z = lambda *s: torch.zeros(*s, device=dev)
    rs = dgr.GaussianRasterizationSettings(32, 48, 0.5, 0.5, z(3), 1.0, torch.eye(4, device=dev), torch.eye(4, device=dev),
                                           torch.eye(4, device=dev), 0, z(3), False, dgr.ExtendedSettings(), False, False)
    color, radii = dgr.GaussianRasterizer(rs)(z(0, 3), z(0, 3), z(0, 1), colors_precomp=z(0, 3), scales=z(0, 3), rotations=z(0, 4))
    assert color.shape == (3, 32, 48) and not color.any() and radii.numel() == 0


def test_mark_visible_matches_oracle():
    import diff_gaussian_rasterization as dgr
    from oracle import oracle as orc
    sc = scenes.make_scene(P=5000, W=64, H=64, sigma_min=1.0, sigma_max=4.0, seed=6, camera="orbit")
    sc.means3D[::7] = sc.campos
    dev = torch.device("cuda:0")
    t = lambda a: torch.tensor(a, device=dev)
    rs = dgr.GaussianRasterizationSettings(64, 64, sc.tanfovx, sc.tanfovy, t(sc.bg), 1.0, t(sc.viewmatrix), t(sc.projmatrix),
                                           t(sc.inv_viewprojmatrix), 3, t(sc.campos), False, dgr.ExtendedSettings(), False, False)
    vis = dgr.GaussianRasterizer(rs).markVisible(t(sc.means3D)).cpu().numpy()
    assert vis.dtype == np.bool_ and np.array_equal(vis, orc.mark_visible(sc.means3D, sc.viewmatrix, sc.projmatrix))


def test_debug_flag_synchronises_and_gives_the_same_frame():
    sc = scenes.make_scene(**DENSE)
    a = GpuRun(sc, settings_dict(**FULL_STP), backward=False)
    b = GpuRun(sc, settings_dict(**FULL_STP), backward=False, debug=True)
    assert np.array_equal(a.color, b.color)


@pytest.mark.parametrize("degree,M", [(0, 16), (1, 16), (2, 9), (1, 4), (0, 1)])
def test_sh_degrees_and_coefficient_counts(degree, M):
    """Active SH degree below the stored one, and SH tensors with fewer coefficients (row lengths 48, 27, 12, 3
    floats: both the 16-byte and the scalar staging path of the per-Gaussian backward)."""
    sc = scenes.make_scene(P=700, W=64, H=48, sigma_min=2.0, sigma_max=9.0, seed=31, camera="orbit")
    sc.shs = np.ascontiguousarray(sc.shs[:, :M, :])
    sc.sh_degree = degree
    g, f = check_against_oracle(sc, settings_dict(3, h44=True))
    assert g.grads["dL_dsh"].shape == (700, M, 3)
    assert not np.any(g.grads["dL_dsh"][:, (degree + 1) ** 2:, :])  # nothing flows into inactive coefficients


@pytest.mark.parametrize("sd", [settings_dict(0), settings_dict(0, order=1), settings_dict(2, per_pixel=16), settings_dict(1),
                                settings_dict(3), settings_dict(**FULL_STP), settings_dict(3, per_pixel=8, tile_2x2=12, h44=True),
                                settings_dict(2, per_pixel=4)],   # (kbuffer4: the k-buffer's register window; kbuffer16 is the ring in LDS)
                         ids=["global_z", "global_dist", "kbuffer16", "ppx_full", "hier", "full_stp", "hier_8_12", "kbuffer4"])
def test_render_depth_visualisation(sd):
    """`render_depth=True` (reference rasterize_points.cu:104-107): sum(depth * alpha * T) per pixel, normalised by the
    frame's extrema, Turbo colormap -- in every sort mode, against the oracle."""
    # (a sparse scene: uncovered pixels put the frame minimum at 0, otherwise the reference's normalisation
    # clamp(v, min, max) / (max - min) saturates almost everywhere)
    sc = scenes.make_scene(P=800, W=80, H=64, sigma_min=2.0, sigma_max=8.0, seed=9, camera="orbit", opacity_range=(0.5, 0.95))
    g = GpuRun(sc, sd, backward=False, render_depth=True)
    f, _ = oracle_run(sc, sd, backward=False, render_depth=True)
    assert g.color.shape == (3, sc.H, sc.W) and g.color.min() >= 0.0 and g.color.max() <= 1.0
    assert np.ptp(f.color) > 0.5  # the test image really spans the colormap
    assert max_abs(g.color, f.color) <= 2e-4  # the colormap's slope multiplies the 1e-6 of the accumulated depth
    # the ordinary image of the same scene is unaffected by the flag's plumbing
    assert np.array_equal(GpuRun(sc, sd, backward=False).color, GpuRun(sc, sd, backward=False, render_depth=False).color)


# ---- blend log (training forward records the blend order, backward replays it) ----
HAZE = dict(P=3000, W=48, H=48, sigma_min=10.0, sigma_max=20.0, seed=21, opacity_range=(0.01, 0.03))


@pytest.mark.parametrize("sd", [settings_dict(3, h44=True), settings_dict(2, per_pixel=16)], ids=["hier", "kbuffer16"])
def test_blend_log_overflow_falls_back_to_the_resorting_backward(sd):
    """Thousands of faint, wide Gaussians: pixels blend far more than BLEND_LOG_DEPTH (256) entries, the recording
    forward flags those tiles and the resorting backward kernel takes them.  Result must not change."""
    sc = scenes.make_scene(**HAZE)
    g, f = check_against_oracle(sc, sd)
    flags = g.image_array("tile_flags")
    assert flags.size == 9 and flags.any(), "scene did not overflow the blend log: test is vacuous"


def test_blend_log_mixed_tiles():
    """Some tiles overflow, the others replay: both backward kernels write into the same gradient arrays."""
    sc = scenes.make_scene(P=5000, W=96, H=64, sigma_min=3.0, sigma_max=16.0, seed=23, opacity_range=(0.01, 0.05))
    sc.opacities[sc.means3D[:, 0] > 0.0] = 0.6  # right half of the image saturates after a few dozen blends
    gk, _ = check_against_oracle(sc, settings_dict(2, per_pixel=8))
    fk = gk.image_array("tile_flags")
    assert fk.any() and not fk.all(), fk
    g, _ = check_against_oracle(sc, settings_dict(**FULL_STP))
    flags = g.image_array("tile_flags")
    assert flags.any() and not flags.all(), flags


def test_resorting_backward_still_selectable():
    """Backward mode "resort" (process-wide: _C.set_backward_mode / STP_BACKWARD at import; per call: settings._backward_mode):
    no log is recorded, the backward re-runs the resort (the reference's scheme)."""
    from diff_gaussian_rasterization import _C
    sc = scenes.make_scene(**DENSE)
    sd = settings_dict(**FULL_STP)
    W, H = sc.W, sc.H
    log_bytes = _C.blend_log_bytes(W, H)
    _C.set_backward_mode("resort")
    try:
        g_resort, _ = check_against_oracle(sc, sd)
    finally:
        _C.set_backward_mode("replay")
    g_replay = GpuRun(sc, sd)
    assert g_replay.img.numel() >= g_resort.img.numel() + log_bytes  # the resorting run really carried no log
    assert np.array_equal(g_resort.color, g_replay.color)  # recording must not change the image
    for k in GRAD_KEYS:
        if g_resort.grads.get(k) is not None:
            assert _rel(g_replay.grads[k], g_resort.grads[k]) < 1e-5, k
    # the same choice per call, through the settings object
    g_call = GpuRun(sc, {**sd, "_backward_mode": "resort"})
    assert g_call.img.numel() == g_resort.img.numel()
    for k in GRAD_KEYS:
        if g_resort.grads.get(k) is not None:
            assert _rel(g_call.grads[k], g_resort.grads[k]) < 1e-5, k   # (the re-sorting backward sums with fp32 atomics: not bit-reproducible)


def test_backward_mode_auto_holds_eight_1080p_forwards_within_a_4GB_log_budget():
    """A trainer that sums K views before ONE backward holds K blend logs (0.6-1.1 GB each at 1080p, by the log depth).  Mode "auto"
    records while live + pooled + new log bytes fit the budget and lets the remaining forwards take the re-sorting backward.  The depth of a
    log is the library's choice (per frame, up to 512 records): a forward that has not run yet is budgeted at the DEEPEST log it may carve, a
    forward that has run is accounted at what its buffer really holds.  Eight un-backpropagated 1080p forwards under a budget of one deepest
    log + 1.5 default ones: some record, some do not, the live bytes never pass the budget, and the gradients of the summed loss equal those of eight replayed
    forwards."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    K = 8
    sc = scenes.make_scene(P=60000, W=1920, H=1080, sigma_min=2.0, sigma_max=12.0, seed=71, camera="orbit")
    dev = torch.device("cuda:0")
    t = lambda a, rg=False: torch.tensor(a, device=dev).requires_grad_(rg)
    es = ext_settings(settings_dict(**FULL_STP))
    rs = dgr.GaussianRasterizationSettings(
        image_height=sc.H, image_width=sc.W, tanfovx=sc.tanfovx, tanfovy=sc.tanfovy, bg=t(sc.bg), scale_modifier=1.0,
        viewmatrix=t(sc.viewmatrix), projmatrix=t(sc.projmatrix), inv_viewprojmatrix=t(sc.inv_viewprojmatrix), sh_degree=sc.sh_degree,
        campos=t(sc.campos), prefiltered=False, settings=es, render_depth=False, debug=False)
    rast = dgr.GaussianRasterizer(rs)
    w = t(sc.dL_dout)
    log_bytes = _C.blend_log_bytes(sc.W, sc.H)
    assert 0.5e9 < log_bytes < 1.2e9
    deepest = _C.blend_log_bytes(sc.W, sc.H, depth=0)
    assert 2.5 * log_bytes < deepest < 2.8 * log_bytes and _C.blend_log_bytes(sc.W, sc.H, depth=192) == log_bytes
    budget = int(deepest + 1.5 * log_bytes)   # the first two forwards (default depth, nothing known about the scene yet) fit, a third might not

    def run(mode, budget):
        _C.clear_scratch_pool(dev)
        _C.set_backward_mode(mode, log_budget_bytes=budget)
        try:
            leaves = [t(sc.means3D, True), torch.zeros(sc.P, 3, device=dev, requires_grad=True), t(sc.opacities, True), t(sc.shs, True),
                      t(sc.scales, True), t(sc.rotations, True)]
            m3, m2, op, sh, scl, rot = leaves
            total, recorded, peak, held = 0.0, 0, 0, 0
            for i in range(K):
                color, _ = rast(m3, m2, op, shs=sh, scales=scl, rotations=rot)
                if getattr(color.grad_fn, "log_lease", None) is not None:   # (the lease says whether a log was recorded)
                    recorded += 1
                    held += _C.blend_log_bytes(sc.W, sc.H, depth=_C.blend_log_depth(color.grad_fn.saved_tensors[11]))
                total = total + (color * w).sum() * (1.0 + 0.125 * i)
                assert _C.live_log_bytes(dev) == held                        # accounted at the depth the buffers were really carved with
                peak = max(peak, _C.live_log_bytes(dev))
            total.backward()
            assert _C.live_log_bytes(dev) == 0   # every lease went back with its backward
            return [x.grad.detach().cpu().numpy() for x in leaves], recorded, peak
        finally:
            _C.set_backward_mode("replay", log_budget_bytes=16 << 30)
            _C.clear_scratch_pool(dev)

    g_auto, n_auto, peak_auto = run("auto", budget)
    assert 2 <= n_auto < K and peak_auto <= budget, (n_auto, peak_auto)   # some logs fit the budget, the rest re-sort
    assert peak_auto + deepest > budget                                   # ... and it stopped because the next one might not have
    g_replay, n_replay, _ = run("replay", None)
    assert n_replay == K
    for a, b in zip(g_auto, g_replay):
        assert _rel(a, b) < 2e-5


def test_forward_without_grad_records_nothing():
    sc = scenes.make_scene(**C1)
    g = GpuRun(sc, settings_dict(3), backward=False)
    W, H = sc.W, sc.H
    n_plain = g.img.numel()
    g2 = GpuRun(sc, settings_dict(3), backward=True)
    from diff_gaussian_rasterization import _C
    assert g2.img.numel() >= n_plain + _C.blend_log_bytes(W, H) > n_plain + ((W + 15) // 16) * ((H + 15) // 16) * 256 * 64 * 2
    assert np.array_equal(g.color, g2.color)


@pytest.mark.parametrize("sd", [settings_dict(3, h44=True), settings_dict(2, per_pixel=16)], ids=["hier", "kbuffer16"])
def test_backward_after_a_render_depth_forward_is_memory_safe(sd):
    """The depth-visualisation forward records no blend log.  (1) Through the public API the backward that follows takes
    the re-sorting path and gives the gradients of the same frame rendered without the log.  (2) At the _C level, a
    backward that is WRONGLY told a log exists (what the autograd function used to do) finds every tile marked "no valid
    log" and re-sorts them all: same gradients, no read of a log that was never allocated."""
    sc = scenes.make_scene(**DENSE)
    g = GpuRun(sc, sd, backward=True, render_depth=True)      # (1) must not fault; gradients are finite
    assert all(np.isfinite(v).all() for v in g.grads.values() if v is not None)
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    dev = torch.device("cuda:0")
    t = lambda a: torch.tensor(a, device=dev)
    empty = torch.Tensor([])
    fwd = lambda d, depth: _C.rasterize_gaussians(t(sc.bg), t(sc.means3D), empty, t(sc.opacities), t(sc.scales), t(sc.rotations), 1.0, empty,
                                                  t(sc.viewmatrix), t(sc.projmatrix), t(sc.inv_viewprojmatrix), sc.tanfovx, sc.tanfovy,
                                                  sc.H, sc.W, t(sc.shs), 3, t(sc.campos), False, d, depth, False)
    def bwd(out, d):
        R, color, radii, geom, binning, img = out
        return _C.rasterize_gaussians_backward(t(sc.bg), t(sc.means3D), radii, t(sc.opacities), empty, t(sc.scales), t(sc.rotations), 1.0,
                                               empty, t(sc.viewmatrix), t(sc.projmatrix), t(sc.inv_viewprojmatrix), sc.tanfovx,
                                               sc.tanfovy, color, t(sc.dL_dout), t(sc.shs), 3, t(sc.campos), geom, R, binning, img, d, False)
    out = fwd(sd, True)                                          # depth forward: no log in the image buffer
    lied = bwd(out, {**sd, "_record_blend_log": True})           # (2)
    honest = bwd(fwd(sd, True), sd)
    for a, b in zip(lied, honest):
        if a is not None and a.numel():
            assert _rel(a.cpu().numpy(), b.cpu().numpy()) < 1e-5


LARGE = dict(P=300, W=640, H=480, sigma_min=10.0, sigma_max=200.0, seed=61, camera="orbit", opacity_range=(0.02, 0.3))


@pytest.mark.parametrize("sd", [settings_dict(**FULL_STP), settings_dict(3), settings_dict(0, order=2, rect=True, tbc=True), settings_dict(2, per_pixel=8, tbc=True)],
                         ids=["full_stp", "hier_min", "global_ptd_tbc", "kbuffer_tbc"])
def test_large_splats_take_the_wave_cooperative_tile_loops(sd):
    """Pixel sigmas up to 200: rectangles of hundreds to over a thousand tiles per Gaussian -- more than COOP_TILES = 64, so
    preprocess_kernel's tile-based-culling count and duplicate_kernel's key emission run wave-cooperatively (the counterpart
    of the reference's load balancing, stopthepop_common.cuh:207-259, 510-621).  Same bit-exact checks as everywhere."""
    sc = scenes.make_scene(**LARGE)
    g, f = check_against_oracle(sc, sd)
    assert int(g.geom_array("tiles_touched").view(np.uint32).max()) > 64          # the cooperative path is what ran
    assert np.array_equal(g.binning_array("keys_unsorted"), f.array("keys_unsorted"))       # emission order included
    assert np.array_equal(g.binning_array("point_list_unsorted"), f.array("values_unsorted"))


@pytest.mark.parametrize("name", ["c1_global", "dense_hier_full", "dense_kbuffer"])
def test_golden_fixtures(name):
    from golden.make_golden import CASES
    ref = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    case = CASES[name]
    g = GpuRun(scenes.make_scene(**case["scene"]), case["settings"], backward=True)
    assert g.num_rendered == int(ref["num_rendered"]) and np.array_equal(g.radii, ref["radii"])
    assert psnr(g.color, ref["color"]) >= 100.0
    for k in ("dL_dmeans3D", "dL_dopacity", "dL_dscales"):
        assert _rel(g.grads[k], ref[k]) < 1e-4


def test_tile_row_windows_paste_to_the_full_frame():
    """The sharding primitive on one GPU: disjoint tile-row windows reproduce the full frame bit for bit."""
    sc = scenes.make_scene(P=20000, W=320, H=240, sigma_min=1.0, sigma_max=10.0, seed=8, camera="orbit")
    sd = settings_dict(**FULL_STP)
    full = GpuRun(sc, sd, backward=False)
    img = np.zeros_like(full.color)
    for rows in ((0, 4), (4, 9), (9, 15)):
        part = GpuRun(sc, sd, backward=False, tile_rows=rows)
        assert np.array_equal(part.radii, full.radii)
        img[:, rows[0] * 16:rows[1] * 16] = part.color[:, rows[0] * 16:rows[1] * 16]
    assert np.array_equal(img, full.color)


def test_tile_row_window_holds_only_its_rows_of_the_image_state():
    """A forward restricted to a tile-row window (a rank of a tile-row shard) allocates the per-pixel arrays, the tile ranges and the blend
    log for ITS rows only (stp_buffers.hip: carve_image) -- a third of the rows, a third of the log -- and its arrays are the full frame's rows."""
    from diff_gaussian_rasterization import _C
    sc = scenes.make_scene(P=20000, W=320, H=240, sigma_min=1.0, sigma_max=10.0, seed=8, camera="orbit")
    sd = settings_dict(**FULL_STP)
    gx, rows = 20, (5, 10)
    full = GpuRun(sc, sd, backward=True)
    part = GpuRun(sc, sd, backward=True, tile_rows=rows)
    assert _C.blend_log_bytes(sc.W, sc.H, rows) * 3 == _C.blend_log_bytes(sc.W, sc.H)
    assert part.img.numel() < 0.36 * full.img.numel()
    arr = lambda name: _C.image_array(part.img, sc.W, sc.H, name, tile_rows=rows).cpu().numpy()
    fT = full.image_array("final_T").reshape(sc.H, sc.W)[rows[0] * 16:rows[1] * 16]
    assert np.array_equal(arr("final_T").reshape(-1, sc.W), fT)
    n_full = full.image_array("n_contrib").reshape(sc.H, sc.W)[rows[0] * 16:rows[1] * 16]
    assert np.array_equal(arr("n_contrib").reshape(-1, sc.W), n_full)
    r_full = full.image_array("ranges").view(np.uint32).reshape(-1, 2)[gx * rows[0]:gx * rows[1]]
    r_part = arr("ranges").view(np.uint32).reshape(-1, 2)
    assert r_part.shape == r_full.shape and np.array_equal(r_part[:, 1] - r_part[:, 0], r_full[:, 1] - r_full[:, 0])   # same lists, other offsets
    assert np.array_equal(part.color[:, rows[0] * 16:rows[1] * 16], full.color[:, rows[0] * 16:rows[1] * 16])
    empty = GpuRun(sc, sd, backward=True, tile_rows=(15, 15))   # a rank without rows: nothing rendered, nothing read out of bounds
    assert empty.num_rendered == 0 and all(v is None or not np.any(v) for v in empty.grads.values())


@pytest.mark.parametrize("name,scale,sd,backward", [
    ("C3", 0.01, settings_dict(2, per_pixel=16), True),
    ("C4", 0.01, settings_dict(**FULL_STP), False),
    ("C5", 0.004, settings_dict(**FULL_STP), True),
    ("C5", 0.004, settings_dict(3), True),
], ids=["C3_kbuffer16", "C4_fwd", "C5_full_stp", "C5_plain_hier"])
def test_baseline_configs_at_reduced_area(name, scale, sd, backward):
    """BASELINE configs C3 / C4 / C5 with Gaussian count and image area shrunk together (same entries per tile as the
    full-size frame: ~1100 for C3, ~1800 for C5: several windows of the replay), forward + backward
    against the oracle: image max-abs-diff and gradient max-abs-diff relative to the largest gradient."""
    sc = scenes.config(name, scale)
    g, f = check_against_oracle(sc, sd, backward=backward)
    lens = np.diff(g.image_array("ranges").view(np.uint32).reshape(-1, 2), axis=1)
    if name != "C4":
        assert lens.max() > 512  # the long-list path (window-by-window replay) is what runs here


@pytest.mark.parametrize("sd", [settings_dict(3), settings_dict(3, h44=True), settings_dict(**FULL_STP), settings_dict(3, per_pixel=8, tile_2x2=12),
                                settings_dict(2, per_pixel=16), settings_dict(0)], ids=["hier", "hier_cull", "full_stp", "hier_8_12", "kbuffer16", "global"])
def test_exact_depth_ties(sd):
    """Every Gaussian exists twice (same geometry, different colour and opacity): bit-identical depths along every ray, at
    every level.  The global sort keeps list order (stable), the tail's Batcher network does NOT (the reference's network
    is unstable: the HIP path redoes such a batch with the network itself), the mid level ranks by lane, the head's swap
    loop has its own rule -- all of it must come out as in the oracle."""
    import dataclasses
    base = scenes.make_scene(P=2500, W=80, H=64, sigma_min=2.0, sigma_max=12.0, seed=77, camera="orbit")
    tw = lambda a: None if a is None else np.concatenate([a, a], axis=0)
    sc = dataclasses.replace(base, means3D=tw(base.means3D), scales=tw(base.scales), rotations=tw(base.rotations),
                             opacities=np.concatenate([base.opacities, (0.7 * base.opacities).astype(np.float32)], axis=0),
                             shs=np.concatenate([base.shs, base.shs[::-1]], axis=0), colors_precomp=None)
    check_against_oracle(sc, sd)


@pytest.mark.parametrize("sd", [settings_dict(3), settings_dict(**FULL_STP)], ids=["hier", "full_stp"])
def test_wild_inverse_covariance_takes_the_checked_reciprocal(sd):
    """Depth keys are num * (1 / max(1e-5, v' Sigma^-1 v)) with the IEEE quotient (ref: stopthepop_common.cuh:44-55).  The
    render kernels take it as v_rcp + one Newton step, which is the correctly rounded quotient below 2^126; a frame whose
    Sigma^-1 entries all stay below 1e36 (every sane frame) runs kernels WITHOUT the domain check, anything else is
    reported by preprocess_kernel through the status word and runs the kernels with it.  Here: rotations of magnitude
    4e7..7.4e7 on scales of 1e-17 (which the inverse clamps at 1e-3) in a scene close to the camera -- Sigma^-1 entries of
    1e37..1.1e38, denominators in the two top binades, everything still finite, the covariance itself ordinary -- must
    give the oracle's frame bit for bit in its lists and to 2e-6 in its pixels."""
    sc = scenes.make_scene(P=600, W=112, H=80, sigma_min=1.5, sigma_max=8.0, seed=41, z_range=(0.3, 0.9))
    wild = np.arange(0, sc.P, 7)
    mag = np.linspace(4.0e7, 7.4e7, wild.size).astype(np.float32)
    # keep the visible covariance ordinary: Sigma = (S R)'(S R) grows with |q|^4, so the scales shrink by |q|^2
    sc.rotations[wild] *= mag[:, None]
    sc.scales[wild] /= (mag * mag)[:, None]
    g = GpuRun(sc, sd, backward=False)
    f, _ = oracle_run(sc, sd, backward=False)
    assert g.num_rendered == f.num_rendered and g.num_rendered > 0
    assert np.array_equal(g.radii, f.radii)
    vis = f.radii > 0
    inv = g.geom_array("cov3D_inv").reshape(sc.P, -1)[vis]
    assert np.isfinite(inv).all() and float(np.abs(inv).max()) > 8.5e37  # the scene is what it claims to be
    assert np.array_equal(g.binning_array("keys"), f.array("keys"))
    assert np.array_equal(g.binning_array("point_list"), f.array("point_list"))
    assert not np.isnan(g.color).any()
    assert max_abs(g.color, f.color) <= 2e-6


def test_tile_lists_longer_than_the_lds_sort_capacity():
    """A tile with more than 4096 entries: the tile-local depth sort takes its counting-pass route through the scratch
    arrays (stp_tilesort.hip); keys, list and everything downstream must still match the oracle bit for bit."""
    sc = scenes.make_scene(P=7000, W=24, H=20, sigma_min=6.0, sigma_max=20.0, seed=41, opacity_range=(0.02, 0.2))
    g, f = check_against_oracle(sc, settings_dict(3, h44=True))
    lens = np.diff(g.image_array("ranges").view(np.uint32).reshape(-1, 2), axis=1)
    assert lens.max() > 4096, lens.ravel()


def test_tile_order_changes_no_pixel():
    """STP_TILE_ORDER (read once per process, so this runs in children): the render kernels' workgroups take the tiles longest list first by default, in
    the XCD-contiguous spatial order of rounds 1-5 with STP_TILE_ORDER=0 -- a schedule, not a result: image, keys and list are the same bit for bit,
    gradients to the summation order of the atomics.  The scene is lumpy (clusters), so the two orders really differ."""
    import os, subprocess, sys, tempfile
    code = ("import sys, numpy as np; sys.path[:0] = ['tests', 'stopthepop-rasterization_amd', '.']; import conftest;"
            "from helpers import *; from diff_gaussian_rasterization import scenes;"
            "sc = scenes.make_scene(P=30000, W=640, H=480, sigma_min=1.0, sigma_max=8.0, seed=77, clusters=(5, 0.6, 0.03));"   # (1200 tiles: windows of up to 1024 are not ordered)
            "out = {};"
            "[out.update({m: GpuRun(sc, sd, backward=True)}) for m, sd in (('hier', settings_dict(**FULL_STP)), ('kb', settings_dict(2, per_pixel=16)))];"
            "np.savez(sys.argv[1], **{m + '_' + k: v for m, g in out.items() for k, v in (('color', g.color), ('keys', g.binning_array('keys')), ('list', g.binning_array('point_list')),"
            " ('g_means', g.grads['dL_dmeans3D']), ('g_sh', g.grads['dL_dsh']), ('g_op', g.grads['dL_dopacity']))})")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        res = {}
        for mode in ("1", "0"):
            f = os.path.join(d, f"o{mode}.npz")
            subprocess.run([sys.executable, "-c", code, f], check=True, env=dict(os.environ, STP_TILE_ORDER=mode), cwd=root)
            res[mode] = dict(np.load(f))
    for k, a in res["1"].items():
        b = res["0"][k]
        if k.endswith(("color", "keys", "list")):
            assert np.array_equal(a, b), k
        else:
            assert _rel(a, b) < 2e-5, (k, _rel(a, b))


@pytest.mark.parametrize("scene_kw", [
    "P=3000, W=96, H=80, sigma_min=2.0, sigma_max=12.0, seed=11, camera='orbit'",
    "P=7000, W=24, H=20, sigma_min=6.0, sigma_max=20.0, seed=41, opacity_range=(0.02, 0.2)"], ids=["dense", "lists_over_4096"])
def test_reference_style_full_radix_sort_still_selectable(monkeypatch, scene_kw):
    """STP_SORT (read once per process, so this runs in children): the reference's single full-width radix sort +
    separate entry gather ("radix"), the default (radix sort on the tile bits + per-tile sort) and binning by tile
    counters + per-tile sort ("counters") give the same sorted list and the same frame."""
    import subprocess, sys
    code = ("import sys, numpy as np; sys.path[:0] = ['tests', 'stopthepop-rasterization_amd', '.']; import conftest;"
            "from helpers import *; from diff_gaussian_rasterization import scenes;"
            f"sc = scenes.make_scene({scene_kw});"
            "g = GpuRun(sc, settings_dict(3, h44=True)); np.save(sys.argv[1], g.color); np.save(sys.argv[2], g.binning_array('keys'));"
            "np.save(sys.argv[2] + '.list.npy', g.binning_array('point_list'))")
    import os, tempfile
    with tempfile.TemporaryDirectory() as d:
        outs = {}
        for mode in ("radix", "default", "counters"):
            env = dict(os.environ, STP_SORT=mode)
            a, b = os.path.join(d, mode + "_c.npy"), os.path.join(d, mode + "_k.npy")
            subprocess.run([sys.executable, "-c", code, a, b], check=True, env=env, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
            outs[mode] = (np.load(a), np.load(b), np.load(b + ".list.npy"))
    for mode in ("default", "counters"):
        for part in (1, 2, 0):  # sorted keys, sorted id list, frame
            assert np.array_equal(outs["radix"][part], outs[mode][part]), (mode, part)


def test_scan_and_colour_stream_switches_change_nothing():
    """STP_SCAN=rocprim (device-wide scan of the tile counts instead of the two-level scan inside preprocess / duplicate) and
    STP_COLOUR_LATE=0 (the colour kernel beside duplicate_kernel instead of behind it) are schedules, not results: point_offsets,
    the unsorted and sorted keys, the sorted list and the frame are the default's bit for bit.  (Read once per process: children.)"""
    import os, subprocess, sys, tempfile
    code = ("import sys, numpy as np; sys.path[:0] = ['tests', 'stopthepop-rasterization_amd', '.']; import conftest;"
            "from helpers import *; from diff_gaussian_rasterization import scenes;"
            "sc = scenes.make_scene(P=5000, W=200, H=120, sigma_min=1.0, sigma_max=30.0, seed=23, camera='orbit');"
            "g = GpuRun(sc, settings_dict(3, order=3, rect=True, tight=True, tbc=True, h44=True, lb=True));"
            "np.savez(sys.argv[1], color=g.color, offsets=g.geom_array('point_offsets'), ku=g.binning_array('keys_unsorted'),"
            " k=g.binning_array('keys'), l=g.binning_array('point_list'), n=np.int64(g.num_rendered))")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        outs = {}
        for name, extra in (("default", {}), ("rocprim", {"STP_SCAN": "rocprim"}), ("early", {"STP_COLOUR_LATE": "0"})):
            f = os.path.join(d, name + ".npz")
            subprocess.run([sys.executable, "-c", code, f], check=True, env=dict(os.environ, **extra), cwd=root)
            outs[name] = dict(np.load(f))
    for name in ("rocprim", "early"):
        for part in ("n", "offsets", "ku", "k", "l", "color"):
            assert np.array_equal(outs["default"][part], outs[name][part]), (name, part)


@pytest.mark.parametrize("scene_kw", [
    "P=5000, W=200, H=120, sigma_min=1.0, sigma_max=30.0, seed=23, camera='orbit'",
    "P=40000, W=1280, H=720, sigma_min=1.0, sigma_max=12.0, seed=3, camera='orbit'",
    "P=300, W=64, H=48, sigma_min=1.0, sigma_max=6.0, seed=4"], ids=["8bit_digits", "13_tile_bits", "tiny"])
def test_tile_bit_sort_under_our_own_onesweep_driver(scene_kw):
    """The tile-bit sort runs rocPRIM's onesweep kernels under our own driver (stp_binning.hip: every pass with its own look-back states
    and block counter, all cleared once by duplicate_kernel's trailing workgroups -- instead of the library's five fill launches per
    sort).  STP_TILE_SORT=own forces it for every size, =rocprim is the library call: same sorted keys, list and frame, also in a
    run-ahead forward (GpuRun renders both ways), for one, two and (tiles < 256) a single digit place."""
    import os, subprocess, sys, tempfile
    code = ("import sys, numpy as np; sys.path[:0] = ['tests', 'stopthepop-rasterization_amd', '.']; import conftest;"
            "from helpers import *; from diff_gaussian_rasterization import scenes;"
            f"sc = scenes.make_scene({scene_kw});"
            "g = GpuRun(sc, settings_dict(3, order=3, rect=True, tight=True, tbc=True, h44=True, lb=True));"
            "np.savez(sys.argv[1], color=g.color, k=g.binning_array('keys'), l=g.binning_array('point_list'), n=np.int64(g.num_rendered),"
            " r=g.image_array('ranges'), dm=g.grads['dL_dmeans3D'])")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        outs = {}
        for name in ("own", "rocprim"):
            f = os.path.join(d, name + ".npz")
            subprocess.run([sys.executable, "-c", code, f], check=True, env=dict(os.environ, STP_TILE_SORT=name), cwd=root)
            outs[name] = dict(np.load(f))
    assert int(outs["own"]["n"]) > 0
    for part in ("n", "k", "l", "r", "color"):
        assert np.array_equal(outs["own"][part], outs["rocprim"][part]), part
    assert _rel(outs["own"]["dm"], outs["rocprim"]["dm"]) < 1e-5


def test_second_backward_after_buffer_recycling_fails_loudly():
    """retain_graph + a later forward that reuses the pooled scratch buffers: the second backward must raise instead
    of replaying somebody else's tile lists."""
    import torch
    sc = scenes.config("C2", 0.4)  # big enough for the pooled (>= 256 MiB) buffer class: 0.4 x 2.09 M tile-grid pixels x 418 B of log
    g = GpuRun(sc, settings_dict(**FULL_STP), backward=False)
    t = lambda a: torch.tensor(a, device="cuda:0")
    import diff_gaussian_rasterization as dgr
    rast = dgr.GaussianRasterizer(g.rs)
    m3 = t(sc.means3D).requires_grad_(True)
    args = dict(shs=t(sc.shs), scales=t(sc.scales), rotations=t(sc.rotations))
    color, _ = rast(m3, torch.zeros_like(m3), t(sc.opacities), **args)
    color.sum().backward(retain_graph=True)                       # returns the buffers to the free list
    color2, _ = rast(m3, torch.zeros_like(m3), t(sc.opacities), **args)   # ... and this forward takes them
    with pytest.raises(RuntimeError, match="recycled"):
        color.sum().backward()
    color2.sum().backward()                                       # the newer graph is fine


def test_stage_timers_and_viewer_text():
    """stp_timing_* (the reference's Timer, rasterizer_impl.h:77-147): means per stage over the calls since enabling,
    and the text the viewer shows."""
    from diff_gaussian_rasterization import _C
    sc = scenes.make_scene(**C1)
    _C.timing_enable(True)
    for _ in range(3):
        GpuRun(sc, settings_dict(**FULL_STP), backward=True)
    ms = _C.timing_read()
    text = _C.timing_text()
    _C.timing_enable(False)
    assert all(ms[k] > 0 for k in ("Preprocess", "Duplicate", "Sort", "Render", "BwdRender", "BwdPreprocess")), ms
    lines = text.splitlines()
    assert lines[0] == "Timings: " and len(lines) == 8
    total = float(lines[5].split(":")[1].rstrip("ms"))
    assert abs(total - sum(ms[k] for k in ("Preprocess", "Duplicate", "Sort", "Render"))) < 1e-3 * max(total, 1.0)


# ---------------------------------------------------------------- BASELINE-size property tests
@pytest.fixture(scope="module")
def c2_scene():
    return scenes.config("C2")


def test_c2_full_size_properties(c2_scene):
    """Full 1M-Gaussian 1080p frame (the oracle would take minutes): size-independent properties."""
    sd = settings_dict(**FULL_STP)
    g = GpuRun(c2_scene, sd, backward=True)
    R = g.num_rendered
    tiles = g.geom_array("tiles_touched").view(np.uint32)
    assert int(tiles.astype(np.int64).sum()) == R                       # checksum of the duplicate count
    assert np.array_equal(np.cumsum(tiles.astype(np.int64)).astype(np.uint32), g.geom_array("point_offsets").view(np.uint32))
    keys = g.binning_array("keys")
    T = ((c2_scene.W + 15) // 16) * ((c2_scene.H + 15) // 16)
    bit = int(np.ceil(np.log2(T + 1)))
    masked = keys & np.uint64((1 << (32 + bit)) - 1)
    assert np.all(masked[1:] >= masked[:-1])                            # sortedness on the sorted bit range
    ids = g.binning_array("point_list")
    vis_ids = np.nonzero(tiles)[0]
    assert np.array_equal(np.bincount(ids[ids != 0xFFFFFFFF].astype(np.int64), minlength=c2_scene.P)[vis_ids], tiles[vis_ids])  # every Gaussian appears tiles_touched times
    ranges = g.image_array("ranges").view(np.uint32).reshape(-1, 2)
    valid_tiles = (keys >> np.uint64(32)) < T
    assert int((ranges[:, 1] - ranges[:, 0]).astype(np.int64).sum()) == int(valid_tiles.sum())  # ranges tile the valid part
    fT = g.image_array("final_T")
    assert np.all(fT >= 0) and np.all(fT <= 1) and np.isfinite(g.color).all()
    assert all(np.isfinite(v).all() for v in g.grads.values() if v is not None)
    # determinism of the forward, and linearity of the backward in dL/dimage
    g2 = GpuRun(c2_scene, sd, backward=False)
    assert np.array_equal(g.color, g2.color)
    scaled = scenes.config("C2")
    scaled.dL_dout = scaled.dL_dout * np.float32(2.0)
    g3 = GpuRun(scaled, sd, backward=True)
    assert _rel(g3.grads["dL_dmeans3D"], 2.0 * g.grads["dL_dmeans3D"]) < 1e-4
    assert _rel(g3.grads["dL_dsh"], 2.0 * g.grads["dL_dsh"]) < 1e-4


def test_c2_tile_rows_against_oracle(c2_scene):
    """A window of tile rows of the FULL C2 frame (1M Gaussians preprocessed, ~6% of the tiles blended), in both C2
    variants, against the oracle on the same window: image, radii and the render-half gradients."""
    for sd in (settings_dict(**FULL_STP), settings_dict(3)):
        rows = (32, 36)
        g = GpuRun(c2_scene, sd, backward=True, tile_rows=rows)
        f, og = oracle_run(c2_scene, sd, backward=True, tile_rows=rows)
        assert g.num_rendered == f.num_rendered and np.array_equal(g.radii, f.radii)
        sl = slice(rows[0] * 16, rows[1] * 16)
        assert psnr(g.color[:, sl], f.color[:, sl]) >= 100.0 and max_abs(g.color[:, sl], f.color[:, sl]) <= 2e-6
        for k in ("dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dsh"):
            assert _rel(g.grads[k], og[k]) < 1e-4, k
        assert _rel(g.grads["dL_dmeans2D"][:, :2], og["dL_dmeans2D"][:, :2]) < 1e-4


def test_c2_whole_frame_is_the_oracle_with_its_threshold_decisions_forced(c2_scene):
    """The headline frame, WHOLE (1M Gaussians, 1080p, full StopThePop settings, forward + backward; the oracle on the GPU box's 128 cores takes seconds): sort
    keys and lists bit-equal; the pixels that move by more than 2e-6 -- two of 2 073 600 on the synthetic scene -- each have an alpha within 6e-7 of 1/255
    (oracle/explain.py), and the oracle re-run with exactly those alpha tests taken the other way (oracle.forced_alpha_flips) agrees with the product on EVERY
    pixel to 2e-6 and on every gradient tensor to 1e-4: nothing but those decisions separates the two."""
    sd = settings_dict(**FULL_STP)
    g = GpuRun(c2_scene, sd, backward=True)
    f, og = oracle_run(c2_scene, sd, backward=True)
    assert g.num_rendered == f.num_rendered and np.array_equal(g.radii, f.radii)
    assert np.array_equal(g.binning_array("keys"), f.array("keys")) and np.array_equal(g.binning_array("point_list"), f.array("point_list"))
    d = np.abs(g.color.astype(np.float64) - f.color.astype(np.float64))
    assert d.max() <= 1.0 / 255.0 + 1e-6
    moved = (d > 2e-6).any(axis=0)
    if moved.any():
        from oracle import explain
        ex = explain.explain_moved_pixels(moved, W=c2_scene.W, H=c2_scene.H, ranges=f.array("ranges").reshape(-1), point_list=f.array("point_list"),
                                          conic_opacity=f.array("conic_opacity").reshape(-1), means2D=f.array("means2D").reshape(-1),
                                          final_T_a=g.image_array("final_T").reshape(-1), final_T_b=f.array("final_T").reshape(-1), cull_4x4=True)
        assert int(moved.sum()) <= 8 and not ex["unexplained"], (int(moved.sum()), ex["by"], ex["unexplained"][:5])
        assert _matches_a_nudged_oracle(c2_scene, sd, g, True, 2e-6, 1e-4, ex, max_tries=3), ex["by"]
    else:
        for k in GRAD_KEYS:
            if g.grads.get(k) is None or og.get(k) is None:
                continue
            a, b = g.grads[k], og[k]
            if k == "dL_dmeans2D":
                a, b = a[:, :2], b[:, :2]
            assert _rel(a, b) < 1e-4, k


# ---------------------------------------------------------------- the run-ahead forward (stp_forward.hip, round 4)
def _layout_count(g):
    import ctypes
    from diff_gaussian_rasterization import _C
    return int(_C._load().stp_binning_layout_count(ctypes.c_void_p(g.binning.data_ptr()), int(g.num_rendered)))


@pytest.mark.parametrize("sd", [settings_dict(0), settings_dict(2, per_pixel=16), settings_dict(**FULL_STP)], ids=["global", "kbuffer16", "full_stp"])
def test_run_ahead_forward_launches_on_a_capacity(sd):
    """Every GpuRun renders its frame twice (helpers.py): first the default path, then -- what the tests inspect -- the run-ahead path.  Here
    the claim itself: the second forward carved its binning buffer for the guessed capacity (count + 12.5 % + 1024), padded the slots
    behind num_rendered, and everything the oracle can see is unchanged -- unsorted emission order included."""
    sc = scenes.make_scene(**DENSE)
    g, f = check_against_oracle(sc, sd)
    R = g.num_rendered
    assert _layout_count(g) == R + R // 8 + 1024
    assert np.array_equal(g.binning_array("keys_unsorted"), f.array("keys_unsorted"))
    assert np.array_equal(g.binning_array("point_list_unsorted"), f.array("values_unsorted"))
    cold = GpuRun(sc, sd, backward=True, warm=False, run_ahead=True)      # a third forward: still run-ahead, same results
    assert _layout_count(cold) == R + R // 8 + 1024
    assert np.array_equal(cold.color, g.color)
    exact = GpuRun(sc, sd, backward=True, warm=False, run_ahead=False)    # the default: the reference's order of events, exact layout
    assert _layout_count(exact) == R
    assert np.array_equal(exact.color, g.color) and np.array_equal(exact.binning_array("keys"), g.binning_array("keys"))
    from diff_gaussian_rasterization import _C
    _C.reset_size_guesses()
    first = GpuRun(sc, sd, backward=True, warm=False, run_ahead=True)     # switched on, but no guess yet: exact
    assert _layout_count(first) == R and np.array_equal(first.color, g.color)
    for other in (cold, exact):   # (gradient sums leave the chip through float atomics: equal up to their order)
        for k in g.grads:
            if g.grads[k] is not None:
                assert _rel(other.grads[k], g.grads[k]) < 1e-5, k


@pytest.mark.parametrize("sd", [settings_dict(3, h44=True), settings_dict(2, per_pixel=16), settings_dict(0, order=3)], ids=["hier_cull", "kbuffer16", "global_ptd_max"])
def test_run_ahead_overflow_is_redone(sd):
    """A frame with far more tile-list entries than the frame before it of the same kind (same P, resolution and settings; splats four times
    the size): the run-ahead launch overflows its guessed capacity -- duplicate_kernel writes nothing out of bounds -- and the host, which
    learns the true count after its last launch, redoes the frame from duplicate_kernel on with the exact size before the call returns."""
    from diff_gaussian_rasterization import _C
    small = scenes.make_scene(P=4000, W=96, H=80, sigma_min=1.0, sigma_max=3.0, seed=5, camera="orbit")
    big = scenes.make_scene(P=4000, W=96, H=80, sigma_min=4.0, sigma_max=14.0, seed=5, camera="orbit")
    _C.reset_size_guesses()
    a = GpuRun(small, sd, backward=False, warm=False, run_ahead=True)
    f_big, og = oracle_run(big, sd, backward=True)
    assert f_big.num_rendered > 2 * a.num_rendered + 4096      # the guess cannot hold it
    b = GpuRun(big, sd, backward=True, warm=False, run_ahead=True)
    assert b.num_rendered == f_big.num_rendered and _layout_count(b) == b.num_rendered   # redone with the exact size
    assert np.array_equal(b.radii, f_big.radii)
    assert np.array_equal(b.binning_array("keys"), f_big.array("keys")) and np.array_equal(b.binning_array("point_list"), f_big.array("point_list"))
    assert np.array_equal(b.image_array("ranges").view(np.uint32), f_big.array("ranges"))
    assert max_abs(b.color, f_big.color) <= 2e-6
    for k in ("dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dsh"):
        assert _rel(b.grads[k], og[k]) < 1e-4, k
    c = GpuRun(big, sd, backward=True, warm=False, run_ahead=True)   # the next frame of the kind fits again
    assert _layout_count(c) > c.num_rendered and np.array_equal(c.color, b.color)
    d = GpuRun(small, sd, backward=False, warm=False, run_ahead=True)   # and a small frame behind a big one is padded, not redone
    assert _layout_count(d) > 2 * d.num_rendered and np.array_equal(d.color, a.color)


def test_gradient_record_buffer_is_kept_clean_between_backwards():
    """The (P, 16) gradient-record buffer of a whole backward is kept by the binding and NOT zero-filled again: the per-Gaussian half clears
    every record it reads (stp_backward_phases, phases bit 3).  Different scenes of one size back to back -- other visible sets, other modes --
    must each get their own gradients, not the previous frame's leftovers."""
    scs = [scenes.make_scene(P=4000, W=96, H=80, sigma_min=2.0, sigma_max=12.0, seed=s, camera="orbit") for s in (31, 32)]
    scs[1].means3D[::3, 2] = -5.0    # a third of the second scene's Gaussians behind the camera: invisible there, visible in the first
    for sc, sd in ((scs[0], settings_dict(**FULL_STP)), (scs[1], settings_dict(2, per_pixel=8)), (scs[0], settings_dict(0)), (scs[1], settings_dict(3))):
        g = GpuRun(sc, sd, backward=True, warm=False)
        f, og = oracle_run(sc, sd, backward=True)
        for k in ("dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dsh", "dL_dmeans2D"):
            a, b = g.grads[k], og[k]
            if k == "dL_dmeans2D":
                a, b = a[:, :2], b[:, :2]
            assert _rel(a, b) < 1e-4, k
        invisible = f.radii == 0
        assert invisible.any() or sc is scs[0]
        assert not np.any(g.grads["dL_dmeans3D"][invisible]) and not np.any(g.grads["dL_dsh"][invisible])


def test_blend_log_depth_follows_the_scene():
    """The blend log's depth is chosen per frame (stp_forward.hip: log_depth_for): a frame nothing is known about gets 192 records per pixel,
    every recording forward reports the largest blend count of its pixels, and the frames of the same kind after it size their log by it
    -- smaller for a scene that blends a few dozen entries per pixel, deeper (up to 512) for one that overflowed."""
    from diff_gaussian_rasterization import _C
    sd = settings_dict(**FULL_STP)
    sc = scenes.make_scene(**DENSE)
    _C.reset_size_guesses()
    runs = [GpuRun(sc, sd, backward=True, warm=False) for _ in range(3)]
    need = int(runs[0].image_array("n_contrib").view(np.uint32).max())
    assert 8 < need < 165
    assert _C.blend_log_depth(runs[0].img) == 192 and _C.blend_log_depth(runs[1].img) == 192    # (the second frame is sized before the first one's report arrives)
    want = min(512, max(32, (need + need // 8 + 4 + 15) // 16 * 16))
    assert _C.blend_log_depth(runs[2].img) == want and want < 192 and runs[2].img.numel() < runs[0].img.numel()
    assert not runs[2].image_array("tile_flags").any()
    for r in runs[1:]:
        assert np.array_equal(r.color, runs[0].color)
        for k in GRAD_KEYS:
            if runs[0].grads.get(k) is not None:
                assert _rel(r.grads[k], runs[0].grads[k]) < 1e-5, k
    # a scene whose pixels blend more than 192 entries: flagged tiles (re-sorting backward) at first, a deeper log afterwards
    hz = scenes.make_scene(P=4000, W=48, H=48, sigma_min=8.0, sigma_max=20.0, seed=9, opacity_range=(0.004, 0.012))
    _C.reset_size_guesses()
    h = [GpuRun(hz, sd, backward=True, warm=False) for _ in range(3)]
    need_h = int(h[0].image_array("n_contrib").view(np.uint32).max())
    assert 192 < need_h, need_h
    assert h[0].image_array("tile_flags").any() and _C.blend_log_depth(h[0].img) == 192
    assert _C.blend_log_depth(h[2].img) == min(512, (need_h + need_h // 8 + 4 + 15) // 16 * 16)
    if need_h <= _C.blend_log_depth(h[2].img):
        assert not h[2].image_array("tile_flags").any()
    for k in GRAD_KEYS:
        if h[0].grads.get(k) is not None:
            assert _rel(h[2].grads[k], h[0].grads[k]) < 2e-5, k     # replayed == re-sorted


def _direct_forward(sc, sd, dev="cuda:0"):
    """One forward through _C directly (no autograd): the tensors and the six outputs of rasterize_gaussians."""
    from diff_gaussian_rasterization import _C
    t = lambda a: torch.tensor(a, device=dev)
    empty = torch.Tensor([])
    ten = dict(bg=t(sc.bg), means3D=t(sc.means3D), opac=t(sc.opacities), scales=t(sc.scales), rots=t(sc.rotations), shs=t(sc.shs),
               view=t(sc.viewmatrix), proj=t(sc.projmatrix), inv=t(sc.inv_viewprojmatrix), cam=t(sc.campos), w=t(sc.dL_dout))
    out = _C.rasterize_gaussians(ten["bg"], ten["means3D"], empty, ten["opac"], ten["scales"], ten["rots"], sc.scale_modifier, empty, ten["view"],
                                 ten["proj"], ten["inv"], sc.tanfovx, sc.tanfovy, sc.H, sc.W, ten["shs"], sc.sh_degree, ten["cam"], False, sd, False, False)
    return ten, out


def _direct_backward(sc, sd, ten, out, geom, binning, img):
    from diff_gaussian_rasterization import _C
    empty = torch.Tensor([])
    R, color, radii = out[0], out[1], out[2]
    return _C.rasterize_gaussians_backward(ten["bg"], ten["means3D"], radii, ten["opac"], empty, ten["scales"], ten["rots"], sc.scale_modifier, empty,
                                           ten["view"], ten["proj"], ten["inv"], sc.tanfovx, sc.tanfovy, color, ten["w"], ten["shs"], sc.sh_degree,
                                           ten["cam"], geom, R, binning, img, sd, False)


@pytest.mark.parametrize("sd", [settings_dict(**FULL_STP), settings_dict(2, per_pixel=16), settings_dict(0)], ids=["full_stp", "kbuffer16", "global"])
def test_scratch_buffers_describe_themselves(sd):
    """The reference hands (buffer, num_rendered) to its backward as self-contained blobs.  Ours carry what they were carved with -- the binning
    buffer's capacity (a run-ahead forward carves for a guess, not for num_rendered), the blend log's depth (chosen per frame) -- in a header
    of their own: a CLONE of the buffers, which no cache of the library knows, gives the same gradients as the originals; a buffer whose
    header is gone is refused instead of being carved on a guess.  (Round 6: the clones of this test DID land on addresses the library's cache
    still knew from forwards whose buffers had been freed -- the binding now checks which storage a tensor is before the library may trust the address.)"""
    from diff_gaussian_rasterization import _C
    sc = scenes.make_scene(**DENSE)
    sd = {**sd, "_record_blend_log": True, "_backward_mode": "replay"}
    _C.reset_size_guesses()
    before = _C.set_run_ahead(1)
    try:
        _, o0 = _direct_forward(sc, sd)                       # the first forward of the kind: exact size, default depth
        _C.release_scratch(o0[5]); _C.release_scratch(o0[4])
        for _ in range(2):                                    # the third: run-ahead capacity, depth by the scene
            ten, out = _direct_forward(sc, sd)
        R, geom, binning, img = out[0], out[3], out[4], out[5]
        cap = _C.binning_array(binning, R, "keys").numel()   # (view of the first R entries)
        assert cap == R
        assert int(_C._load().stp_binning_layout_count(binning.data_ptr(), R)) == R + R // 8 + 1024
        ref = _direct_backward(sc, sd, ten, out, geom, binning, img)
        geom2, binning2, img2 = geom.clone(), binning.clone(), img.clone()
        # (the binding tells the library to forget an address whose tensor is not the storage a forward of this process returned there -- a clone
        # may well land on the address of a buffer that was freed a moment ago and whose cache entry carries the same num_rendered)
        _C._native().forget_unless_same_storage(binning2)
        assert int(_C._load().stp_binning_layout_count(binning2.data_ptr(), R)) == R + R // 8 + 1024   # read from the clone's own header
        if sd["sort_settings"]["sort_mode"] in (2, 3):
            assert _C.blend_log_depth(img2) == _C.blend_log_depth(img) > 0
        else:
            assert _C.blend_log_depth(img2) == 0
        got = _direct_backward(sc, sd, ten, out, geom2, binning2, img2)
        for a, b in zip(got, ref):
            if a is not None and b is not None and b.numel():
                assert _rel(a.cpu().numpy(), b.cpu().numpy()) < 1e-5
        # an address whose cached layout belongs to a PREVIOUS tenant with the same num_rendered: the exact-size buffer of the
        # first forward copied over the run-ahead one.  stp_forget_buffer -- what the binding's pool calls when it releases a buffer -- sends
        # the lookup to the header the copy brought along
        _C.reset_size_guesses()
        _, o1 = _direct_forward(sc, sd)                       # first of its kind again: exact size
        assert o1[0] == R and int(_C._load().stp_binning_layout_count(o1[4].data_ptr(), R)) == R
        n1 = int(_C._load().stp_binning_buffer_size(R))
        binning[:n1].copy_(o1[4][:n1])
        assert int(_C._load().stp_binning_layout_count(binning.data_ptr(), R)) == R + R // 8 + 1024      # the stale entry
        _C._load().stp_forget_buffer(binning.data_ptr())
        assert int(_C._load().stp_binning_layout_count(binning.data_ptr(), R)) == R                      # the header
        got = _direct_backward(sc, sd, ten, out, geom, binning, img)
        for a, b in zip(got, ref):
            if a is not None and b is not None and b.numel():
                assert _rel(a.cpu().numpy(), b.cpu().numpy()) < 1e-5
        _C.release_scratch(o1[5]); _C.release_scratch(o1[4])
        # no header, no backward
        img3 = img.clone(); img3[:16] = 0
        if sd["sort_settings"]["sort_mode"] in (2, 3):
            with pytest.raises(RuntimeError, match="header"):
                _direct_backward(sc, sd, ten, out, geom2, binning2, img3)
        bin3 = binning.clone(); bin3[:16] = 0
        with pytest.raises(RuntimeError, match="header"):
            _direct_backward(sc, sd, ten, out, geom2, bin3, img2)
    finally:
        _C.set_run_ahead(before)


def test_forward_split_renders_the_same_frame_and_fires_its_event_between_the_launches():
    """stp_set_forward_split (tile-row sharding, round 6): the render kernel in two launches with the caller's event between them -- same pixels,
    same scratch state, same gradients; the request is consumed by ONE forward."""
    import torch
    from diff_gaussian_rasterization import _C
    sc = scenes.make_scene(**DENSE)
    for sd in (settings_dict(**FULL_STP), settings_dict(2, per_pixel=8), settings_dict(0)):
        sd = {**sd, "_record_blend_log": sd["sort_settings"]["sort_mode"] in (2, 3), "_backward_mode": "replay"}
        ten, ref = _direct_forward(sc, sd)
        gref = _direct_backward(sc, sd, ten, ref, ref[3], ref[4], ref[5])
        ev = torch.cuda.Event(); ev.record()
        _C.set_forward_split(((sc.H + 15) // 16) // 2, ev)
        ten2, out = _direct_forward(sc, sd)
        ev.synchronize()
        assert out[0] == ref[0] and torch.equal(out[1], ref[1]) and torch.equal(out[2], ref[2])
        got = _direct_backward(sc, sd, ten2, out, out[3], out[4], out[5])
        for a, b in zip(got, gref):
            if a is not None and b is not None and b.numel():
                assert _rel(a.cpu().numpy(), b.cpu().numpy()) < 1e-5
        _, again = _direct_forward(sc, sd)            # no request pending any more: one launch, same frame
        assert torch.equal(again[1], ref[1])
        for o in (ref, out, again):
            _C.release_scratch(o[5]); _C.release_scratch(o[4])


def test_stage_timer_keeps_per_call_times():
    """stp_timing_history: the six stage times of every call since timing_enable(True), in order -- what lets bench.py say WHICH step of a timed
    region was slow and in which stage."""
    from diff_gaussian_rasterization import _C
    sc = scenes.make_scene(**C1)
    _C.timing_enable(True)
    for _ in range(5):
        GpuRun(sc, settings_dict(**FULL_STP), backward=True, warm=False)
    mean = _C.timing_read()
    hist = _C.timing_history()
    _C.timing_enable(False)
    assert len(hist) == 5
    for k in ("Preprocess", "Duplicate", "Sort", "Render", "BwdRender", "BwdPreprocess"):
        assert all(h[k] > 0 for h in hist), (k, hist)
        assert abs(sum(h[k] for h in hist) / 5 - mean[k]) < 1e-3 * max(mean[k], 1.0)


def test_per_gaussian_half_by_id_range():
    """stp_backward_phases, phases bits 8-23: the per-Gaussian half of the backward on chunk k of K id ranges -- what lets a tile-row shard run it
    on the records that have already been all-reduced while the rest is still on the links (tile_shard.py).  Gaussians are independent in that
    half: K chunks into shared output tensors are bit-identical to one launch, whatever K."""
    from diff_gaussian_rasterization import _C, tile_shard
    sc = scenes.make_scene(**DENSE)
    sd = {**settings_dict(**FULL_STP), "_record_blend_log": True, "_backward_mode": "replay"}
    ten, out = _direct_forward(sc, sd)
    empty = torch.Tensor([])
    args = (ten["bg"], ten["means3D"], out[2], ten["opac"], empty, ten["scales"], ten["rots"], sc.scale_modifier, empty, ten["view"], ten["proj"], ten["inv"],
            sc.tanfovx, sc.tanfovy, out[1], ten["w"], ten["shs"], sc.sh_degree, ten["cam"], out[3], out[0], out[4], out[5], sd, False)
    records = _C.rasterize_gaussians_backward(*args, phases=1 | 4)
    assert records.shape == (sc.P, 9)
    whole = _C.rasterize_gaussians_backward(*args, phases=2 | 4, partial=records.clone())
    for K in (2, 3, 7):
        b = tile_shard.record_chunk_bounds(sc.P, K)
        assert b[0] == 0 and b[-1] == sc.P and all(x % 256 == 0 for x in b[:-1]) and sorted(b) == b
        got = None
        for k in range(K):
            piece = torch.zeros_like(records)            # only piece k has "arrived": the other rows are not read by chunk k
            piece[b[k]:b[k + 1]] = records[b[k]:b[k + 1]]
            got = _C.rasterize_gaussians_backward(*args, phases=2 | 4, partial=piece, chunk=(k, K), outputs=got)
        for a, w in zip(got, whole):
            assert torch.equal(a, w)
    with pytest.raises(RuntimeError):
        _C.rasterize_gaussians_backward(*args, phases=2 | 4 | (2 << 8) | (5 << 16), partial=records)   # chunk 5 of 2


@pytest.mark.parametrize("sd", [settings_dict(**FULL_STP), settings_dict(3), settings_dict(2, per_pixel=2), settings_dict(2, per_pixel=16)],
                         ids=["full_stp", "hier", "kbuffer2", "kbuffer16"])
def test_frame_without_any_entry_is_background_whatever_the_memory_holds(sd):
    """The per-pixel-sort forwards let pads and stand-ins read "entry 0 of the tile's list" and weigh it with zero.  In a frame without ANY
    tile-list entry behind a run-ahead launch (num_rendered == 0, capacity > 0) the entry records are never written: with NaN in that memory
    0 x NaN reached the image (found by tools/fuzz_parity.py in round 5: tile-row windows over empty rows).  Empty tiles are background by an
    early exit now; here the allocator's free memory is poisoned with NaN first."""
    sc = scenes.make_scene(P=300, W=100, H=70, sigma_min=2.0, sigma_max=6.0, seed=3)
    sc.means3D[:, 2] = -5.0                  # every Gaussian behind the camera: no tile-list entry in the whole frame
    for rows in (None, (1, 3)):
        for _ in range(2):
            poison = torch.full((48 << 20,), float("nan"), device="cuda:0")
            del poison                       # (back to the caching allocator: the next buffers are cut from it)
            g = GpuRun(sc, sd, backward=False, tile_rows=rows)   # exact pass, then the run-ahead pass (helpers.py)
            assert g.num_rendered == 0
            win = g.color if rows is None else g.color[:, 16 * rows[0]:min(16 * rows[1], sc.H)]
            assert not np.isnan(g.color).any()
            assert np.array_equal(win, np.broadcast_to(np.asarray(sc.bg, np.float32)[:, None, None], win.shape))
