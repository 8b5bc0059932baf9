"""GPU tests (-m gpu) of the blend statistics: settings._blend_stats = True makes every backward leave, in means2D.blend_stats, per
Gaussian the sum, the maximum and the count of its blend weights w = alpha * T over the pixels (include/stp_raster.h:
stp_set_backward_blend_stats).  Through the public API, except where the record buffer itself is looked at.

  * tiny scenes against the float64 yardstick (torch_ref_blend_stats.py): GLOBAL, k-buffer, hierarchical; replay and resort;
  * with colors_precomp as the leaf and dL_dout all ones the sum is dL/dcolour, which the existing path delivers;
  * a Gaussian blended by one pixel has max == sum;
  * frames whose tiles are partly replayed and partly re-sorted; replay == resort;
  * the statistics do not depend on dL_dout; the request moves nothing else; with absgrad and camera gradients in one backward;
  * the record buffer is zero again behind a request; empty and culled frames, refusals, overwrite.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import FULL_STP, GAUSS, _direct, _precomp, _rel, _scene_a, _scene_b, api_render, api_settings, ext_settings, settings_dict
from diff_gaussian_rasterization import scenes
import torch_ref_blend_stats

pytestmark = pytest.mark.gpu

MODES = {   # settings, the yardstick's order, the backward modes the settings have
    "global": (settings_dict(0), "global", (None,)),
    "kbuffer16": (settings_dict(2, per_pixel=16), "exact", ("replay", "resort")),
    "hier_full": (settings_dict(**FULL_STP), "exact", ("replay", "resort")),
}
CASES = [(m, bm) for m, (_, _, bms) in MODES.items() for bm in bms]
CASE_IDS = [f"{m}-{bm or 'own'}" for m, bm in CASES]


render = functools.partial(api_render, stats=True)


def _check_shape(got, P):
    s = got["stats"]
    assert s is not None and s.shape == (P, 3) and s.dtype == torch.float32 and s.device.type == "cuda" and not s.requires_grad
    assert torch.isfinite(s).all() and torch.all(s >= 0)
    assert torch.all(s[got["radii"] <= 0] == 0)
    assert torch.equal(s[:, 2], s[:, 2].round()) and torch.equal(s[:, 2] == 0, s[:, 0] == 0)
    # w = alpha T <= 0.99 -- with four float32 roundings of room: the GLOBAL backward rebuilds T back to front by division, T / (1 - alpha),
    # which can come out an ulp or two above the forward's T = 1 of a list's first entry
    assert torch.all(s[:, 1] <= np.float32(0.99) * (1 + 4 * 2.0 ** -24)) and torch.all(s[:, 1] <= s[:, 0] * (1 + 1e-6))


def _same_stats(a, b, what=""):
    """count and max bit-equal, sum to 1e-5 of the largest entry"""
    assert torch.equal(a[:, 2], b[:, 2]), f"{what}: counts differ for {int((a[:, 2] != b[:, 2]).sum())} Gaussians"
    assert torch.equal(a[:, 1], b[:, 1]), f"{what}: maxima differ for {int((a[:, 1] != b[:, 1]).sum())} Gaussians"
    assert _rel(a[:, 0].cpu().numpy(), b[:, 0].cpu().numpy()) < 1e-5, what


# ---- 1. against the float64 yardstick --------------------------------------------------------------------------------------------
# Tolerance of sum and max, relative to the column's largest entry: ten times the largest error measured on MI355X over the ten cases
# below (float32 alpha = opacity * exp(power) and a float32 transmittance chain against float64).
YARD_MEASURED = 9.3e-7
YARD_TOL = 10 * YARD_MEASURED


@pytest.mark.parametrize("camera", ["origin", "orbit"])
@pytest.mark.parametrize("mode,backward_mode", CASES, ids=CASE_IDS)
def test_blend_stats_match_float64_yardstick(mode, backward_mode, camera):
    """Sum and max within YARD_TOL = 9.3e-6 of the column's largest entry: ten times the largest error measured on MI355X, which was
    1.0e-7 .. 2.7e-7 for the sum in GLOBAL, both replays and the k-buffer re-sort, 4.4e-7 .. 6.6e-7 in the hierarchical re-sort, and
    3.3e-7 (origin) .. 9.3e-7 (orbit) for the max in every kernel.  Every count was equal.  The count equal for every Gaussian the yardstick does not mark as hanging on a rounding (at most 1 % are
    marked: asserted here and, without a GPU, in test_blend_stats_cpu.py)."""
    sd, order, _ = MODES[mode]
    sc = scenes.make_scene(P=150, W=40, H=36, sigma_min=1.0, sigma_max=8.0, seed=torch_ref_blend_stats.YARD_SEED, camera=camera)
    ref, explained, _ = torch_ref_blend_stats.blend_stats(sc, order=order, key=(camera, order))
    assert explained.mean() <= 0.01
    got = render(sc, sd, backward_mode=backward_mode)
    _check_shape(got, sc.P)
    s = got["stats"].cpu().numpy().astype(np.float64)
    err_sum, err_max = _rel(s[:, 0], ref[:, 0]), _rel(s[:, 1], ref[:, 1])
    bad = (s[:, 2] != ref[:, 2]) & ~explained
    print(f"\n{mode} {backward_mode} {camera}: sum rel err {err_sum:.2e}, max rel err {err_max:.2e}, counts differ for {int((s[:, 2] != ref[:, 2]).sum())} "
          f"Gaussians ({int(bad.sum())} unexplained), {int(explained.sum())} marked, {int((ref[:, 2] > 0).sum())} blended")
    assert (ref[:, 2] > 0).sum() > 30
    assert err_sum < YARD_TOL
    assert err_max < YARD_TOL
    assert not bad.any(), np.nonzero(bad)[0]


# ---- 2. the sum is dL/dcolour under an all-ones dL_dout ----------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["a", "b"])
@pytest.mark.parametrize("mode,backward_mode", CASES, ids=CASE_IDS)
def test_sum_is_the_colour_gradient_under_all_ones(mode, backward_mode, scene):
    """dL/dcolour[i, ch] = sum_p w[p, i] dL_dout[ch, p]: with dL_dout = 1 the existing gradient path delivers column 0, up to summation
    order (1e-5 of the largest entry).  Scene b has tile lists above 1024 entries: the replay's sliding window and its stragglers."""
    sc = _precomp(_scene_a() if scene == "a" else _scene_b())
    got = render(sc, MODES[mode][0], backward_mode=backward_mode, w=np.ones((3, sc.H, sc.W), np.float32))
    _check_shape(got, sc.P)
    s, g = got["stats"], got["colors_precomp"]
    assert int((s[:, 2] > 0).sum()) > 100
    r = _rel(s[:, 0].cpu().numpy(), g[:, 0].cpu().numpy())
    print(f"\n{mode} {backward_mode} {scene}: sum vs dL/dcolour rel {r:.2e}, largest count {int(s[:, 2].max())}, largest max {float(s[:, 1].max()):.3f}")
    assert r < 1e-5


# ---- 3. a single contribution: max == sum -----------------------------------------------------------------------------------------
_lit = {}


def _lit_pixel(mode):
    """flat index of the pixel that blends the most entries (from a recording forward, whose n_contrib counts the blended entries)"""
    if mode not in _lit:
        n = render(_scene_b(), MODES[mode][0], backward_mode="replay" if mode != "global" else None, forward_only=True)["n_contrib"]
        _lit[mode] = int(torch.argmax(n))
    return _lit[mode]


@pytest.mark.parametrize("mode,backward_mode", CASES, ids=CASE_IDS)
def test_single_contribution_has_max_equal_to_sum(mode, backward_mode):
    """dL_dout lit at one pixel (the statistics cover every pixel all the same).  A sum of one term is the term: bit-equal -- in the
    replay kernel because every blend weight is a whole number of the on-chip fixed point's 2^-45."""
    sc = _scene_b()
    got = render(sc, MODES[mode][0], backward_mode=backward_mode, lit_pixel=_lit_pixel(mode))
    _check_shape(got, sc.P)
    s = got["stats"]
    one = s[:, 2] == 1
    print(f"\n{mode} {backward_mode}: {int(one.sum())} Gaussians blended once, {int((s[:, 2] > 1).sum())} more often")
    assert int(one.sum()) >= 5 and int((s[:, 2] > 1).sum()) >= 100
    assert torch.equal(s[one, 1], s[one, 0])
    many = s[:, 2] > 1
    assert torch.all(s[many, 1] < s[many, 0])


# ---- 4. frames with replayed and overflowed tiles -------------------------------------------------------------------------------------
def _haze(mixed):
    sc = scenes.make_scene(P=5000, W=96, H=64, sigma_min=3.0, sigma_max=16.0, seed=23, opacity_range=(0.01, 0.05))
    if mixed:
        sc.opacities[sc.means3D[:, 0] > 0.0] = 0.6   # the right half of the image saturates after a few dozen blends: its tiles are replayed
    return sc


HAZE_CASES = {"haze-hier_full": (False, MODES["hier_full"][0]), "haze-kbuffer16": (False, MODES["kbuffer16"][0]),
              "mixed-hier_full": (True, MODES["hier_full"][0]), "mixed-kbuffer8": (True, settings_dict(2, per_pixel=8))}


@pytest.mark.parametrize("case", list(HAZE_CASES))
def test_overflowed_and_replayed_tiles(case):
    """The haze: tiles whose blend log overflowed go to the re-sorting kernel, the others are replayed.  Both write the three terms, and
    the result is that of a run that re-sorts every tile: count and max exactly (a maximum has no summation order), sum to 1e-5.  In the
    plain haze every tile overflows; in the mixed frames, whose right half is opaque, both kinds of tile meet in the records."""
    mixed, sd = HAZE_CASES[case]
    mode = case
    sc = _haze(mixed)
    got = render(sc, sd, backward_mode="replay")
    flags = got["tile_flags"]
    assert flags is not None and flags.any(), "scene did not overflow the blend log: test is vacuous"
    if mixed:
        assert not flags.all(), "no tile was replayed: test is vacuous"
    ref = render(sc, sd, backward_mode="resort")
    _check_shape(got, sc.P)
    _check_shape(ref, sc.P)
    a, b = got["stats"], ref["stats"]
    print(f"\n{mode}: {int((flags != 0).sum())} of {flags.size} tiles overflowed; counts differ for {int((a[:, 2] != b[:, 2]).sum())}, maxima for "
          f"{int((a[:, 1] != b[:, 1]).sum())} of {int((b[:, 2] > 0).sum())} Gaussians; sum rel {_rel(a[:, 0].cpu().numpy(), b[:, 0].cpu().numpy()):.2e}")
    _same_stats(a, b, mode)


# ---- 5. independence from dL_dout ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,backward_mode", CASES, ids=CASE_IDS)
def test_statistics_do_not_depend_on_dL_dout(mode, backward_mode):
    sc = scenes.make_scene(P=400, W=64, H=64, sigma_min=1.0, sigma_max=8.0, seed=7, camera="orbit")
    shape = (3, sc.H, sc.W)
    rnd = np.random.default_rng(3).normal(size=shape).astype(np.float32)
    bad = rnd.copy()
    bad[0, ::7, ::5], bad[1, 3::11, :] = np.nan, np.inf
    runs = {n: render(sc, MODES[mode][0], backward_mode=backward_mode, w=w)
            for n, w in (("zeros", np.zeros(shape, np.float32)), ("ones", np.ones(shape, np.float32)), ("random", rnd), ("non-finite", bad))}
    for n, got in runs.items():
        _check_shape(got, sc.P)
        assert int((got["stats"][:, 2] > 0).sum()) > 100
        _same_stats(got["stats"], runs["ones"]["stats"], f"{mode} {backward_mode} {n}")


# ---- 6. the request changes nothing else ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,backward_mode", CASES, ids=CASE_IDS)
def test_request_changes_nothing_else(mode, backward_mode):
    sd = MODES[mode][0]
    sc = scenes.make_scene(P=20000, W=256, H=256, sigma_min=1.0, sigma_max=10.0, seed=3, camera="orbit")
    a = render(sc, sd, backward_mode=backward_mode)
    b, b2 = render(sc, sd, stats=False, backward_mode=backward_mode), render(sc, sd, stats=False, backward_mode=backward_mode)
    assert a["has_stats"] and not b["has_stats"] and not b2["has_stats"] and a["absgrad"] is None
    assert torch.equal(a["color"], b["color"]) and torch.equal(a["radii"], b["radii"])
    for n in GAUSS:
        if b[n] is None:
            assert a[n] is None, n
            continue
        spread = (b[n] - b2[n]).abs().max().item()
        if spread == 0:
            # (the render half's float atomics are the only run-to-run variation; where two plain runs agree bit for bit the request,
            # which adds three terms next to the sums and touches none of the nine, must too)
            assert torch.equal(a[n], b[n]), n
        else:
            assert (a[n] - b[n]).abs().max().item() <= 4 * spread, n
    _check_shape(a, sc.P)


# ---- 7. with absgrad and camera gradients in the same backward -------------------------------------------------------------------------
@pytest.mark.parametrize("mode,backward_mode", CASES, ids=CASE_IDS)
def test_with_absgrad_and_camera_gradients(mode, backward_mode):
    sc = scenes.make_scene(P=400, W=64, H=64, sigma_min=1.0, sigma_max=8.0, seed=7, camera="orbit")
    sd = MODES[mode][0]
    kw = dict(backward_mode=backward_mode)
    all3 = render(sc, sd, absgrad=True, camera=True, **kw)
    only_stats, only_abs, only_cam = render(sc, sd, **kw), render(sc, sd, stats=False, absgrad=True, **kw), render(sc, sd, stats=False, camera=True, **kw)
    assert all3["grad_fn"] == "_RasterizeGaussiansCameraBackward" and only_stats["grad_fn"] == "_RasterizeGaussiansBackward"
    assert not only_abs["has_stats"] and not only_cam["has_stats"] and only_stats["absgrad"] is None
    _check_shape(all3, sc.P)
    _same_stats(all3["stats"], only_stats["stats"], "all three")
    assert all3["absgrad"].shape == (sc.P, 3) and _rel(all3["absgrad"].cpu().numpy(), only_abs["absgrad"].cpu().numpy()) < 1e-5
    for n in ("viewmatrix", "projmatrix", "campos"):
        assert all3[n] is not None and _rel(all3[n].cpu().numpy(), only_cam[n].cpu().numpy()) < 1e-5, n
    both = render(sc, sd, absgrad=True, **kw)
    _same_stats(both["stats"], only_stats["stats"], "with absgrad")
    assert _rel(both["absgrad"].cpu().numpy(), only_abs["absgrad"].cpu().numpy()) < 1e-5


# ---- 8. the record buffer behind a request -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,backward_mode", CASES, ids=CASE_IDS)
def test_records_are_zero_again_behind_a_request(mode, backward_mode):
    """A caller who keeps the record buffer between steps (phases bit 3: the per-Gaussian half clears what it reads) finds it all zeros
    behind a backward with the request too -- slots 11 .. 13 included, two of which lie behind the 48 bytes that bit clears -- and the
    next backwards on the same buffer, without and with the request, give what a fresh buffer gives."""
    from diff_gaussian_rasterization import _C
    sc = scenes.make_scene(P=3000, W=128, H=96, sigma_min=1.5, sigma_max=12.0, seed=21, camera="orbit")
    sd = {**MODES[mode][0], "_record_blend_log": backward_mode == "replay", "_backward_mode": backward_mode or "resort"}
    args = _direct(sc, sd)
    fresh = lambda: torch.zeros(sc.P, _C.GRAD_RECORD_FLOATS, device="cuda:0")
    plain = _C.rasterize_gaussians_backward(*args, phases=3 | 8, partial=fresh())
    assert len(plain) == 8
    buf = fresh()
    first = _C.rasterize_gaussians_backward(*args, phases=3 | 8, partial=buf, blend_stats=True)
    assert len(first) == 9 and first[8].shape == (sc.P, 3) and float(first[8][:, 2].max()) > 1
    assert not buf.any(), "records are not zero-filled again behind a backward with the request"
    second = _C.rasterize_gaussians_backward(*args, phases=3 | 8, partial=buf)
    assert len(second) == 8 and not buf.any()
    for k in range(8):
        assert _rel(second[k].cpu().numpy(), plain[k].cpu().numpy()) < 1e-5, k
        assert _rel(first[k].cpu().numpy(), plain[k].cpu().numpy()) < 1e-5, k
    third = _C.rasterize_gaussians_backward(*args, phases=3 | 8, partial=buf, absgrad=True, blend_stats=True)
    assert len(third) == 10 and not buf.any()
    _same_stats(third[9], first[8], "second request on the kept buffer")
    # the compact record has no room for the three terms, a split half is refused: the refusal consumes the request
    with pytest.raises(RuntimeError, match="blend statistics.*compact"):
        _C.rasterize_gaussians_backward(*args, phases=3 | 4, blend_stats=True)
    with pytest.raises(RuntimeError, match="blend statistics.*chunked per-Gaussian half"):
        _C.rasterize_gaussians_backward(*args, phases=3 | (2 << 8), blend_stats=True)   # (K = 2 chunks, through the C ABI's own check)
    with pytest.raises(RuntimeError, match="blend_stats needs both halves"):
        _C.rasterize_gaussians_backward(*args, phases=2, partial=fresh(), blend_stats=True)
    assert len(_C.rasterize_gaussians_backward(*args, phases=3)) == 8
    # both requests pending for a call that is refused (for absgrad, which is checked first): neither may stay behind for the next, plain
    # backward of the thread -- it would write P x 3 floats through a pointer whose tensor is gone
    with pytest.raises(RuntimeError, match="compact"):
        _C.rasterize_gaussians_backward(*args, phases=3 | 4, absgrad=True, blend_stats=True)
    with pytest.raises(RuntimeError, match="chunked per-Gaussian half"):
        _C.rasterize_gaussians_backward(*args, phases=3 | (2 << 8), absgrad=True, blend_stats=True)
    kept = fresh()   # (without bit 3 nothing clears the records: a request left behind shows in slots 9 .. 13)
    after = _C.rasterize_gaussians_backward(*args, phases=3, partial=kept)
    assert len(after) == 8 and kept[:, :9].any() and not kept[:, 9:].any(), "a refused call left a request behind"
    for k in range(8):
        assert _rel(after[k].cpu().numpy(), plain[k].cpu().numpy()) < 1e-5, k


# ---- 9. surface -------------------------------------------------------------------------------------------------------------------------
def test_empty_culled_and_single_gaussian_frames():
    empty = scenes.make_scene(P=1, W=48, H=40, sigma_min=1.0, sigma_max=2.0, seed=1, camera="orbit")
    for f in ("means3D", "scales", "rotations", "opacities", "shs"):
        setattr(empty, f, getattr(empty, f)[:0])
    got = render(empty, settings_dict(**FULL_STP), only=("opacities", "means2D"))
    assert got["has_stats"] and got["stats"].shape == (0, 3) and got["stats"].dtype == torch.float32 and got["stats"].is_cuda
    behind = scenes.make_scene(P=200, W=48, H=40, sigma_min=1.0, sigma_max=8.0, seed=7)   # camera at the origin looking down +z
    behind.means3D = (behind.means3D * np.array([1, 1, -1], np.float32)).astype(np.float32)
    for sd, _, _ in MODES.values():
        got = render(behind, sd)
        assert int(got["radii"].max()) == 0
        assert got["stats"].shape == (200, 3) and torch.equal(got["stats"], torch.zeros_like(got["stats"]))
    one = scenes.make_scene(P=1, W=48, H=40, sigma_min=3.0, sigma_max=4.0, seed=1)
    for sd, _, bms in MODES.values():
        for bm in bms:
            got = render(one, sd, backward_mode=bm)
            _check_shape(got, 1)
            s = got["stats"][0]
            if int(got["radii"][0]) > 0:   # alone in the frame: T = 1 in front of it, its weight is its alpha
                assert float(s[2]) >= 1 and 0 < float(s[1]) <= min(0.99, float(one.opacities[0, 0])) * (1 + 1e-6)


def test_blend_stats_refusals():
    from diff_gaussian_rasterization import tile_shard
    sc = scenes.make_scene(P=100, W=48, H=40, sigma_min=1.0, sigma_max=6.0, seed=2, camera="orbit")
    with pytest.raises(RuntimeError, match="blend statistics.*render_depth"):
        render(sc, settings_dict(3), render_depth=True)
    dev = torch.device("cuda:0")
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    es = ext_settings(settings_dict(3))
    es._blend_stats = True
    rs = api_settings(sc, es, dev)
    m = t(sc.means3D).requires_grad_(True)
    with pytest.raises(RuntimeError, match=r"blend statistics.*tile-row sharding.*\(P, 9\)"):
        tile_shard.TileRowShardedRasterizer(rs, None, 0, 1)(m, torch.zeros_like(m), t(sc.opacities), shs=t(sc.shs), scales=t(sc.scales),
                                                            rotations=t(sc.rotations))


def test_second_backward_overwrites_blend_stats():
    """Assigned, not accumulated: means2D.grad holds the sum of both steps, blend_stats the second step's alone -- a new tensor with the
    first step's values (the statistics do not depend on the loss)."""
    sc = scenes.make_scene(P=400, W=64, H=64, sigma_min=1.0, sigma_max=8.0, seed=7, camera="orbit")
    got = render(sc, settings_dict(**FULL_STP), backwards=2)
    first, second = got["all_stats"]
    assert first is not second and got["stats"] is second
    _same_stats(second, first, "second backward")
    once = render(sc, settings_dict(**FULL_STP))
    assert _rel(got["means2D"].cpu().numpy(), 3.0 * once["means2D"].cpu().numpy()) < 1e-5
