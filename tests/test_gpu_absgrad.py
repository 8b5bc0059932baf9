"""GPU tests (-m gpu) of absgrad: settings._absgrad = True makes every backward leave, in means2D.absgrad, the per-Gaussian sums over
pixels of |that pixel's contribution to dL/dmeans2D| (include/stp_raster.h: stp_set_backward_absgrad).  Through the public API only.

  * tiny scenes against the float64 yardstick (torch_ref_absgrad.py): GLOBAL, k-buffer, hierarchical; replay and resort;
  * a loss with ONE lit pixel: every Gaussian receives a single contribution, absgrad == |means2D.grad| -- on every kernel path, at
    sizes the dense yardstick cannot reach (one window, the sliding window, the blocked and the rows log);
  * many contributions: absgrad >= |grad| everywhere and strictly above it for a good part of the Gaussians (an absolute value taken
    after the lanes' merge, or after the sum, fails this); replay == resort;
  * frames whose tiles are partly replayed and partly re-sorted;
  * the request moves nothing else; the surface (camera gradients, frozen means2D, empty frames, refusals, overwrite).
"""
import functools

import numpy as np
import pytest
import torch

from helpers import FULL_STP, GAUSS, _direct, _rel, _scene_a, _scene_b, api_render, api_settings, ext_settings, max_abs, settings_dict
from diff_gaussian_rasterization import scenes
import torch_ref_absgrad

pytestmark = pytest.mark.gpu

render = functools.partial(api_render, absgrad=True)


def _check_shape(got, P):
    a = got["absgrad"]
    assert a is not None and a.shape == (P, 3) and a.dtype == torch.float32 and a.device.type == "cuda"
    assert not a.requires_grad and torch.all(a[:, 2] == 0) and torch.isfinite(a).all() and torch.all(a >= 0)
    assert torch.all(a[got["radii"] <= 0] == 0)


# ---- 1. against the float64 yardstick --------------------------------------------------------------------------------------------
YARD = {   # settings, the yardstick's order, the backward modes the settings have
    "global": (settings_dict(0), "global", (None,)),
    "kbuffer16": (settings_dict(2, per_pixel=16), "exact", ("replay", "resort")),
    "hier": (settings_dict(3), "exact", ("replay", "resort")),
}
YARD_CASES = [(m, bm) for m, (_, _, bms) in YARD.items() for bm in bms]


@pytest.mark.parametrize("camera", ["origin", "orbit"])
@pytest.mark.parametrize("mode,backward_mode", YARD_CASES, ids=[f"{m}-{bm or 'own'}" for m, bm in YARD_CASES])
def test_absgrad_matches_float64_yardstick(mode, backward_mode, camera):
    """max |absgrad - yardstick| below 1e-4 of the largest entry (the relative tolerance of GPU gradients); in the same
    run means2D.grad to 5e-5 and the image to 2e-6, as the existing float64 comparisons ask."""
    sd, order, _ = YARD[mode]
    sc = scenes.make_scene(P=150, W=40, H=36, sigma_min=1.0, sigma_max=8.0, seed=7, camera=camera)
    img, ref_abs, ref_signed = torch_ref_absgrad.absgrad(sc, order=order, key=(camera, order))
    got = render(sc, sd, backward_mode=backward_mode)
    _check_shape(got, sc.P)
    a = got["absgrad"].cpu().numpy()
    err_abs, err_grad, err_img = _rel(a[:, :2], ref_abs), _rel(got["means2D"].cpu().numpy()[:, :2], ref_signed), \
        max_abs(got["color"].cpu().numpy(), img)
    print(f"\n{mode} {backward_mode} {camera}: absgrad rel err {err_abs:.2e}, means2D.grad rel err {err_grad:.2e}, image {err_img:.2e}")
    assert err_abs < 1e-4
    assert err_grad < 5e-5
    assert err_img < 2e-6
    assert float(np.mean(ref_abs > np.abs(ref_signed) * 1.01)) > 0.3   # (the scene tells the two quantities apart)


# ---- 2. a single contribution per Gaussian: absgrad == |grad| ----------------------------------------------------------------------
SINGLE = {
    "a-hier_full": (_scene_a, settings_dict(**FULL_STP)),
    "b-hier": (_scene_b, settings_dict(3)),
    "b-hier_full": (_scene_b, settings_dict(**FULL_STP)),
    "c-kbuffer16": (_scene_b, settings_dict(2, per_pixel=16)),
    "c-kbuffer4": (_scene_b, settings_dict(2, per_pixel=4)),
}


_lit = {}


def _lit_pixel(case):
    """(flat index, blends) of the pixel that blends the most entries: from a RECORDING forward, whose n_contrib is the number of log
    records = blended entries of the pixel (the other forwards keep the reference's contributor index there)."""
    if case not in _lit:
        make, sd = SINGLE[case]
        n = render(make(), sd, backward_mode="replay", forward_only=True)["n_contrib"]
        flat = int(torch.argmax(n))
        _lit[case] = (flat, int(n[flat]))
    return _lit[case]


@pytest.mark.parametrize("backward_mode", ["replay", "resort"])
@pytest.mark.parametrize("case", list(SINGLE))
def test_single_contribution_identity(case, backward_mode):
    """dL_dout lit at one pixel: every Gaussian gets at most one contribution, the sum of absolute values is the absolute value of the
    sum -- within 1e-6 of the largest entry.  Observed on MI355X: bit-equal on every replay path and in the k-buffer re-sorting kernel (the
    on-chip fixed point rounds symmetrically); 1.1e-9 at most in the re-sorting hierarchical kernel, whose signed terms alone pass the quad
    pre-reduction and the fixed point."""
    make, sd = SINGLE[case]
    sc = make()
    flat, blends = _lit_pixel(case)
    assert blends >= 30, blends
    got = render(sc, sd, backward_mode=backward_mode, lit_pixel=flat)
    _check_shape(got, sc.P)
    a, g = got["absgrad"][:, :2], got["means2D"][:, :2].abs()
    assert int((g.max(1).values > 0).sum()) >= 30
    diff = float((a - g).abs().max()) / float(g.max())
    print(f"\n{case} {backward_mode}: lit pixel blends {blends}, max |absgrad - |grad|| / max = {diff:.2e}, bit-equal {torch.equal(a, g)}")
    assert diff <= 1e-6


# ---- 3. many contributions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hier", "kbuffer16"])
def test_many_contributions_dominate_the_signed_gradient(name):
    sc = _scene_b()
    sd = settings_dict(3) if name == "hier" else settings_dict(2, per_pixel=16)
    runs = {bm: render(sc, sd, backward_mode=bm) for bm in ("replay", "resort")}
    for bm, got in runs.items():
        _check_shape(got, sc.P)
        a, g = got["absgrad"][:, :2], got["means2D"][:, :2].abs()
        top = float(a.max())
        assert top > 0
        assert torch.all(a >= g - 1e-6 * top), bm
        vis = got["radii"] > 0
        strictly = ((a > g + 1e-6 * top).any(1) & vis).sum().item()
        print(f"\n{name} {bm}: absgrad strictly above |grad| for {strictly} of {int(vis.sum())} visible Gaussians")
        assert strictly >= 0.25 * int(vis.sum()), (bm, strictly, int(vis.sum()))
    r = _rel(runs["replay"]["absgrad"].cpu().numpy(), runs["resort"]["absgrad"].cpu().numpy())
    print(f"{name}: replay vs resort absgrad rel {r:.2e}")
    assert r < 1e-4


# ---- 4. frames with replayed and overflowed tiles -------------------------------------------------------------------------------------
HAZE = dict(P=3000, W=48, H=48, sigma_min=10.0, sigma_max=20.0, seed=21, opacity_range=(0.01, 0.03))


def _mixed_scene():
    sc = scenes.make_scene(P=5000, W=96, H=64, sigma_min=3.0, sigma_max=16.0, seed=23, opacity_range=(0.01, 0.05))
    sc.opacities[sc.means3D[:, 0] > 0.0] = 0.6   # the right half of the image saturates after a few dozen blends
    return sc


@pytest.mark.parametrize("case", ["haze-hier", "haze-kbuffer16", "mixed-hier_full", "mixed-kbuffer8"])
def test_overflowed_and_replayed_tiles(case):
    """Tiles whose blend log overflowed go to the re-sorting kernel, the others are replayed: both write the two extra sums, and the
    result is that of a run that re-sorts every tile."""
    if case.startswith("haze"):
        sc, sd = scenes.make_scene(**HAZE), (settings_dict(3, h44=True) if case.endswith("hier") else settings_dict(2, per_pixel=16))
    else:
        sc, sd = _mixed_scene(), (settings_dict(**FULL_STP) if case.endswith("hier_full") else settings_dict(2, per_pixel=8))
    got = render(sc, sd, backward_mode="replay")
    flags = got["tile_flags"]
    assert flags is not None and flags.any(), "scene did not overflow the blend log: test is vacuous"
    if case.startswith("mixed"):
        assert not flags.all(), flags
    ref = render(sc, sd, backward_mode="resort")
    _check_shape(got, sc.P)
    r = _rel(got["absgrad"].cpu().numpy(), ref["absgrad"].cpu().numpy())
    print(f"\n{case}: {int((flags != 0).sum())} of {flags.size} tiles overflowed, absgrad vs resort rel {r:.2e}")
    assert r < 1e-4
    assert _rel(got["means2D"].cpu().numpy(), ref["means2D"].cpu().numpy()) < 1e-4
    assert torch.all(got["absgrad"][:, :2] >= got["means2D"][:, :2].abs() - 1e-6 * got["absgrad"].max())


# ---- 5. the request changes nothing else ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,backward_mode", [("hier_full", "replay"), ("hier_full", "resort"), ("kbuffer16", "replay"),
                                                ("kbuffer16", "resort"), ("global", None)])
def test_request_changes_nothing_else(name, backward_mode):
    sd = {"hier_full": settings_dict(**FULL_STP), "kbuffer16": settings_dict(2, per_pixel=16), "global": settings_dict(0)}[name]
    sc = scenes.make_scene(P=20000, W=256, H=256, sigma_min=1.0, sigma_max=10.0, seed=3, camera="orbit")
    a = render(sc, sd, backward_mode=backward_mode)
    b, b2 = render(sc, sd, absgrad=False, backward_mode=backward_mode), render(sc, sd, absgrad=False, backward_mode=backward_mode)
    assert a["has_absgrad"] and not b["has_absgrad"] and not b2["has_absgrad"]
    assert torch.equal(a["color"], b["color"]) and torch.equal(a["radii"], b["radii"])
    for n in GAUSS:
        if b[n] is None:
            assert a[n] is None, n
            continue
        spread = (b[n] - b2[n]).abs().max().item()
        if spread == 0:
            # (the render half's float atomics are the only run-to-run variation; where two plain runs agree bit for bit the request,
            # which adds two terms to the same sums and touches none of the nine, must too)
            assert torch.equal(a[n], b[n]), n
        else:
            assert (a[n] - b[n]).abs().max().item() <= 4 * spread, n
    _check_shape(a, sc.P)


@pytest.mark.parametrize("backward_mode", ["replay", "resort"])
def test_records_are_zero_again_behind_a_request(backward_mode):
    """A caller who keeps the record buffer between steps (phases bit 3: the per-Gaussian half clears what it reads) finds it all
    zeros behind a backward with the request too -- slots 9, 10 included -- and the next backwards on the same buffer, without and
    with the request, give what a fresh buffer gives."""
    from diff_gaussian_rasterization import _C
    sc = scenes.make_scene(P=3000, W=128, H=96, sigma_min=1.5, sigma_max=12.0, seed=21, camera="orbit")
    sd = {**settings_dict(**FULL_STP), "_record_blend_log": backward_mode == "replay", "_backward_mode": backward_mode}
    args = _direct(sc, sd)
    fresh = lambda: torch.zeros(sc.P, _C.GRAD_RECORD_FLOATS, device="cuda:0")
    plain = _C.rasterize_gaussians_backward(*args, phases=3 | 8, partial=fresh())
    assert len(plain) == 8
    buf = fresh()
    first = _C.rasterize_gaussians_backward(*args, phases=3 | 8, partial=buf, absgrad=True)
    assert len(first) == 9 and first[8].shape == (sc.P, 3) and float(first[8].max()) > 0
    assert not buf.any(), "records are not zero-filled again behind a backward with the request"
    second = _C.rasterize_gaussians_backward(*args, phases=3 | 8, partial=buf)
    assert len(second) == 8 and not buf.any()
    for k in range(8):
        assert _rel(second[k].cpu().numpy(), plain[k].cpu().numpy()) < 1e-5, k
        assert _rel(first[k].cpu().numpy(), plain[k].cpu().numpy()) < 1e-5, k
    third = _C.rasterize_gaussians_backward(*args, phases=3 | 8, partial=buf, absgrad=True)
    assert _rel(third[8].cpu().numpy(), first[8].cpu().numpy()) < 1e-5 and not buf.any()
    # the compact record has no room for the two sums, a chunked or a split half is refused: the refusal consumes the request
    with pytest.raises(RuntimeError, match="absgrad"):
        _C.rasterize_gaussians_backward(*args, phases=3 | 4, absgrad=True)
    with pytest.raises(RuntimeError, match="absgrad"):
        _C.rasterize_gaussians_backward(*args, phases=2, partial=fresh(), absgrad=True)
    assert len(_C.rasterize_gaussians_backward(*args, phases=3)) == 8


# ---- 6. surface -------------------------------------------------------------------------------------------------------------------------
def test_absgrad_with_camera_gradients():
    sc = scenes.make_scene(P=400, W=64, H=64, sigma_min=1.0, sigma_max=8.0, seed=7, camera="orbit")
    sd = settings_dict(**FULL_STP)
    both, plain, cam = render(sc, sd, camera=True), render(sc, sd), render(sc, sd, camera=True, absgrad=False)
    assert both["grad_fn"] == "_RasterizeGaussiansCameraBackward" and plain["grad_fn"] == "_RasterizeGaussiansBackward"
    _check_shape(both, sc.P)
    assert not cam["has_absgrad"]
    assert _rel(both["absgrad"].cpu().numpy(), plain["absgrad"].cpu().numpy()) < 1e-5
    for n in ("viewmatrix", "projmatrix", "campos"):
        assert both[n] is not None and _rel(both[n].cpu().numpy(), cam[n].cpu().numpy()) < 1e-5, n


@pytest.mark.parametrize("sd", [settings_dict(**FULL_STP), settings_dict(2, per_pixel=16), settings_dict(0)], ids=["hier_full", "kbuffer16", "global"])
def test_absgrad_with_frozen_means2D(sd):
    """means2D does not require grad and only the opacities do: the blend log is recorded, the render half runs, absgrad is delivered."""
    sc = scenes.make_scene(P=400, W=64, H=64, sigma_min=1.0, sigma_max=8.0, seed=7, camera="orbit")
    full = render(sc, sd)
    got = render(sc, sd, only=("opacities",), means2D_grad=False)
    assert got["means2D"] is None and got["means3D"] is None and got["opacities"] is not None
    _check_shape(got, sc.P)
    assert float(got["absgrad"].max()) > 0
    assert _rel(got["absgrad"].cpu().numpy(), full["absgrad"].cpu().numpy()) < 1e-5


def test_absgrad_of_empty_and_culled_frames():
    empty = scenes.make_scene(P=1, W=48, H=40, sigma_min=1.0, sigma_max=2.0, seed=1, camera="orbit")
    for f in ("means3D", "scales", "rotations", "opacities", "shs"):
        setattr(empty, f, getattr(empty, f)[:0])
    got = render(empty, settings_dict(**FULL_STP), only=("opacities", "means2D"))
    assert got["has_absgrad"] and got["absgrad"].shape == (0, 3) and got["absgrad"].dtype == torch.float32 and got["absgrad"].is_cuda
    behind = scenes.make_scene(P=200, W=48, H=40, sigma_min=1.0, sigma_max=8.0, seed=7)   # camera at the origin looking down +z
    behind.means3D = (behind.means3D * np.array([1, 1, -1], np.float32)).astype(np.float32)
    for sd in (settings_dict(**FULL_STP), settings_dict(2, per_pixel=16), settings_dict(0)):
        got = render(behind, sd)
        assert int(got["radii"].max()) == 0
        assert got["absgrad"].shape == (200, 3) and torch.equal(got["absgrad"], torch.zeros_like(got["absgrad"]))


def test_absgrad_refusals():
    from diff_gaussian_rasterization import tile_shard
    sc = scenes.make_scene(P=100, W=48, H=40, sigma_min=1.0, sigma_max=6.0, seed=2, camera="orbit")
    with pytest.raises(RuntimeError, match="absgrad.*render_depth"):
        render(sc, settings_dict(3), render_depth=True)
    dev = torch.device("cuda:0")
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    es = ext_settings(settings_dict(3))
    es._absgrad = True
    rs = api_settings(sc, es, dev)
    m = t(sc.means3D).requires_grad_(True)
    with pytest.raises(RuntimeError, match=r"absgrad.*tile-row sharding.*\(P, 9\)"):
        tile_shard.TileRowShardedRasterizer(rs, None, 0, 1)(m, torch.zeros_like(m), t(sc.opacities), shs=t(sc.shs), scales=t(sc.scales),
                                                            rotations=t(sc.rotations))


def test_second_backward_overwrites_absgrad():
    """Assigned, not accumulated: the second step's loss is twice the first's, means2D.grad holds the sum of both steps, absgrad the
    second step's alone."""
    sc = scenes.make_scene(P=400, W=64, H=64, sigma_min=1.0, sigma_max=8.0, seed=7, camera="orbit")
    got = render(sc, settings_dict(**FULL_STP), backwards=2)
    first, second = got["absgrads"]
    assert first is not second and got["absgrad"] is second
    assert _rel(second.cpu().numpy(), 2.0 * first.cpu().numpy()) < 1e-5
    once = render(sc, settings_dict(**FULL_STP))
    assert _rel(got["means2D"].cpu().numpy(), 3.0 * once["means2D"].cpu().numpy()) < 1e-5
