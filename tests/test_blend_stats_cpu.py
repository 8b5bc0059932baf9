"""CPU tests of the blend-statistics extension (settings._blend_stats / means2D.blend_stats; include/stp_raster.h:
stp_set_backward_blend_stats): the settings dict, the C ABI's declaration and export, the loader's message for a library without the
symbol, the refusals that come from the forward, and the float64 yardstick the GPU tests pin the kernels against."""
import os
import re
import types

import numpy as np
import pytest

from helpers import settings_dict
from diff_gaussian_rasterization import scenes
import torch_ref_blend_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blend_stats_rides_in_the_settings_dict():
    import diff_gaussian_rasterization as dgr
    es = dgr.ExtendedSettings.from_dict(settings_dict(3, h44=True))
    es._blend_stats = False   # (switched off: no key)
    assert es.to_dict() == settings_dict(3, h44=True)
    es._blend_stats = True
    assert es.to_dict() == {**settings_dict(3, h44=True), "_blend_stats": True}
    es._absgrad = True        # (a request of its own: both ride)
    assert es.to_dict() == {**settings_dict(3, h44=True), "_absgrad": True, "_blend_stats": True}
    assert "_blend_stats" not in {f for f in es.__dataclass_fields__}   # an extension attribute, not a field of the reference's dataclass


def test_header_declares_the_entry_point_and_the_record_slots():
    h = open(os.path.join(ROOT, "include", "stp_raster.h")).read()
    assert re.search(r"void\s+stp_set_backward_blend_stats\s*\(\s*float\s*\*\s*\w+", h)
    define = lambda n: int(re.search(rf"#define\s+{n}\s+(\d+)\b", h).group(1))
    assert define("STP_GRAD_RECORD_STATS") == 11
    assert define("STP_GRAD_RECORD_STATS") + 3 <= define("STP_GRAD_RECORD_FLOATS")
    assert define("STP_GRAD_RECORD_STATS") >= define("STP_GRAD_RECORD_ABS") + 2   # (behind absgrad's two slots)
    assert define("STP_ABI_VERSION") == 7
    hpp = open(os.path.join(ROOT, "include", "stp_rasterizer.hpp")).read()
    assert re.search(r"float\*\s*dL_dmean2D_abs\s*=\s*nullptr,\s*float\*\s*blend_stats\s*=\s*nullptr\)", hpp)   # one trailing optional argument


def test_library_exports_the_entry_point():
    from diff_gaussian_rasterization import _C
    L = _C._load()
    assert hasattr(L, "stp_set_backward_blend_stats")
    assert _C._require("stp_set_backward_blend_stats") is not None
    L.stp_set_backward_blend_stats(None)   # NULL only clears the (thread-local) request: callable without a GPU
    assert L.stp_abi_version() == 7


def test_loader_message_for_a_library_without_the_symbol(monkeypatch):
    from diff_gaussian_rasterization import _C
    monkeypatch.setattr(_C, "_lib", types.SimpleNamespace())   # a loaded library that predates the export
    with pytest.raises(RuntimeError) as ex:
        _C._require("stp_set_backward_blend_stats")
    assert str(ex.value) == (f"{_C.library_path()} does not export stp_set_backward_blend_stats (a library built before blend statistics): "
                             "rebuild it")


@pytest.mark.parametrize("camera", ["origin", "orbit"])
@pytest.mark.parametrize("order", ["global", "exact"])
def test_yardstick_is_consistent_with_itself(camera, order):
    """What a pixel's Gaussians take is what the background loses: sum_i sum_p w = sum_p (1 - T_final) (1e-12 relative); max <= sum; the
    count is zero exactly where the sum is; where it is one, the maximum is the sum."""
    sc = scenes.make_scene(P=150, W=40, H=36, sigma_min=1.0, sigma_max=8.0, seed=7, camera=camera)
    stats, explained, T_final = torch_ref_blend_stats.blend_stats(sc, order=order)
    assert stats.shape == (150, 3) and explained.shape == (150,) and T_final.shape == (40 * 36,)
    total = float(np.sum(1.0 - T_final))
    assert total > 100.0
    assert abs(float(stats[:, 0].sum()) - total) <= 1e-12 * total
    assert np.all(stats[:, 1] <= stats[:, 0]) and np.all(stats[:, 1] <= 0.99) and np.all(stats >= 0)
    assert np.array_equal(stats[:, 2] == 0, stats[:, 0] == 0)
    assert np.array_equal(stats[:, 2], np.round(stats[:, 2])) and (stats[:, 2] > 0).sum() > 30
    one = stats[:, 2] == 1
    assert np.array_equal(stats[one, 1], stats[one, 0])


def test_scene_of_the_gpu_comparison_has_few_pairs_that_hang_on_a_rounding():
    """The GPU test compares counts exactly except for Gaussians the yardstick itself marks (a pair with alpha within 1e-6 of 1/255, or
    T (1 - alpha) within 1e-6 relative of 1e-4): at most 1 % of them, for every camera and order it uses.  Seed 9: seed 7, the scene of
    the absgrad comparison, marks 4 of its 150 Gaussians with the camera at the origin."""
    for camera in ("origin", "orbit"):
        sc = scenes.make_scene(P=150, W=40, H=36, sigma_min=1.0, sigma_max=8.0, seed=torch_ref_blend_stats.YARD_SEED, camera=camera)
        for order in ("global", "exact"):
            _, explained, _ = torch_ref_blend_stats.blend_stats(sc, order=order)
            assert explained.mean() <= 0.01, (camera, order, int(explained.sum()))


def _cpu_settings(sc, render_depth=False):
    import torch
    import diff_gaussian_rasterization as dgr
    t = lambda a: torch.tensor(np.asarray(a, np.float32))
    es = dgr.ExtendedSettings.from_dict(settings_dict(3))
    es._blend_stats = True
    return dgr.GaussianRasterizationSettings(
        image_height=sc.H, image_width=sc.W, tanfovx=sc.tanfovx, tanfovy=sc.tanfovy, bg=t(sc.bg), scale_modifier=1.0, viewmatrix=t(sc.viewmatrix),
        projmatrix=t(sc.projmatrix), inv_viewprojmatrix=t(sc.inv_viewprojmatrix), sh_degree=sc.sh_degree, campos=t(sc.campos),
        prefiltered=False, settings=es, render_depth=render_depth, debug=False), t


def test_render_depth_and_tile_row_shard_refuse_the_request():
    """Both refusals come from the forward, in front of anything that touches a device."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import tile_shard
    sc = scenes.make_scene(P=20, W=32, H=32, sigma_min=1.0, sigma_max=4.0, seed=2)
    rs, t = _cpu_settings(sc, render_depth=True)
    m = t(sc.means3D).requires_grad_(True)
    call = dict(shs=t(sc.shs), scales=t(sc.scales), rotations=t(sc.rotations))
    with pytest.raises(RuntimeError, match="blend statistics.*render_depth"):
        dgr.GaussianRasterizer(rs)(m, m.detach() * 0, t(sc.opacities), **call)
    rs, _ = _cpu_settings(sc)
    with pytest.raises(RuntimeError, match=r"blend statistics.*tile-row sharding.*\(P, 9\)"):
        tile_shard.TileRowShardedRasterizer(rs, None, 0, 1)(m, m.detach() * 0, t(sc.opacities), **call)
