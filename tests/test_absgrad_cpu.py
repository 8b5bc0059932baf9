"""CPU tests of the absgrad extension (settings._absgrad / means2D.absgrad; include/stp_raster.h: stp_set_backward_absgrad): the settings
dict, the C ABI's declaration and export, the loader's message for a library without the symbol, and the float64 yardstick the GPU tests
pin the kernels against."""
import os
import re
import types

import numpy as np
import pytest

from helpers import settings_dict
from diff_gaussian_rasterization import scenes
import torch_ref
import torch_ref_absgrad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_settings_dict_is_unchanged():
    import diff_gaussian_rasterization as dgr
    assert dgr.ExtendedSettings().to_dict() == {
        "sort_settings": {"queue_sizes": {"tile_4x4": 64, "tile_2x2": 8, "per_pixel": 4}, "sort_mode": 0, "sort_order": 0},
        "culling_settings": {"rect_bounding": False, "tight_opacity_bounding": False, "tile_based_culling": False,
                             "hierarchical_4x4_culling": False},
        "load_balancing": False, "proper_ewa_scaling": False}
    es = dgr.ExtendedSettings.from_dict(settings_dict(3, h44=True))
    assert es.to_dict() == settings_dict(3, h44=True)
    es._absgrad = False   # (switched off again: no key)
    assert es.to_dict() == settings_dict(3, h44=True)


def test_absgrad_rides_in_the_settings_dict():
    import diff_gaussian_rasterization as dgr
    es = dgr.ExtendedSettings.from_dict(settings_dict(3, h44=True))
    es._absgrad = True
    assert es.to_dict() == {**settings_dict(3, h44=True), "_absgrad": True}
    es._backward_mode = "resort"
    assert es.to_dict() == {**settings_dict(3, h44=True), "_backward_mode": "resort", "_absgrad": True}
    assert "_absgrad" not in {f for f in es.__dataclass_fields__}   # an extension attribute, not a field of the reference's dataclass


def test_header_declares_the_entry_point_and_the_record_slots():
    h = open(os.path.join(ROOT, "include", "stp_raster.h")).read()
    assert re.search(r"void\s+stp_set_backward_absgrad\s*\(\s*float\s*\*\s*dL_dmean2D_abs", h)
    assert re.search(r"#define\s+STP_GRAD_RECORD_ABS\s+9\b", h)
    assert re.search(r"#define\s+STP_ABI_VERSION\s+7\b", h)
    assert re.search(r"#define\s+STP_GRAD_RECORD_USED\s+9\b", h) and re.search(r"#define\s+STP_GRAD_RECORD_FLOATS\s+16\b", h)
    assert "[9..10] sum |dL/dmean2D| xy (only with the absgrad request)" in h


def test_library_exports_the_entry_point():
    from diff_gaussian_rasterization import _C
    L = _C._load()
    assert hasattr(L, "stp_set_backward_absgrad")
    assert _C._require("stp_set_backward_absgrad") is not None
    L.stp_set_backward_absgrad(None)   # NULL only clears the (thread-local) request: callable without a GPU
    assert L.stp_abi_version() == 7


def test_loader_message_for_a_library_without_the_symbol(monkeypatch):
    from diff_gaussian_rasterization import _C
    monkeypatch.setattr(_C, "_lib", types.SimpleNamespace())   # a loaded library that predates the export
    with pytest.raises(RuntimeError) as ex:
        _C._require("stp_set_backward_absgrad")
    assert str(ex.value) == f"{_C.library_path()} does not export stp_set_backward_absgrad (a library built before absgrad): rebuild it"
    with pytest.raises(RuntimeError, match=r"does not export stp_set_backward_camera_grads \(a library built before camera gradients\): rebuild it"):
        _C._require("stp_set_backward_camera_grads")


@pytest.mark.parametrize("camera", ["origin", "orbit"])
@pytest.mark.parametrize("order", ["global", "exact"])
def test_yardstick_signed_sum_is_torch_refs_means2D_gradient(camera, order):
    """The signed sum of the yardstick's per-pixel contributions is torch_ref's dL/dmeans2D (1e-10 relative), its image torch_ref's; the
    absolute sums dominate the signed ones and exceed them for most Gaussians."""
    sc = scenes.make_scene(P=150, W=40, H=36, sigma_min=1.0, sigma_max=8.0, seed=7, camera=camera)
    img0, g0 = torch_ref.loss_and_grads(sc, order=order)
    img, ab, signed = torch_ref_absgrad.absgrad(sc, order=order)
    assert np.max(np.abs(img - img0)) < 1e-12
    ref = g0["means2D"]
    assert ab.shape == ref.shape == signed.shape == (150, 2)
    assert np.max(np.abs(signed - ref)) <= 1e-10 * np.max(np.abs(ref))
    assert np.all(ab >= np.abs(signed) - 1e-12 * ab.max())
    touched = ab.max(1) > 0
    assert touched.sum() > 30 and np.mean((ab > np.abs(signed) * (1 + 1e-9))[touched]) > 0.5


def _cpu_settings(sc, render_depth=False):
    import torch
    import diff_gaussian_rasterization as dgr
    t = lambda a: torch.tensor(np.asarray(a, np.float32))
    es = dgr.ExtendedSettings.from_dict(settings_dict(3))
    es._absgrad = True
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
    with pytest.raises(RuntimeError, match="absgrad.*render_depth"):
        dgr.GaussianRasterizer(rs)(m, m.detach() * 0, t(sc.opacities), **call)
    rs, _ = _cpu_settings(sc)
    with pytest.raises(RuntimeError, match=r"absgrad.*tile-row sharding.*\(P, 9\)"):
        tile_shard.TileRowShardedRasterizer(rs, None, 0, 1)(m, m.detach() * 0, t(sc.opacities), **call)
