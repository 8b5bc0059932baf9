"""CPU tests of the split SH inputs (GaussianRasterizer.forward's dc=; include/stp_raster.h: stp_set_forward_split_sh,
stp_set_backward_split_sh): the C ABI's declarations and exports, the requests called without a device, the public signature, and the
refusals that are raised before any device work."""
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

from helpers import FULL_STP, settings_dict
from diff_gaussian_rasterization import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("stp_set_forward_split_sh", "stp_set_backward_split_sh")


def test_header_declares_the_two_requests():
    h = open(os.path.join(ROOT, "include", "stp_raster.h")).read()
    assert int(re.search(r"#define\s+STP_ABI_VERSION\s+(\d+)\b", h).group(1)) == 7
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)   # (the declarations carry their shapes as comments)
    assert re.search(r"void\s+stp_set_forward_split_sh\s*\(\s*const\s+float\s*\*\s*dc\s*\)\s*;", h)
    assert re.search(r"void\s+stp_set_backward_split_sh\s*\(\s*const\s+float\s*\*\s*dc\s*,\s*float\s*\*\s*dL_ddc\s*\)\s*;", h)


@pytest.mark.parametrize("lib", ["libstp_raster.so", "libstp_raster_fma.so"])
def test_both_libraries_export_the_two_requests(lib):
    from diff_gaussian_rasterization import _C
    path = os.path.join(os.path.dirname(_C.library_path()), lib)
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in SYMBOLS:
        assert name in exported, (lib, name)


def test_requests_are_callable_without_a_device():
    import ctypes
    from diff_gaussian_rasterization import _C
    L = _C._load()
    assert L.stp_abi_version() == 7
    for name in SYMBOLS:
        assert hasattr(L, name) and _C._require(name) is not None
    buf = (ctypes.c_float * 6)()
    out = (ctypes.c_float * 6)()
    L.stp_set_forward_split_sh(buf)          # a pending request ...
    L.stp_set_forward_split_sh(None)         # ... cleared by a NULL dc
    L.stp_set_backward_split_sh(buf, out)
    L.stp_set_backward_split_sh(None, None)
    L.stp_set_backward_split_sh(None, out)   # (a NULL dc clears, whatever the second pointer)


def test_backward_request_is_checked_and_consumed():
    """stp_backward_phases with a pending request: dc without dL_ddc is refused on the request itself, before any argument is read; the
    per-Gaussian call consumes the request whatever its outcome, a render-only call (phases = 1) leaves it pending."""
    import ctypes
    from diff_gaussian_rasterization import _C
    L = _C._load()
    buf = (ctypes.c_float * 4)()
    call = lambda phases: L.stp_backward_phases(*([ctypes.c_int(phases)] + [ctypes.c_int(0)] * 4 + [None] * 35))
    err = lambda: L.stp_last_error().decode()
    L.stp_set_backward_split_sh(buf, None)
    assert call(3) < 0 and "split SH" in err() and "dL_ddc" in err()
    assert call(3) < 0 and "split SH" not in err()   # (consumed: the next call fails on its null settings)
    L.stp_set_backward_split_sh(buf, None)
    assert call(1) < 0 and "split SH" not in err()   # render-only: neither checked nor consumed ...
    assert call(2) < 0 and "split SH" in err()       # ... the per-Gaussian call finds it
    assert call(2) < 0 and "split SH" not in err()


@pytest.mark.parametrize("name", SYMBOLS)
def test_loader_message_for_a_library_without_the_symbols(monkeypatch, name):
    from diff_gaussian_rasterization import _C
    monkeypatch.setattr(_C, "_lib", types.SimpleNamespace())   # a loaded library that predates the exports
    with pytest.raises(RuntimeError) as ex:
        _C._require(name)
    assert str(ex.value) == f"{_C.library_path()} does not export {name} (a library built before split SH inputs): rebuild it"


def test_forward_signature_has_dc_last():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C, tile_shard
    for cls in (dgr.GaussianRasterizer, tile_shard.TileRowShardedRasterizer):
        names = list(inspect.signature(cls.forward).parameters)
        assert names == ["self", "means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp", "dc"]
        assert inspect.signature(cls.forward).parameters["dc"].default is None
    # the binding's wrappers: dc is a keyword behind the 22 / 25 positional arguments and the earlier extensions
    for fn, positional in ((_C.rasterize_gaussians, 22), (_C.rasterize_gaussians_backward, 25)):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "dc" and params[-1].default is None
        assert sum(p.default is inspect.Parameter.empty for p in params) == positional
    # the three Functions take dc as their last input
    for fn in (dgr._RasterizeGaussians, dgr._RasterizeGaussiansCamera, dgr._RasterizeGaussiansBackground):
        p = list(inspect.signature(fn.forward).parameters.values())[-1]
        assert p.name == "dc" and p.default is None


def tiny():
    return scenes.make_scene(P=40, W=48, H=32, sigma_min=1.0, sigma_max=9.0, seed=4)


def _cpu_call(sc, dc, rest, colors=None, sharded=False):
    """The public forward on CPU tensors: a refusal that needs no device is raised before the binding asks for a GPU tensor."""
    import torch
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import tile_shard
    t = lambda a: torch.tensor(np.asarray(a, np.float32))
    rs = dgr.GaussianRasterizationSettings(
        image_height=sc.H, image_width=sc.W, tanfovx=sc.tanfovx, tanfovy=sc.tanfovy, bg=t(sc.bg), scale_modifier=sc.scale_modifier,
        viewmatrix=t(sc.viewmatrix), projmatrix=t(sc.projmatrix), inv_viewprojmatrix=t(sc.inv_viewprojmatrix), sh_degree=sc.sh_degree,
        campos=t(sc.campos), prefiltered=False, settings=dgr.ExtendedSettings.from_dict(settings_dict(**FULL_STP)), render_depth=False,
        debug=False)
    m = t(sc.means3D)
    r = tile_shard.TileRowShardedRasterizer(rs, None, 0, 1) if sharded else dgr.GaussianRasterizer(rs)
    return r(m, torch.zeros_like(m), t(sc.opacities), shs=rest, colors_precomp=colors, scales=t(sc.scales), rotations=t(sc.rotations), dc=dc)


def test_refusals_are_raised_before_any_device_work():
    import torch
    sc = tiny()
    P = len(sc.means3D)
    shs = torch.tensor(np.asarray(sc.shs, np.float32))
    dc, rest = shs[:, :1].contiguous(), shs[:, 1:].contiguous()
    with pytest.raises(Exception, match=r"excatly one of either SHs or precomputed colors"):
        _cpu_call(sc, dc, None, colors=torch.rand(P, 3))
    with pytest.raises(Exception, match=r"excatly one of either SHs or precomputed colors"):
        _cpu_call(sc, dc, rest, colors=torch.rand(P, 3))
    with pytest.raises(RuntimeError, match=r"\bdc must have dimensions \(num_points, 1, 3\) or \(num_points, 3\)"):
        _cpu_call(sc, shs[:, :2].contiguous(), rest)      # (P, 2, 3)
    with pytest.raises(RuntimeError, match=r"\bdc must have dimensions"):
        _cpu_call(sc, dc.reshape(-1), rest)               # rank 1
    with pytest.raises(RuntimeError, match=r"\bdc must have dimensions"):
        _cpu_call(sc, dc.reshape(P, 1, 1, 3), rest)       # rank 4
    with pytest.raises(RuntimeError, match=rf"\bdc must have one row per Gaussian: {P - 1} rows for {P} points"):
        _cpu_call(sc, dc[1:].contiguous(), rest)
    with pytest.raises(RuntimeError, match=r"\bdc must be a float32 tensor, got torch.float64"):
        _cpu_call(sc, dc.double(), rest)
    with pytest.raises(RuntimeError, match=r"\bdc must be a float32 tensor, got torch.float16"):
        _cpu_call(sc, dc.half(), rest)
    with pytest.raises(RuntimeError, match=r"\bdc must be a tensor"):
        _cpu_call(sc, np.asarray(dc), rest)
    with pytest.raises(RuntimeError, match=r"with dc, shs is the rest"):
        _cpu_call(sc, dc, rest[1:].contiguous())
    with pytest.raises(RuntimeError, match=r"dc=.*not wired through the tile-row shard"):
        _cpu_call(sc, dc, rest, sharded=True)
    # a well-formed pair passes the checks and reaches the binding, which has no CPU path
    with pytest.raises(RuntimeError, match=r"no CPU path"):
        _cpu_call(sc, dc, rest)
    with pytest.raises(RuntimeError, match=r"no CPU path"):
        _cpu_call(sc, dc.reshape(P, 3), None)


def test_wrong_device_names_dc():
    """dc on another device than means3D: refused by the Python check, which compares devices without touching one (meta tensors stand in
    for the other device)."""
    import torch
    from diff_gaussian_rasterization import _check_split_sh
    m = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match=r"\bdc must be on the device of means3D \(cpu\), got meta"):
        _check_split_sh(torch.zeros(5, 3, device="meta"), None, m)
    _check_split_sh(torch.zeros(5, 1, 3), torch.zeros(5, 0, 3), m)   # (a degree-0 model: an empty rest is fine)
    _check_split_sh(torch.zeros(5, 3), None, m)


def test_dc_is_reachable_from_the_package():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    assert "dc" in inspect.signature(dgr.rasterize_gaussians).parameters
    assert "dc" in inspect.signature(_C.rasterize_gaussians).parameters and "dc" in inspect.signature(_C.rasterize_gaussians_backward).parameters
    assert set(SYMBOLS) <= set(_C._OPTIONAL_SYMBOLS)
