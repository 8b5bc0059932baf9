"""CPU tests of the inverse-depth output (settings._invdepth; include/stp_raster.h: stp_set_forward_invdepth, stp_set_backward_invdepth):
the float64 yardstick of the GPU tests (torch_ref_invdepth.py) held against the CPU oracle's channel run, the settings dict, the C ABI's
declarations and exports, and the refusals that are raised before any device work."""
import os
import re
import types

import numpy as np
import pytest

from helpers import FULL_STP, _rel, max_abs, settings_dict
from diff_gaussian_rasterization import scenes
from oracle import oracle as orc
import torch_ref_invdepth as tri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODES = {   # settings, the float64 yardstick's order
    "global": (settings_dict(0), dict(order="global", depth_key="z")),
    "kbuffer16": (settings_dict(2, per_pixel=16), dict(order="exact")),
    "hier_full": (settings_dict(**FULL_STP), dict(order="exact")),
}


def tiny():
    return scenes.make_scene(P=150, W=40, H=36, sigma_min=1.0, sigma_max=8.0, seed=7, camera="orbit")


def sparse():
    """20 tiles, some with empty lists, more than half of the pixels untouched, a frame that is no multiple of 16"""
    return scenes.make_scene(P=25, W=72, H=56, sigma_min=1.0, sigma_max=4.0, seed=3, camera="orbit")


SCENES = {"tiny": tiny, "sparse": sparse}
ORACLE_NAMES = (("dL_dmeans3D", "means3D"), ("dL_dopacity", "opacities"), ("dL_dscales", "scales"), ("dL_drotations", "rotations"),
                ("dL_dsh", "shs"), ("dL_dcolors", "colors_precomp"))


def oracle_decomposed(sc, sd, w, wD):
    """torch_ref_invdepth's decomposition on the CPU oracle (float32): the scene's forward and its channel run's, and their backwards."""
    frames = [orc.forward_scene(s, sd) for s in (sc, tri.channel_scene(sc, np.float32))]

    def grads_of(k):
        def grads(dL):
            g = frames[k].backward(np.asarray(dL, np.float32))
            out = {r: g[o] for o, r in ORACLE_NAMES}
            out["means2D"] = g["dL_dmeans2D"][:, :2]
            if k == 0:
                out["colors_precomp"] = None   # (the plain scene's colours come from its SH)
            else:
                out["shs"] = None
            return out
        return grads

    return tri.decompose(sc, frames[0].color, frames[1].color, grads_of(0), grads_of(1), w, wD, dtype=np.float32)


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("mode", list(MODES))
def test_yardstick_holds_against_the_cpu_oracle(mode, scene):
    """The float32 oracle's channel run against the float64 yardstick: invdepth to 2e-6 absolute, every gradient to 5e-5 of its tensor's
    largest entry (the tolerances of tests/test_oracle_cpu.py and tests/test_background_cpu.py).  1 / z stays below 0.5 on these scenes."""
    sd, ref_kw = MODES[mode]
    sc = SCENES[scene]()
    w, wD = tri.weights(sc)
    assert 0.0 < float(tri.inv_z(sc).max()) < 0.5
    ref = tri.reference(sc, w, wD, **ref_kw)
    got = oracle_decomposed(sc, sd, w, wD)
    e_img, e_inv = max_abs(got["image"], ref["image"]), max_abs(got["invdepth"], ref["invdepth"])
    print(f"\n{mode} {scene}: image {e_img:.2e} invdepth {e_inv:.2e}")
    assert e_img < 2e-6 and e_inv < 2e-6
    assert float(np.max(ref["invdepth"])) > 0.01 and float(np.min(ref["invdepth"])) >= 0.0
    for n in ("means3D", "means2D", "opacities", "scales", "rotations", "shs"):
        r = _rel(got["grads"][n], ref["grads"][n])
        print(f"  {n}: rel {r:.2e}")
        assert r < 5e-5, (n, r)
    # the path through z is a part of dL/dmeans3D that counts: without it the gradient is off by far more than the tolerance
    assert _rel(ref["grads"]["means3D"] - ref["chain"][0], ref["grads"]["means3D"]) > 1e-3


def test_yardstick_without_a_depth_term_is_render_cores_own():
    import torch_ref
    sc = tiny()
    w = np.asarray(sc.dL_dout, np.float64)
    ref = tri.reference(sc, w, np.zeros((sc.H, sc.W)), order="exact")
    img, g = torch_ref.loss_and_grads(sc, order="exact")
    assert max_abs(ref["image"], img) < 1e-12
    for n in ("means3D", "opacities", "scales", "rotations", "shs", "means2D"):
        assert _rel(ref["grads"][n], g[n]) < 1e-10, n


def test_invdepth_rides_in_the_settings_dict():
    import diff_gaussian_rasterization as dgr
    es = dgr.ExtendedSettings.from_dict(settings_dict(3, h44=True))
    assert "_invdepth" not in es.to_dict()
    es._invdepth = False   # (switched off: no key)
    assert es.to_dict() == settings_dict(3, h44=True)
    es._invdepth = True
    assert es.to_dict() == {**settings_dict(3, h44=True), "_invdepth": True}
    es._alpha = True   # (requests of their own: both ride)
    assert es.to_dict() == {**settings_dict(3, h44=True), "_alpha": True, "_invdepth": True}
    assert "_invdepth" not in {f for f in es.__dataclass_fields__}   # an extension attribute, not a field of the reference's dataclass


def test_header_declares_the_setters_and_the_slot():
    h = open(os.path.join(ROOT, "include", "stp_raster.h")).read()
    assert int(re.search(r"#define\s+STP_GRAD_RECORD_INVDEPTH\s+(\d+)\b", h).group(1)) == 14
    assert int(re.search(r"#define\s+STP_GRAD_RECORD_FLOATS\s+(\d+)\b", h).group(1)) == 16   # (slot 14 exists in the padded record only)
    assert int(re.search(r"#define\s+STP_GRAD_RECORD_USED\s+(\d+)\b", h).group(1)) == 9
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)   # (the declarations carry their shapes as comments)
    assert re.search(r"void\s+stp_set_forward_invdepth\s*\(\s*float\s*\*\s*out_invdepth[^)]*\)\s*;", h)
    assert re.search(r"void\s+stp_set_backward_invdepth\s*\(\s*const\s+float\s*\*\s*invdepth[^,]*,\s*const\s+float\s*\*\s*dL_dinvdepth[^)]*\)\s*;", h)


def test_library_exports_the_setters():
    import ctypes
    from diff_gaussian_rasterization import _C
    L = _C._load()
    assert hasattr(L, "stp_set_forward_invdepth") and hasattr(L, "stp_set_backward_invdepth")
    assert _C._require("stp_set_forward_invdepth") is not None and _C._require("stp_set_backward_invdepth") is not None
    # NULL pointers only clear the (thread-local) requests: callable without a GPU
    L.stp_set_forward_invdepth(None)
    L.stp_set_backward_invdepth(None, None)
    # the geometry buffer keeps 1 / z per Gaussian behind everything else: P floats under the name "invz"
    s = _C.settings_from_dict(settings_dict(**FULL_STP))
    off, cnt, off2, cnt2 = (ctypes.c_size_t() for _ in range(4))
    assert L.stp_geometry_layout(1000, ctypes.byref(s), b"invz", ctypes.byref(off), ctypes.byref(cnt)) == 0 and cnt.value == 1000
    assert L.stp_geometry_layout(1000, ctypes.byref(s), b"point_offsets", ctypes.byref(off2), ctypes.byref(cnt2)) == 0
    assert off.value > off2.value and off.value + 4 * 1000 <= L.stp_geometry_buffer_size(1000, ctypes.byref(s))


@pytest.mark.parametrize("name", ["stp_set_forward_invdepth", "stp_set_backward_invdepth"])
def test_loader_message_for_a_library_without_the_symbols(monkeypatch, name):
    from diff_gaussian_rasterization import _C
    monkeypatch.setattr(_C, "_lib", types.SimpleNamespace())   # a loaded library that predates the exports
    with pytest.raises(RuntimeError) as ex:
        _C._require(name)
    assert str(ex.value) == f"{_C.library_path()} does not export {name} (a library built before the inverse-depth output): rebuild it"


def _cpu_call(sc, es, render_depth=False, sharded=False):
    """The public forward on CPU tensors: a refusal that needs no device is raised before the binding asks for a GPU tensor."""
    import torch
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import tile_shard
    t = lambda a: torch.tensor(np.asarray(a, np.float32))
    rs = dgr.GaussianRasterizationSettings(
        image_height=sc.H, image_width=sc.W, tanfovx=sc.tanfovx, tanfovy=sc.tanfovy, bg=t(sc.bg), scale_modifier=sc.scale_modifier,
        viewmatrix=t(sc.viewmatrix), projmatrix=t(sc.projmatrix), inv_viewprojmatrix=t(sc.inv_viewprojmatrix), sh_degree=sc.sh_degree,
        campos=t(sc.campos), prefiltered=False, settings=es, render_depth=render_depth, debug=False)
    m = t(sc.means3D)
    r = tile_shard.TileRowShardedRasterizer(rs, None, 0, 1) if sharded else dgr.GaussianRasterizer(rs)
    return r(m, torch.zeros_like(m), t(sc.opacities), shs=t(sc.shs), scales=t(sc.scales), rotations=t(sc.rotations))


def test_refusals_are_raised_before_any_device_work():
    import diff_gaussian_rasterization as dgr
    sc = tiny()
    es = dgr.ExtendedSettings.from_dict(settings_dict(**FULL_STP))
    es._invdepth = True
    with pytest.raises(RuntimeError, match=r"inverse-depth output.*_invdepth.*render_depth=True"):
        _cpu_call(sc, es, render_depth=True)
    with pytest.raises(RuntimeError, match=r"inverse-depth output.*_invdepth.*tile-row sharding.*not exchanged"):
        _cpu_call(sc, es, sharded=True)


def test_c_abi_refuses_compact_records_and_a_chunked_half():
    """stp_backward_phases with a pending request: compact records (phases bit 2) have no slot 14, a chunked per-Gaussian half is no
    whole half -- refused on the request itself, before any argument is read, and the request is consumed."""
    import ctypes
    from diff_gaussian_rasterization import _C
    L = _C._load()
    buf = (ctypes.c_float * 4)()
    call = lambda phases: L.stp_backward_phases(*([ctypes.c_int(phases)] + [ctypes.c_int(0)] * 4 + [None] * 35))
    for phases, text in ((3 | 4, "compact gradient records"), (2 | (2 << 8), "chunked per-Gaussian half")):
        L.stp_set_backward_invdepth(buf, buf)
        assert call(phases) < 0 and "inverse-depth" in L.stp_last_error().decode() and text in L.stp_last_error().decode()
        assert call(phases) < 0 and "inverse-depth" not in L.stp_last_error().decode()   # (consumed: the next call fails on its null settings)
    L.stp_set_backward_invdepth(buf, None)   # one pointer of the two
    assert call(3) < 0 and "must both be given" in L.stp_last_error().decode()
