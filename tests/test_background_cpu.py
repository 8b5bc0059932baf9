"""CPU tests of the alpha output / per-pixel background / background gradient extension (settings._alpha, a (3, H, W) bg, a bg that
requires grad; include/stp_raster.h: stp_set_forward_background, stp_set_backward_background): the settings dict, the C ABI's
declarations and exports, the loader's message for a library without the symbols, and the float64 yardstick of the GPU tests
(torch_ref_background.py) held against the CPU oracle decomposed the same way."""
import os
import re
import types

import numpy as np
import pytest

from helpers import FULL_STP, _rel, max_abs, settings_dict
from diff_gaussian_rasterization import scenes
from oracle import oracle as orc
import torch_ref_background as trb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# settings, the float64 yardstick's order (as tests/test_gpu_camera_grad.py maps them)
MODES = {
    "global": (settings_dict(0), dict(order="global", depth_key="z")),
    "kbuffer16": (settings_dict(2, per_pixel=16), dict(order="exact")),
    "hier": (settings_dict(3), dict(order="exact")),
    "hier_full": (settings_dict(**FULL_STP), dict(order="exact")),
}


def tiny(seed=7, camera="orbit"):
    return scenes.make_scene(P=150, W=40, H=36, sigma_min=1.0, sigma_max=8.0, seed=seed, camera=camera)


def sparse():
    """20 tiles, some with empty lists, more than half of the pixels untouched (T == 1), a frame that is no multiple of 16"""
    return scenes.make_scene(P=25, W=72, H=56, sigma_min=1.0, sigma_max=4.0, seed=3, camera="orbit")


SCENES = {"seed7_orbit": lambda: tiny(7, "orbit"), "seed7_origin": lambda: tiny(7, "origin"), "seed11_orbit": lambda: tiny(11, "orbit"),
          "sparse": sparse}


def test_alpha_rides_in_the_settings_dict():
    import diff_gaussian_rasterization as dgr
    es = dgr.ExtendedSettings.from_dict(settings_dict(3, h44=True))
    assert "_alpha" not in es.to_dict()
    es._alpha = False   # (switched off: no key)
    assert es.to_dict() == settings_dict(3, h44=True)
    es._alpha = True
    assert es.to_dict() == {**settings_dict(3, h44=True), "_alpha": True}
    es._absgrad = True   # (requests of their own: both ride)
    assert es.to_dict() == {**settings_dict(3, h44=True), "_absgrad": True, "_alpha": True}
    assert "_alpha" not in {f for f in es.__dataclass_fields__}   # an extension attribute, not a field of the reference's dataclass


def test_header_declares_the_two_setters():
    h = open(os.path.join(ROOT, "include", "stp_raster.h")).read()
    assert int(re.search(r"#define\s+STP_ABI_VERSION\s+(\d+)\b", h).group(1)) == 7
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)   # (the declarations carry their shapes as comments)
    assert re.search(r"void\s+stp_set_forward_background\s*\(\s*const\s+float\s*\*\s*bg_image[^,]*,\s*float\s*\*\s*out_alpha[^)]*\)\s*;", h)
    assert re.search(r"void\s+stp_set_backward_background\s*\(\s*const\s+float\s*\*\s*bg_image[^,]*,\s*const\s+float\s*\*\s*dL_dalpha[^,]*,"
                     r"\s*float\s*\*\s*dL_dbackground[^)]*\)\s*;", h)
    hpp = open(os.path.join(ROOT, "include", "stp_rasterizer.hpp")).read()   # trailing, defaulted arguments on the C++ face
    assert re.search(r"bool\s+recordBlendLog\s*=\s*false,\s*const\s+float\*\s*bg_image\s*=\s*nullptr,\s*float\*\s*out_alpha\s*=\s*nullptr\)", hpp)
    # (backward() keeps its pinned argument list and stays one function: the background arguments trail those of backwardWithBackground())
    assert re.search(r"void\s+backwardWithBackground\(", hpp)
    assert re.search(r"float\*\s*blend_stats\s*=\s*nullptr,\s*const\s+float\*\s*bg_image\s*=\s*nullptr,\s*const\s+float\*\s*dL_dalpha\s*=\s*nullptr,"
                     r"\s*float\*\s*dL_dbackground\s*=\s*nullptr\)", hpp)


def test_library_exports_the_two_setters():
    from diff_gaussian_rasterization import _C
    L = _C._load()
    assert hasattr(L, "stp_set_forward_background") and hasattr(L, "stp_set_backward_background")
    assert _C._require("stp_set_forward_background") is not None and _C._require("stp_set_backward_background") is not None
    # NULL pointers only clear the (thread-local) requests: callable without a GPU
    L.stp_set_forward_background(None, None)
    L.stp_set_backward_background(None, None, None)
    assert L.stp_abi_version() == 7


@pytest.mark.parametrize("name", ["stp_set_forward_background", "stp_set_backward_background"])
def test_loader_message_for_a_library_without_the_symbols(monkeypatch, name):
    from diff_gaussian_rasterization import _C
    monkeypatch.setattr(_C, "_lib", types.SimpleNamespace())   # a loaded library that predates the exports
    with pytest.raises(RuntimeError) as ex:
        _C._require(name)
    assert str(ex.value) == (f"{_C.library_path()} does not export {name} (a library built before the alpha output and per-pixel "
                             "background): rebuild it")


def oracle_decomposed(sc, sd, B, w, wA):
    """torch_ref_background's decomposition on the CPU oracle (float32): two forwards, bg = 0 and bg = e0, and their backwards."""
    frames = [orc.forward_scene(trb.with_bg(sc, bg), sd) for bg in (np.zeros(3, np.float32), trb.E0)]
    grads = lambda which, dL: frames[which].backward(dL.astype(np.float32))
    return trb.decompose(frames[0].color, frames[1].color, grads, B, w, wA, dtype=np.float32)


ORACLE_NAMES = (("dL_dmeans3D", "means3D"), ("dL_dopacity", "opacities"), ("dL_dscales", "scales"), ("dL_drotations", "rotations"),
                ("dL_dsh", "shs"))


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("mode", list(MODES))
def test_yardstick_holds_against_the_cpu_oracle(mode, scene):
    """Image and alpha to 2e-6, every gradient to 5e-5 of its tensor's largest entry, dL/dB to 2e-6 of |w|'s largest: the tolerances of
    tests/test_oracle_cpu.py and tests/test_gpu_camera_grad.py.  Measured worst: image 5.0e-7, alpha 8.6e-7, gradients 1.0e-5."""
    sd, ref_kw = MODES[mode]
    sc = SCENES[scene]()
    B, w, wA = trb.weights(sc)
    ref = trb.reference(sc, B, w, wA, **ref_kw)
    got = oracle_decomposed(sc, sd, B, w, wA)
    e_img, e_alpha = max_abs(got["image"], ref["image"]), max_abs(got["alpha"], ref["alpha"])
    print(f"\n{mode} {scene}: image {e_img:.2e} alpha {e_alpha:.2e}")
    assert e_img < 2e-6 and e_alpha < 2e-6
    assert np.all(ref["alpha"] >= -1e-15) and np.all(ref["alpha"] <= 1.0)
    for o_name, r_name in ORACLE_NAMES:
        r = _rel(got["grads"][o_name], ref["grads"][r_name])
        print(f"  {r_name}: rel {r:.2e}")
        assert r < 5e-5, (r_name, r)
    assert _rel(got["grads"]["dL_dmeans2D"][:, :2], ref["grads"]["means2D"]) < 5e-5
    assert max_abs(got["dB"], ref["dB"]) < 2e-6 * float(np.max(np.abs(w)))
    assert _rel(got["dbg"], ref["dbg"]) < 5e-5


def test_yardstick_uniform_background_is_render_cores_own():
    """With a uniform colour the decomposition gives back render_core's image and gradients for that bg (1e-12): it is linear in bg."""
    import torch_ref
    sc = tiny()
    w = np.asarray(sc.dL_dout, np.float64)
    ref = trb.reference(sc, np.asarray(sc.bg, np.float64), w, np.zeros((sc.H, sc.W)), order="exact")
    img, g = torch_ref.loss_and_grads(sc, order="exact")
    assert max_abs(ref["image"], img) < 1e-12
    for n in ("means3D", "opacities", "scales", "rotations", "shs", "means2D"):
        assert _rel(ref["grads"][n], g[n]) < 1e-10, n


def test_sparse_scene_is_what_the_gpu_tests_count_on():
    """Tiles with empty lists, thousands of untouched pixels: where a forward writes the background alone and alpha must be exactly 0."""
    sc = sparse()
    for sd, empty_tiles in ((settings_dict(0), 1), (settings_dict(**FULL_STP), 3)):
        f = orc.forward_scene(sc, sd)
        ranges = f.array("ranges").reshape(-1, 2)
        assert len(ranges) == 20 and int(np.sum(ranges[:, 0] == ranges[:, 1])) == empty_tiles
        assert int(np.sum(f.array("final_T")[:sc.W * sc.H] == 1.0)) == 2275
