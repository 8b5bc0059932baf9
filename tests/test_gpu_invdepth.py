"""GPU tests (-m gpu) of the inverse-depth output (settings._invdepth; include/stp_raster.h: stp_set_forward_invdepth,
stp_set_backward_invdepth):  invdepth[p] = sum_i alpha_i T_i / z_i  over the pairs the colour blends, differentiable.

  1. against the float64 yardstick (torch_ref_invdepth.py): image, invdepth, every Gaussian gradient; the camera as leaves once;
  2. against the existing API, product against product: invdepth is color[0] of the product's own channel run (colors_precomp = (1/z, 0, 0),
     bg = 0), the depth-only gradients are that run's plus the float64 chain through 1/z -- also where the replay and the re-sorting
     backward share a frame's tiles;
  3. the request moves nothing else; exact zeros where nothing blended; the per-pixel extremes;
  4. together with camera gradients, absgrad and blend statistics;
  5. a tile-row window;  6. the path switches, in child processes;  7. P == 0, a culled frame, PPX_FULL, the refusals, the example.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from helpers import CAMERA, FULL_STP, _rel, _scene_a, _scene_b, api_settings, ext_settings, max_abs, settings_dict
from diff_gaussian_rasterization import scenes
import torch_ref
import torch_ref_invdepth as tri

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GAUSS = ("means3D", "means2D", "opacities", "scales", "rotations", "shs", "colors_precomp")

MODES = {   # settings, the float64 yardstick's order
    "global": (settings_dict(0), dict(order="global", depth_key="z")),
    "kbuffer16": (settings_dict(2, per_pixel=16), dict(order="exact")),
    "hier": (settings_dict(3), dict(order="exact")),
    "hier_full": (settings_dict(**FULL_STP), dict(order="exact")),
}
# (GLOBAL has one backward; the two per-pixel-sort modes replay the blend log or re-sort)
MODE_BACKWARD = [(m, b) for m in MODES for b in (("replay",) if m == "global" else ("replay", "resort"))]


def tiny(seed=7):
    return scenes.make_scene(P=150, W=40, H=36, sigma_min=1.0, sigma_max=8.0, seed=seed, camera="orbit")


def sparse():
    """20 tiles of which 1 (GLOBAL) or 3 (full culling) have empty lists, 2275 pixels with T == 1, a frame that is no multiple of 16"""
    return scenes.make_scene(P=25, W=72, H=56, sigma_min=1.0, sigma_max=4.0, seed=3, camera="orbit")


def saturating():
    """hundreds of pixels end below T = 2e-4: decisions on the threshold -- identities only, never the yardstick"""
    sc = scenes.make_scene(P=300, W=72, H=56, sigma_min=2.0, sigma_max=9.0, seed=7, camera="orbit")
    sc.opacities = sc.opacities.copy()
    sc.opacities[0::2] = 0.97
    return sc


def mixed_tiles():
    """tests/test_gpu_parity.py::test_blend_log_mixed_tiles' scene: some tiles overflow their blend log and are re-sorted, the others replay"""
    sc = scenes.make_scene(P=5000, W=96, H=64, sigma_min=3.0, sigma_max=16.0, seed=23, opacity_range=(0.01, 0.05))
    sc.opacities[sc.means3D[:, 0] > 0.0] = 0.6
    return sc


SCENES = {"tiny": tiny, "sparse": sparse, "a": _scene_a, "b": _scene_b, "saturating": saturating, "mixed": mixed_tiles}


def run(sc, sd, invdepth=False, alpha=False, w=None, wD=None, backward_mode=None, camera=(), absgrad=False, stats=False, tile_rows=None,
        backward=True, render_depth=False, only=None, bg=None):
    """One forward (+ backward) through the public API.  Loss: sum(w * color) (w: the scene's dL_dout; False: no colour term) +
    sum(wD * invdepth) (wD None: no inverse-depth term).  Returns color, radii, alpha, invdepth, final_T (H, W), ranges, tile_flags,
    grad_fn, every input's .grad under its name, and means2D's absgrad / blend_stats."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    dev = torch.device(DEV)
    t = lambda a, rg=False: None if a is None else torch.tensor(np.asarray(a, np.float32), device=dev).requires_grad_(rg)
    need = lambda n: backward and (only is None or n in only)
    ten = {n: t(getattr(sc, n), need(n)) for n in ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations")}
    ten["means2D"] = torch.zeros_like(ten["means3D"], requires_grad=need("means2D"))
    cam = {n: t(getattr(sc, n), n in camera) for n in CAMERA}
    d = dict(sd)
    if backward_mode:
        d["_backward_mode"] = backward_mode
    es = ext_settings(d)
    es._alpha, es._invdepth, es._absgrad, es._blend_stats = bool(alpha), bool(invdepth), bool(absgrad), bool(stats)
    if tile_rows is not None:   # (the tile-row window rides along in the dict through a private key, as for helpers.GpuRun)
        base = es.to_dict
        es.to_dict = lambda: {**base(), "_tile_rows": tuple(tile_rows)}
    rs = api_settings(sc, es, dev, render_depth, bg=t(sc.bg if bg is None else bg), **cam)
    res = dgr.GaussianRasterizer(rs)(ten["means3D"], ten["means2D"], ten["opacities"], shs=ten["shs"], colors_precomp=ten["colors_precomp"],
                                      scales=ten["scales"], rotations=ten["rotations"])
    assert len(res) == 2 + int(bool(alpha)) + int(bool(invdepth))   # (color, radii[, alpha][, invdepth])
    color, radii = res[0], res[1]
    fn = color.grad_fn
    out = {"color": color.detach(), "radii": radii, "alpha": res[2].detach() if alpha else None,
           "invdepth": res[-1].detach() if invdepth else None, "grad_fn": type(fn).__name__ if fn is not None else None}
    if invdepth:
        assert res[-1].shape == (1, sc.H, sc.W) and res[-1].dtype == torch.float32 and res[-1].grad_fn is fn
    if fn is not None and len(sc.means3D) > 0:
        img_buf = fn.saved_tensors[11]
        out["final_T"] = _C.image_array(img_buf, sc.W, sc.H, "final_T", tile_rows)[:sc.W * sc.H].clone()
        out["ranges"] = _C.image_array(img_buf, sc.W, sc.H, "ranges", tile_rows).clone().cpu().numpy().reshape(-1, 2)
        if d.get("_backward_mode") != "resort" and int(d["sort_settings"]["sort_mode"]) in (2, 3):
            out["tile_flags"] = _C.image_array(img_buf, sc.W, sc.H, "tile_flags", tile_rows).clone().cpu().numpy()
    if fn is not None and backward:
        loss = 0.0
        if w is not False:
            loss = loss + (color * torch.tensor(np.asarray(sc.dL_dout if w is None else w, np.float32), device=dev)).sum()
        if wD is not None:
            loss = loss + (res[-1] * torch.tensor(np.asarray(wD, np.float32), device=dev)).sum()
        loss.backward()
    for n, x in list(ten.items()) + list(cam.items()):
        out[n] = None if x is None or x.grad is None else x.grad.detach().clone()
    out["absgrad"], out["stats"] = getattr(ten["means2D"], "absgrad", None), getattr(ten["means2D"], "blend_stats", None)
    return out


def reference(scene_name, mode, camera_leaves=False):
    """The yardstick of (scene, order) with the case's w, wD; computed once and shared (read-only arrays)."""
    kw = MODES[mode][1]
    names = ("means3D", "means2D", "opacities", "scales", "rotations", "shs") + (CAMERA if camera_leaves else ())

    def make():
        sc = SCENES[scene_name]()
        w, wD = tri.weights(sc)
        r = tri.reference(sc, w, wD, camera_leaves=camera_leaves, **kw)
        return (r["image"], r["invdepth"], r["chain"][1]) + tuple(r["grads"][n] for n in names)
    out = torch_ref.cached("invdepth", (scene_name, tuple(sorted(kw.items())), camera_leaves), make)
    return dict(image=out[0], invdepth=out[1], chain_view=out[2], grads=dict(zip(names, out[3:])))


def check_grads(got, want, tol, names=GAUSS, label=""):
    """every gradient to tol of its tensor's largest entry; want: tensors or arrays by name"""
    for n in names:
        if want.get(n) is None:
            continue
        g, r = got[n].cpu().numpy(), want[n].cpu().numpy() if isinstance(want[n], torch.Tensor) else want[n]
        if n == "means2D":
            g, r = g[:, :2], r[:, :2]
        e = _rel(g, np.reshape(r, g.shape))
        print(f"  {label}{n}: rel {e:.2e}")
        assert e < tol, (label, n, e)


# ---- 1. against the yardstick -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["tiny", "sparse"])
@pytest.mark.parametrize("mode,backward_mode", MODE_BACKWARD)
def test_against_the_float64_yardstick(mode, backward_mode, scene):
    """_invdepth and _alpha together, random w and wD.  Image and invdepth 2e-6, gradients 5e-5 of the tensor's largest entry (the
    tolerances of tests/test_gpu_background.py and tests/test_gpu_camera_grad.py)."""
    sd = MODES[mode][0]
    sc = SCENES[scene]()
    w, wD = tri.weights(sc)
    ref = reference(scene, mode)
    got = run(sc, sd, invdepth=True, alpha=True, wD=wD, backward_mode=backward_mode)
    assert got["grad_fn"] == "_RasterizeGaussiansBackward"
    e_img, e_inv = max_abs(got["color"].cpu().numpy(), ref["image"]), max_abs(got["invdepth"][0].cpu().numpy(), ref["invdepth"])
    print(f"\n{mode} {backward_mode} {scene}: image {e_img:.2e} invdepth {e_inv:.2e}")
    assert e_img < 2e-6 and e_inv < 2e-6
    assert torch.equal(got["alpha"][0], 1.0 - got["final_T"].view(sc.H, sc.W))
    check_grads(got, ref["grads"], 5e-5)


@pytest.mark.parametrize("mode,backward_mode", [("global", "replay"), ("hier_full", "replay"), ("kbuffer16", "resort")])
def test_camera_as_leaves_carries_the_z_term(mode, backward_mode):
    """viewmatrix, projmatrix and campos as leaves on `tiny`: the path through z reaches viewmatrix.grad, which differs from the plain run's."""
    sd = MODES[mode][0]
    sc = tiny()
    w, wD = tri.weights(sc)
    ref = reference("tiny", mode, camera_leaves=True)
    got = run(sc, sd, invdepth=True, wD=wD, backward_mode=backward_mode, camera=CAMERA)
    assert got["grad_fn"] == "_RasterizeGaussiansCameraBackward"
    print(f"\n{mode} {backward_mode}")
    check_grads(got, ref["grads"], 5e-5, names=GAUSS + CAMERA)
    plain = run(sc, sd, backward_mode=backward_mode, camera=CAMERA)
    scale = float(np.max(np.abs(ref["grads"]["viewmatrix"])))
    assert float(np.max(np.abs(ref["chain_view"]))) > 1e-3 * scale   # the z term is a visible part of the yardstick's gradient ...
    assert max_abs(got["viewmatrix"].cpu().numpy(), plain["viewmatrix"].cpu().numpy()) > 1e-3 * scale   # ... and of the product's


# ---- 2. against the existing API, product against product -------------------------------------------------------------------------------
def channel_run(sc, sd, wD, backward_mode):
    """The product's own channel run: the same geometry with colors_precomp = (1/z, 0, 0) in float32, bg = 0 and dL_dout = (wD, 0, 0)."""
    ch = tri.channel_scene(sc, np.float32)
    w_c = np.zeros((3, sc.H, sc.W), np.float32)
    w_c[0] = wD
    return run(ch, sd, w=w_c, backward_mode=backward_mode)


@pytest.mark.parametrize("scene,mode,backward_mode", [(s, m, b) for s in ("a", "b", "saturating") for m, b in MODE_BACKWARD]
                         + [("mixed", "hier_full", "replay"), ("mixed", "kbuffer8", "replay")])
def test_against_the_products_own_channel_run(scene, mode, backward_mode):
    """invdepth == color[0] of the channel run to 2e-6; the depth-only gradients (w = False) are the channel run's plus the float64 chain of
    its colors_precomp.grad[:, 0] through 1/z, to 1e-5 of each tensor's largest entry; shs gets nothing.  On the mixed scene the replay
    and the re-sorting backward both write slot 14 of the records."""
    from diff_gaussian_rasterization import _C
    sd = settings_dict(2, per_pixel=8) if mode == "kbuffer8" else MODES[mode][0]
    sc = SCENES[scene]()
    wD = tri.weights(sc)[1]
    if scene == "mixed":
        _C.reset_size_guesses()   # (the log's depth is that of a frame nothing is known about: the deep half of the frame overflows it)
    got = run(sc, sd, invdepth=True, w=False, wD=wD, backward_mode=backward_mode)
    if scene == "mixed":
        flags = got["tile_flags"]
        assert flags.any() and not flags.all(), flags
        _C.reset_size_guesses()
    chan = channel_run(sc, sd, wD, backward_mode)
    assert torch.equal(chan["radii"], got["radii"])
    e_inv = max_abs(got["invdepth"][0].cpu().numpy(), chan["color"][0].cpu().numpy())
    print(f"\n{scene} {mode} {backward_mode}: invdepth against the channel run {e_inv:.2e}, max {float(got['invdepth'].max()):.3f}")
    assert e_inv < 2e-6
    gm, _ = tri.chain_through_c(sc, chan["colors_precomp"][:, 0].double().cpu().numpy())
    want = {n: chan[n].double().cpu().numpy() for n in ("means3D", "means2D", "opacities", "scales", "rotations")}
    assert float(np.max(np.abs(gm))) > 1e-3 * float(np.max(np.abs(want["means3D"] + gm)))   # (the z path counts)
    want["means3D"] = want["means3D"] + gm
    check_grads(got, want, 1e-5, names=("means3D", "means2D", "opacities", "scales", "rotations"))
    assert torch.all(got["shs"] == 0)   # the inverse depth does not depend on the colours


# ---- 3. nothing else moves --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["b", "sparse"])
@pytest.mark.parametrize("mode,backward_mode", MODE_BACKWARD)
def test_nothing_else_moves(mode, backward_mode, scene):
    """_invdepth (+ _alpha) with no loss on it: image, radii and alpha bit for bit, gradients to 1e-5 of a run without the request.
    invdepth is exactly 0 where nothing blended and in tiles with empty lists, and lies between the extremes of 1/z times alpha."""
    sd = MODES[mode][0]
    sc = SCENES[scene]()
    plain = run(sc, sd, alpha=True, backward_mode=backward_mode)
    got = run(sc, sd, invdepth=True, alpha=True, backward_mode=backward_mode)
    assert got["grad_fn"] == plain["grad_fn"] == "_RasterizeGaussiansBackward"
    assert torch.equal(got["color"], plain["color"]) and torch.equal(got["radii"], plain["radii"]) and torch.equal(got["alpha"], plain["alpha"])
    print(f"\n{mode} {backward_mode} {scene}")
    check_grads(got, plain, 1e-5)
    D, T = got["invdepth"][0], got["final_T"].view(sc.H, sc.W)
    assert torch.all(D[T == 1.0] == 0.0) and float(D.max()) > 0.0
    if scene == "sparse":
        assert int((T == 1.0).sum()) > 2000
        gx = (sc.W + 15) // 16
        empty_tiles = np.flatnonzero(got["ranges"][:, 0] == got["ranges"][:, 1])
        assert len(empty_tiles) >= 1
        for tile in empty_tiles:
            ty, tx = divmod(int(tile), gx)
            assert torch.all(D[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] == 0.0)
    c = torch.tensor(tri.inv_z(sc, np.float32), device=DEV)[got["radii"] > 0]
    a = got["alpha"][0]
    assert torch.all(D >= float(c.min()) * a - 2e-6) and torch.all(D <= float(c.max()) * a + 2e-6)   # a wrong weight or a stray background term


# ---- 4. combined requests ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,backward_mode", [("global", "replay"), ("hier_full", "replay"), ("hier_full", "resort"), ("kbuffer16", "replay")])
def test_with_camera_gradients_absgrad_and_blend_stats(mode, backward_mode):
    """All four requests (+ alpha) in one backward: Gaussian and camera gradients against the yardstick with the camera as leaves; the
    blend statistics, which do not depend on the loss, are a plain run's, the count exactly; absgrad bounds |means2D.grad|."""
    sd = MODES[mode][0]
    sc = tiny()
    w, wD = tri.weights(sc)
    ref = reference("tiny", mode, camera_leaves=True)
    got = run(sc, sd, invdepth=True, alpha=True, wD=wD, backward_mode=backward_mode, camera=CAMERA, absgrad=True, stats=True)
    assert max_abs(got["color"].cpu().numpy(), ref["image"]) < 2e-6 and max_abs(got["invdepth"][0].cpu().numpy(), ref["invdepth"]) < 2e-6
    print(f"\n{mode} {backward_mode}")
    check_grads(got, ref["grads"], 5e-5, names=GAUSS + CAMERA)
    plain = run(sc, sd, backward_mode=backward_mode, stats=True)
    assert torch.equal(got["stats"][:, 2], plain["stats"][:, 2]) and _rel(got["stats"].cpu().numpy(), plain["stats"].cpu().numpy()) < 1e-5
    assert got["absgrad"].shape == (len(sc.means3D), 3) and torch.isfinite(got["absgrad"]).all()
    assert torch.all(got["absgrad"][:, :2] >= got["means2D"][:, :2].abs() - 1e-5 * got["absgrad"].max())


# ---- 5. tile-row window -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,backward_mode", [("global", "replay"), ("hier_full", "replay"), ("kbuffer16", "resort")])
def test_tile_row_window(mode, backward_mode):
    """A frame of four tile rows rendered for rows [1, 3): inside, image and invdepth are the full frame's bit for bit; outside, nothing is
    written (the zero-filled outputs stand).  The backward reads the window's rows of the two full-frame buffers."""
    sd = MODES[mode][0]
    sc = sparse()
    w, wD = tri.weights(sc)
    full = run(sc, sd, invdepth=True, wD=wD, backward_mode=backward_mode)
    part = run(sc, sd, invdepth=True, wD=wD, backward_mode=backward_mode, tile_rows=(1, 3))
    rows = slice(16, 48)
    for k in ("color", "invdepth"):
        assert torch.equal(part[k][:, rows], full[k][:, rows]), k
        assert torch.all(part[k][:, :16] == 0) and torch.all(part[k][:, 48:] == 0), k
    assert float(part["invdepth"].max()) > 0.0
    # the window's share of the loss: the full frame's gradient with the weights zeroed outside the window
    w_in, wD_in = np.zeros_like(w), np.zeros_like(wD)
    w_in[:, rows], wD_in[rows] = w[:, rows], wD[rows]
    want = run(sc, sd, invdepth=True, w=w_in, wD=wD_in, backward_mode=backward_mode)
    check_grads(part, want, 1e-5)


# ---- 6. path switches -------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys, numpy as np, torch
sys.path[:0] = ['tests', 'stopthepop-rasterization_amd', '.']
import conftest
from helpers import *
from diff_gaussian_rasterization import scenes, _C
import test_gpu_invdepth as tgi
out = {}
modes = dict(tgi.MODES, kbuffer8=(settings_dict(2, per_pixel=8), None))
for scene in ('b', 'sparse'):
    sc = tgi.SCENES[scene]()
    wD = tgi.tri.weights(sc)[1]
    for mode in ('kbuffer8', 'kbuffer16', 'hier', 'hier_full'):
        for bm in ('replay', 'resort'):
            # (an input that requires grad: the forward of 'replay' is the RECORDING forward, the training path; 'resort' the plain one)
            r = tgi.run(sc, modes[mode][0], invdepth=True, wD=wD, backward_mode=bm, only=('opacities',))
            recorded = bool((r['tile_flags'] != -1).all()) if 'tile_flags' in r else False
            assert recorded == (bm == 'replay'), (scene, mode, bm, r.get('tile_flags'))
            out[f'{scene}/{mode}/{bm}/invdepth'] = r['invdepth'].cpu().numpy()
            out[f'{scene}/{mode}/{bm}/color'] = r['color'].cpu().numpy()
            out[f'{scene}/{mode}/{bm}/g_opacities'] = r['opacities'].cpu().numpy()
np.savez(sys.argv[1], **out)
"""
_children = {}


def child(env):
    """invdepth, colour and dL/dopacities (a loss on colour and inverse depth) of two scenes in the per-pixel-sort modes, from the plain
    forward + re-sorting backward and from the recording forward + replay, in a fresh process under `env`"""
    key = tuple(sorted(env.items()))
    if key not in _children:
        with tempfile.TemporaryDirectory() as d:
            f = os.path.join(d, "o.npz")
            subprocess.run([sys.executable, "-c", CHILD, f], check=True, timeout=300, env=dict(os.environ, **env), cwd=ROOT)
            _children[key] = dict(np.load(f))
    return _children[key]


@pytest.mark.parametrize("switch", ["STP_KBUFFER=tile", "STP_KBUFFER=wave", "STP_FUSED_GATHER=0", "STP_SORT=radix", "STP_TILE_SORT=rocprim"])
def test_path_switches_change_no_bit(switch):
    """The switches are read once per process: children.  Plain AND recording forwards (the child asserts that 'replay' recorded a blend
    log and 'resort' did not): invdepth is the default paths' bit for bit (and so is the image, wherever the switch leaves the render kernel
    alone: the one-entry-per-wave k-buffer kernel forms its colour products in another order); the gradient of a loss on both, through the
    replay of that log or the re-sort, to the summation order of the atomics (2e-5, tests/test_gpu_fused_gather.py's bound)."""
    name, value = switch.split("=")
    a, b = child({}), child({name: value})
    assert set(a) == set(b) and len(a) == 48
    for k in a:
        if k.endswith("g_opacities"):
            assert float(np.abs(a[k]).max()) > 0.0 and _rel(b[k], a[k]) < 2e-5, (switch, k, _rel(b[k], a[k]))
            continue
        if k.endswith("invdepth"):
            assert float(a[k].max()) > 0.01
        elif switch == "STP_KBUFFER=tile":
            continue
        assert np.array_equal(a[k], b[k]), (switch, k)


# ---- 6b. the other queue sizes' instantiations ------------------------------------------------------------------------------------------
OTHER_SIZES = {   # every k-buffer window of the ladder but 8 and 16; hierarchical heads 8 / 16 and mids 12 / 20 (head 12 has no forward)
    **{f"kbuffer{w}": settings_dict(2, per_pixel=w) for w in (1, 2, 4, 12, 20, 24)},
    "hier_h8_m12": settings_dict(**{**FULL_STP, "per_pixel": 8, "tile_2x2": 12}),
    "hier_h16_m20": settings_dict(**{**FULL_STP, "per_pixel": 16, "tile_2x2": 20}),
    "hier_h8_m8_nocull": settings_dict(3, per_pixel=8),
    "hier_h4_m12": settings_dict(3, per_pixel=4, tile_2x2=12),
}


@pytest.mark.parametrize("backward_mode", ["replay", "resort"])
@pytest.mark.parametrize("sizes", list(OTHER_SIZES))
def test_other_queue_sizes_against_the_channel_run(sizes, backward_mode):
    """The variants of the queue sizes the other tests do not select, product against product on `_scene_a`: invdepth is the channel
    run's color[0] (2e-6), the depth-only gradients the channel run's plus the chain through 1/z (1e-5)."""
    sd = OTHER_SIZES[sizes]
    sc = _scene_a()
    wD = tri.weights(sc)[1]
    got = run(sc, sd, invdepth=True, w=False, wD=wD, backward_mode=backward_mode)
    chan = channel_run(sc, sd, wD, backward_mode)
    assert max_abs(got["invdepth"][0].cpu().numpy(), chan["color"][0].cpu().numpy()) < 2e-6 and float(got["invdepth"].max()) > 0.01
    gm, _ = tri.chain_through_c(sc, chan["colors_precomp"][:, 0].double().cpu().numpy())
    want = {n: chan[n].double().cpu().numpy() for n in ("means3D", "means2D", "opacities", "scales", "rotations")}
    want["means3D"] = want["means3D"] + gm
    print(f"\n{sizes} {backward_mode}")
    check_grads(got, want, 1e-5, names=("means3D", "means2D", "opacities", "scales", "rotations"))


# ---- 7. edge cases, refusals, the example -----------------------------------------------------------------------------------------------
def test_empty_and_culled_frames():
    empty = scenes.make_scene(P=1, W=48, H=40, sigma_min=1.0, sigma_max=2.0, seed=1, camera="orbit")
    for f in ("means3D", "scales", "rotations", "opacities", "shs"):
        setattr(empty, f, getattr(empty, f)[:0])
    wD = np.ones((empty.H, empty.W), np.float32)
    got = run(empty, settings_dict(**FULL_STP), invdepth=True, alpha=True, wD=wD, only=("opacities", "means2D"))   # P == 0: nothing is launched
    assert torch.all(got["color"] == 0) and torch.all(got["invdepth"] == 0) and got["invdepth"].shape == (1, empty.H, empty.W)
    behind = scenes.make_scene(P=200, W=48, H=40, sigma_min=1.0, sigma_max=8.0, seed=7)   # camera at the origin looking down +z
    behind.means3D = (behind.means3D * np.array([1, 1, -1], np.float32)).astype(np.float32)
    for sd in (settings_dict(0), settings_dict(2, per_pixel=16), settings_dict(**FULL_STP)):   # everything culled: zeros
        got = run(behind, sd, invdepth=True, wD=wD)
        assert torch.all(got["radii"] == 0) and torch.all(got["invdepth"] == 0)
        assert torch.all(got["means3D"] == 0) and torch.all(got["opacities"] == 0)


def test_full_sort_forward_only_and_refusals():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import tile_shard
    sc = tiny()
    sd = settings_dict(**FULL_STP)
    # PPX_FULL: forward only, as without the request; its invdepth is the k-buffer's of a window that holds the whole list, to rounding
    got = run(sc, settings_dict(1), invdepth=True, backward=False)
    assert torch.isfinite(got["invdepth"]).all() and float(got["invdepth"].max()) > 0.01
    c = tri.inv_z(sc, np.float32)
    assert float(got["invdepth"].max()) <= float(c.max()) + 2e-6
    with pytest.raises(RuntimeError, match=r"[Bb]ackward not supported"):
        run(sc, settings_dict(1), invdepth=True, wD=np.ones((sc.H, sc.W), np.float32))
    with pytest.raises(RuntimeError, match=r"inverse-depth output.*_invdepth.*render_depth=True"):
        run(sc, sd, invdepth=True, render_depth=True, backward=False)
    # the refused forward left no request behind: the next plain forward is the plain image, and a render_depth one runs
    plain = run(sc, sd, backward=False)
    assert plain["invdepth"] is None and torch.isfinite(plain["color"]).all()
    assert torch.equal(plain["color"], run(sc, sd, invdepth=True, backward=False)["color"])
    assert torch.isfinite(run(sc, sd, render_depth=True, backward=False)["color"]).all()
    dev = torch.device(DEV)
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    m = t(sc.means3D).requires_grad_(True)
    es = ext_settings(sd)
    es._invdepth = True
    with pytest.raises(RuntimeError, match=r"inverse-depth output.*_invdepth.*tile-row sharding.*not exchanged"):
        tile_shard.TileRowShardedRasterizer(api_settings(sc, es, dev), None, 0, 1)(m, torch.zeros_like(m), t(sc.opacities), shs=t(sc.shs),
                                                                                   scales=t(sc.scales), rotations=t(sc.rotations))


def test_backward_through_the_binding():
    """Through _C: the two tensors of the backward, no extra result; a half on its own is refused by the binding."""
    from diff_gaussian_rasterization import _C
    sc = tiny()
    sd = {**settings_dict(**FULL_STP), "_backward_mode": "resort"}
    dev = torch.device(DEV)
    empty = torch.Tensor([])
    t = lambda a: empty if a is None else torch.tensor(np.asarray(a, np.float32), device=dev)
    ten = dict(bg=t(sc.bg), m=t(sc.means3D), op=t(sc.opacities), sc=t(sc.scales), ro=t(sc.rotations), vm=t(sc.viewmatrix), pm=t(sc.projmatrix),
               inv=t(sc.inv_viewprojmatrix), sh=t(sc.shs), cam=t(sc.campos))
    R, color, radii, geom, binning, img, inv = _C.rasterize_gaussians(
        ten["bg"], ten["m"], empty, ten["op"], ten["sc"], ten["ro"], sc.scale_modifier, empty, ten["vm"], ten["pm"], ten["inv"], sc.tanfovx,
        sc.tanfovy, sc.H, sc.W, ten["sh"], sc.sh_degree, ten["cam"], False, sd, False, False, invdepth=True)
    assert inv.shape == (1, sc.H, sc.W)
    args = (ten["bg"], ten["m"], radii, ten["op"], empty, ten["sc"], ten["ro"], sc.scale_modifier, empty, ten["vm"], ten["pm"], ten["inv"],
            sc.tanfovx, sc.tanfovy, color, torch.zeros_like(color), ten["sh"], sc.sh_degree, ten["cam"], geom, R, binning, img, sd, False)
    dD = torch.ones_like(inv)
    whole = _C.rasterize_gaussians_backward(*args, dL_dinvdepth=dD, invdepth=inv)
    assert len(whole) == 8 and float(whole[3].abs().max()) > 0.0   # (dL_dmeans3D)
    with pytest.raises(RuntimeError, match=r"both halves"):
        _C.rasterize_gaussians_backward(*args, phases=1, dL_dinvdepth=dD, invdepth=inv)
    # (the refused call consumed the request: a plain backward behind it is the plain one; tests/test_invdepth_cpu.py has the C ABI's own refusals)
    plain = _C.rasterize_gaussians_backward(*args)
    assert all(float(g.abs().max()) == 0.0 for g in plain if g.numel())


def test_trainer_example_with_a_depth_term():
    """examples/train_render.py --depth-weight: render() hands the inverse depth out, the 25-iteration fit takes an L1 term on it and
    still descends (the bound of the mask term's test)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_render", os.path.join(ROOT, "examples", "train_render.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    first, last = mod.main(["--iters", "25", "--config", "full", "--points", "4000", "--size", "160", "112", "--depth-weight", "0.5"])
    assert last < 0.6 * first, (first, last)
    dev = torch.device(DEV)
    sc = sparse()
    cfg = mod.splat_config("full")
    cfg._alpha = cfg._invdepth = True
    with torch.no_grad():
        out = mod.render(mod.camera_of(sc, dev), mod.ToyGaussians(sc, dev), torch.tensor(sc.bg, device=dev), cfg)
    assert out["alpha"].shape == out["invdepth"].shape == (1, sc.H, sc.W)
    assert torch.all(out["invdepth"][out["alpha"] == 0] == 0)
