"""GPU tests (-m gpu) of the alpha output, the per-pixel background and the background gradients (settings._alpha, a bg of shape
(3, H, W), a bg that requires grad; include/stp_raster.h: stp_set_forward_background, stp_set_backward_background).

  1. against the float64 yardstick (torch_ref_background.py): image, alpha, every Gaussian gradient, dL/dB and the uniform (3,) gradient;
  2. alpha == 1 - final_T bit for bit in every sort mode, PPX_FULL included; exactly 0 in empty tiles;
  3. a B filled with one colour is the uniform path: image bit for bit, gradients to 1e-5;
  4. the alpha gradient against the existing API's gradient of the same quantity, without cancellation;
  5. the request moves nothing else; the uniform background gradient is bit-reproducible;
  6. together with camera gradients, absgrad and blend statistics; a backward through alpha alone; P == 0, a culled frame, a tile-row
     window; the refusals.
"""
import numpy as np
import pytest
import torch

from helpers import CAMERA, FULL_STP, _rel, _scene_a, _scene_b, api_settings, ext_settings, max_abs, settings_dict
from diff_gaussian_rasterization import scenes
import torch_ref
import torch_ref_background as trb

pytestmark = pytest.mark.gpu

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
    """259 (GLOBAL) to 268 (full culling) pixels end below T = 2e-4: decisions on the threshold -- identities only, never the yardstick"""
    sc = scenes.make_scene(P=300, W=72, H=56, sigma_min=2.0, sigma_max=9.0, seed=7, camera="orbit")
    sc.opacities = sc.opacities.copy()
    sc.opacities[0::2] = 0.97
    return sc


SCENES = {"seed7": tiny, "sparse": sparse, "a": _scene_a, "b": _scene_b, "saturating": saturating}


def run(sc, sd, bg=None, bg_grad=False, alpha=False, w=None, wA=None, backward_mode=None, camera=(), absgrad=False, stats=False,
        tile_rows=None, backward=True, render_depth=False, only=None):
    """One forward (+ backward) through the public API.  bg: the background array, (3,) or (3, H, W) (None: the scene's); bg_grad: it
    requires grad; only: the Gaussian inputs that require grad (None: all).  Loss: sum(w * color) (w: the scene's dL_dout; False: no colour term) + sum(wA * alpha) (wA None: no alpha term).
    Returns color, radii, alpha, final_T (H, W), ranges, grad_fn, every input's .grad under its name, "bg" the background's, and
    means2D's absgrad / blend_stats."""
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
    es._alpha, es._absgrad, es._blend_stats = bool(alpha), bool(absgrad), bool(stats)
    if tile_rows is not None:   # (the tile-row window rides along in the dict through a private key, as for helpers.GpuRun)
        base = es.to_dict
        es.to_dict = lambda: {**base(), "_tile_rows": tuple(tile_rows)}
    bg_t = t(sc.bg if bg is None else bg, bg_grad)
    rs = api_settings(sc, es, dev, render_depth, bg=bg_t, **cam)
    res = dgr.GaussianRasterizer(rs)(ten["means3D"], ten["means2D"], ten["opacities"], shs=ten["shs"], colors_precomp=ten["colors_precomp"],
                                      scales=ten["scales"], rotations=ten["rotations"])
    assert len(res) == (3 if alpha else 2)
    color, radii = res[0], res[1]
    out = {"color": color.detach(), "radii": radii, "alpha": res[2].detach() if alpha else None}
    fn = color.grad_fn
    out["grad_fn"] = type(fn).__name__ if fn is not None else None
    if alpha:
        assert res[2].shape == (1, sc.H, sc.W) and res[2].dtype == torch.float32 and res[2].grad_fn is fn
    if fn is not None and len(sc.means3D) > 0:
        img_buf = fn.saved_tensors[11]
        out["final_T"] = _C.image_array(img_buf, sc.W, sc.H, "final_T", tile_rows)[:sc.W * sc.H].clone()
        out["ranges"] = _C.image_array(img_buf, sc.W, sc.H, "ranges", tile_rows).clone().cpu().numpy().reshape(-1, 2)
    if fn is not None and backward:
        loss = 0.0
        if w is not False:
            loss = loss + (color * torch.tensor(np.asarray(sc.dL_dout if w is None else w, np.float32), device=dev)).sum()
        if wA is not None:
            loss = loss + (res[2] * torch.tensor(np.asarray(wA, np.float32), device=dev)).sum()
        loss.backward()
    for n, x in list(ten.items()) + list(cam.items()) + [("bg", bg_t)]:
        out[n] = None if x is None or x.grad is None else x.grad.detach().clone()
    out["absgrad"], out["stats"] = getattr(ten["means2D"], "absgrad", None), getattr(ten["means2D"], "blend_stats", None)
    return out


def reference(scene_name, mode, camera_leaves=False):
    """The yardstick of (scene, order) with the case's B, w, wA; computed once and shared (read-only arrays)."""
    kw = MODES[mode][1]
    names = ("means3D", "means2D", "opacities", "scales", "rotations", "shs") + (CAMERA if camera_leaves else ())

    def make():
        sc = SCENES[scene_name]()
        B, w, wA = trb.weights(sc)
        r = trb.reference(sc, B, w, wA, camera_leaves=camera_leaves, **kw)
        return (r["image"], r["alpha"], r["dB"], r["dbg"]) + tuple(r["grads"][n] for n in names)
    out = torch_ref.cached("background", (scene_name, tuple(sorted(kw.items())), camera_leaves), make)
    return dict(image=out[0], alpha=out[1], dB=out[2], dbg=out[3], grads=dict(zip(names, out[4:])))


def check_gaussian_grads(got, want, tol, names=GAUSS, label=""):
    """every gradient to tol of its tensor's largest entry; want: tensors or arrays by name"""
    for n in names:
        if want.get(n) is None:
            continue
        g, r = got[n].cpu().numpy(), want[n].cpu().numpy() if isinstance(want[n], torch.Tensor) else want[n]
        if n == "means2D":
            g, r = g[:, :2], r[:, :2]
        e = _rel(g, r)
        print(f"  {label}{n}: rel {e:.2e}")
        assert e < tol, (label, n, e)


# ---- 1. against the yardstick -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["seed7", "sparse"])
@pytest.mark.parametrize("mode,backward_mode", MODE_BACKWARD)
def test_against_the_float64_yardstick(mode, backward_mode, scene):
    """_alpha + a random per-pixel B that requires grad + random alpha weights.  Image and alpha 2e-6, gradients 5e-5 of the tensor's
    largest entry (tests/test_gpu_camera_grad.py's tolerances).  dL/dB = T * w: T is within the alpha tolerance, so 2e-6 * max|w|.  The
    uniform (3,) gradient is a gradient like the others: 5e-5 of its largest entry."""
    sd = MODES[mode][0]
    sc = SCENES[scene]()
    B, w, wA = trb.weights(sc)
    ref = reference(scene, mode)
    got = run(sc, sd, bg=B, bg_grad=True, alpha=True, wA=wA, backward_mode=backward_mode)
    assert got["grad_fn"] == "_RasterizeGaussiansBackgroundBackward"
    e_img, e_alpha = max_abs(got["color"].cpu().numpy(), ref["image"]), max_abs(got["alpha"][0].cpu().numpy(), ref["alpha"])
    print(f"\n{mode} {backward_mode} {scene}: image {e_img:.2e} alpha {e_alpha:.2e}")
    assert e_img < 2e-6 and e_alpha < 2e-6
    check_gaussian_grads(got, ref["grads"], 5e-5)
    assert got["bg"].shape == (3, sc.H, sc.W) and got["bg"].dtype == torch.float32
    e_dB = max_abs(got["bg"].cpu().numpy(), ref["dB"])
    print(f"  dL/dB: abs {e_dB:.2e} (max |w| {np.max(np.abs(w)):.2f})")
    assert e_dB < 2e-6 * float(np.max(np.abs(w)))
    # the same frame over a uniform background that requires grad: the image's own yardstick is linear in bg
    uni = run(sc, sd, bg_grad=True, alpha=True, wA=wA, backward_mode=backward_mode)
    assert uni["bg"].shape == (3,) and uni["bg"].dtype == torch.float32
    assert torch.equal(uni["alpha"], got["alpha"])
    e_bg = _rel(uni["bg"].double().cpu().numpy(), ref["dbg"])
    print(f"  dL/dbg: rel {e_bg:.2e} of {ref['dbg']}")
    assert e_bg < 5e-5


# ---- 2. alpha is 1 - final_T ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["seed7", "sparse"])
@pytest.mark.parametrize("mode", list(MODES) + ["full"])
def test_alpha_is_one_minus_final_T_bit_for_bit(mode, scene):
    """Through _C directly (PPX_FULL has no backward, hence no graph to take the image buffer from), with a per-pixel background."""
    from diff_gaussian_rasterization import _C
    sd = settings_dict(1) if mode == "full" else MODES[mode][0]
    sc = SCENES[scene]()
    B = trb.weights(sc)[0]
    dev = torch.device(DEV)
    empty = torch.Tensor([])
    t = lambda a: empty if a is None else torch.tensor(np.asarray(a, np.float32), device=dev)
    common = (t(sc.means3D), t(sc.colors_precomp), t(sc.opacities), t(sc.scales), t(sc.rotations), sc.scale_modifier, empty, t(sc.viewmatrix),
              t(sc.projmatrix), t(sc.inv_viewprojmatrix), sc.tanfovx, sc.tanfovy, sc.H, sc.W, t(sc.shs), sc.sh_degree, t(sc.campos), False, sd,
              False, False)
    plain = _C.rasterize_gaussians(t(sc.bg), *common)
    assert len(plain) == 6
    out = _C.rasterize_gaussians(t(B), *common, alpha=True)
    assert len(out) == 7 and out[0] == plain[0] and torch.equal(out[2], plain[2])
    alpha, T = out[6], _C.image_array(out[5], sc.W, sc.H, "final_T")[:sc.W * sc.H].view(sc.H, sc.W)
    assert alpha.shape == (1, sc.H, sc.W) and alpha.dtype == torch.float32
    assert torch.equal(alpha[0], 1.0 - T)
    assert torch.all(alpha[0][T == 1.0] == 0.0) and float(alpha.min()) >= 0.0 and float(alpha.max()) <= 1.0
    untouched = (T == 1.0)
    if scene == "sparse":
        assert int(untouched.sum()) > 2000
    assert torch.equal(out[1][:, untouched], t(B)[:, untouched])   # nothing blended: the background itself
    # pixels of tiles with an empty list
    ranges = _C.image_array(out[5], sc.W, sc.H, "ranges").cpu().numpy().reshape(-1, 2)
    gx = (sc.W + 15) // 16
    empty_tiles = np.flatnonzero(ranges[:, 0] == ranges[:, 1])
    if scene == "sparse":
        assert len(empty_tiles) >= 1
    for tile in empty_tiles:
        ty, tx = divmod(int(tile), gx)
        assert torch.all(alpha[0, 16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] == 0.0)


# ---- 3. a uniform colour through the per-pixel path -------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["a", "b", "saturating"])
@pytest.mark.parametrize("mode,backward_mode", MODE_BACKWARD)
def test_uniform_colour_through_the_per_pixel_path(mode, backward_mode, scene):
    """B filled with bg: the image of the existing path bit for bit; gradients to 1e-5 (two runs that sum the same terms in another order)."""
    sd = MODES[mode][0]
    sc = SCENES[scene]()
    plain = run(sc, sd, backward_mode=backward_mode)
    B = np.broadcast_to(np.asarray(sc.bg, np.float32)[:, None, None], (3, sc.H, sc.W)).copy()
    got = run(sc, sd, bg=B, backward_mode=backward_mode)
    assert plain["grad_fn"] == got["grad_fn"] == "_RasterizeGaussiansBackward"
    assert torch.equal(got["color"], plain["color"]) and torch.equal(got["radii"], plain["radii"])
    print(f"\n{mode} {backward_mode} {scene}")
    check_gaussian_grads(got, plain, 1e-5)


# ---- 4. the alpha gradient against the existing API -------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["b", "saturating"])
@pytest.mark.parametrize("mode,backward_mode", MODE_BACKWARD)
def test_alpha_gradient_against_the_existing_api(mode, backward_mode, scene):
    """colors_precomp = 0, bg = (1, 0, 0), dL_dout = (-wA, 0, 0): today's path computes the gradient of sum(wA * (1 - T)) term for term,
    with final_color exactly 0.  The new path's gradient of sum(wA * alpha) is the same sum: 1e-5."""
    sd = MODES[mode][0]
    sc = SCENES[scene]()
    sc.colors_precomp, sc.shs = np.zeros((len(sc.means3D), 3), np.float32), None
    wA = trb.weights(sc)[2]
    w_old = np.zeros((3, sc.H, sc.W), np.float32)
    w_old[0] = -wA
    old = run(sc, sd, bg=trb.E0, w=w_old, backward_mode=backward_mode)
    new = run(sc, sd, alpha=True, w=False, wA=wA, backward_mode=backward_mode)
    assert torch.equal(new["alpha"][0], 1.0 - old["color"][0])   # (C == 0: the image over e0 is T)
    print(f"\n{mode} {backward_mode} {scene}")
    check_gaussian_grads(new, old, 1e-5, names=("means3D", "means2D", "opacities", "scales", "rotations"))
    assert float(old["means3D"].abs().max()) > 0.0


# ---- 5. nothing else moves --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,backward_mode", MODE_BACKWARD)
def test_nothing_else_moves(mode, backward_mode):
    """_alpha with no gradient for alpha: image and radii bit for bit, gradients to 1e-5 of a run without the request.  The uniform
    background gradient is the same bits over two runs."""
    sd = MODES[mode][0]
    sc = _scene_b()
    plain = run(sc, sd, backward_mode=backward_mode)
    got = run(sc, sd, alpha=True, backward_mode=backward_mode)
    assert got["grad_fn"] == plain["grad_fn"] == "_RasterizeGaussiansBackward"
    assert torch.equal(got["color"], plain["color"]) and torch.equal(got["radii"], plain["radii"])
    assert torch.equal(got["alpha"][0], 1.0 - got["final_T"].view(sc.H, sc.W))
    print(f"\n{mode} {backward_mode}")
    check_gaussian_grads(got, plain, 1e-5)
    one, two = (run(sc, sd, bg_grad=True, backward_mode=backward_mode) for _ in range(2))
    assert one["bg"].shape == (3,) and torch.equal(one["bg"], two["bg"]) and torch.equal(one["color"], plain["color"])
    want = (one["final_T"].double().view(1, -1) * torch.tensor(sc.dL_dout, dtype=torch.float64, device=DEV).view(3, -1)).sum(1)
    assert _rel(one["bg"].double().cpu().numpy(), want.cpu().numpy()) < 1e-5
    check_gaussian_grads(one, plain, 1e-5)


# ---- 6. combined requests, edge cases, refusals -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,backward_mode", [("global", "replay"), ("hier_full", "replay"), ("hier_full", "resort"), ("kbuffer16", "replay")])
def test_with_camera_gradients_absgrad_and_blend_stats(mode, backward_mode):
    """All four requests in one backward: the Gaussian and camera gradients against the yardstick with the camera as leaves; the blend
    statistics, which do not depend on the loss, are those of a plain run; absgrad bounds |means2D.grad|."""
    sd = MODES[mode][0]
    sc = tiny()
    B, w, wA = trb.weights(sc)
    ref = reference("seed7", mode, camera_leaves=True)
    got = run(sc, sd, bg=B, bg_grad=True, alpha=True, wA=wA, backward_mode=backward_mode, camera=CAMERA, absgrad=True, stats=True)
    assert got["grad_fn"] == "_RasterizeGaussiansBackgroundBackward"
    assert max_abs(got["color"].cpu().numpy(), ref["image"]) < 2e-6
    print(f"\n{mode} {backward_mode}")
    check_gaussian_grads(got, ref["grads"], 5e-5, names=GAUSS + CAMERA)
    assert max_abs(got["bg"].cpu().numpy(), ref["dB"]) < 2e-6 * float(np.max(np.abs(w)))
    plain = run(sc, sd, backward_mode=backward_mode, stats=True)
    assert torch.equal(got["stats"][:, 2], plain["stats"][:, 2]) and _rel(got["stats"].cpu().numpy(), plain["stats"].cpu().numpy()) < 1e-5
    assert got["absgrad"].shape == (len(sc.means3D), 3) and torch.isfinite(got["absgrad"]).all()
    assert torch.all(got["absgrad"][:, :2] >= got["means2D"][:, :2].abs() - 1e-5 * got["absgrad"].max())
    # only the camera of the three explicit camera inputs that requires grad gets one
    some = run(sc, sd, bg=B, bg_grad=True, backward_mode=backward_mode, camera=("viewmatrix",))
    assert some["viewmatrix"] is not None and some["projmatrix"] is None and some["campos"] is None and some["bg"] is not None


@pytest.mark.parametrize("mode,backward_mode", MODE_BACKWARD)
def test_backward_through_alpha_alone(mode, backward_mode):
    """No colour gradient reaches the node: the alpha term alone, against the yardstick with w = 0 (B drops out of the loss)."""
    sd = MODES[mode][0]
    sc = tiny()
    B, w, wA = trb.weights(sc)
    ref = trb.reference(sc, B, np.zeros_like(w), wA, **MODES[mode][1])
    got = run(sc, sd, bg=B, alpha=True, w=False, wA=wA, backward_mode=backward_mode)
    print(f"\n{mode} {backward_mode}")
    check_gaussian_grads(got, ref["grads"], 5e-5, names=("means3D", "means2D", "opacities", "scales", "rotations"))
    assert torch.all(got["shs"] == 0)   # alpha does not depend on the colours


def test_empty_and_culled_frames():
    empty = scenes.make_scene(P=1, W=48, H=40, sigma_min=1.0, sigma_max=2.0, seed=1, camera="orbit")
    for f in ("means3D", "scales", "rotations", "opacities", "shs"):
        setattr(empty, f, getattr(empty, f)[:0])
    B = trb.weights(empty)[0]
    wA = np.ones((empty.H, empty.W), np.float32)
    for bg in (None, B):   # P == 0: nothing is launched, the zero image stands; alpha and the background gradient are zeros
        got = run(empty, settings_dict(**FULL_STP), bg=bg, bg_grad=True, alpha=True, wA=wA, only=("opacities", "means2D"))
        assert torch.all(got["color"] == 0) and torch.all(got["alpha"] == 0) and got["alpha"].shape == (1, empty.H, empty.W)
        assert got["bg"].shape == ((3,) if bg is None else B.shape) and torch.all(got["bg"] == 0)
    behind = scenes.make_scene(P=200, W=48, H=40, sigma_min=1.0, sigma_max=8.0, seed=7)   # camera at the origin looking down +z
    behind.means3D = (behind.means3D * np.array([1, 1, -1], np.float32)).astype(np.float32)
    B = trb.weights(behind)[0]
    w = np.asarray(behind.dL_dout, np.float32)
    for sd in (settings_dict(0), settings_dict(2, per_pixel=16), settings_dict(**FULL_STP)):   # everything culled: the background alone
        got = run(behind, sd, bg=B, bg_grad=True, alpha=True, wA=wA)
        assert torch.all(got["radii"] == 0) and torch.all(got["alpha"] == 0)
        assert torch.equal(got["color"], torch.tensor(B, device=DEV))
        assert torch.equal(got["bg"], torch.tensor(w, device=DEV))   # T == 1: dL/dB = w
        assert torch.all(got["means3D"] == 0)
        uni = run(behind, sd, bg_grad=True)
        assert _rel(uni["bg"].double().cpu().numpy(), w.astype(np.float64).reshape(3, -1).sum(1)) < 1e-5


@pytest.mark.parametrize("mode,backward_mode", [("global", "replay"), ("hier_full", "replay"), ("kbuffer16", "resort")])
def test_tile_row_window(mode, backward_mode):
    """A frame of four tile rows rendered for rows [1, 3): inside, image, alpha and dL/dB are the full frame's bit for bit; outside,
    nothing is written (the zero-filled outputs stand).  The uniform gradient sums the window's rows."""
    sd = MODES[mode][0]
    sc = sparse()
    B, w, wA = trb.weights(sc)
    full = run(sc, sd, bg=B, bg_grad=True, alpha=True, wA=wA, backward_mode=backward_mode)
    part = run(sc, sd, bg=B, bg_grad=True, alpha=True, wA=wA, backward_mode=backward_mode, tile_rows=(1, 3))
    rows = slice(16, 48)
    for k in ("color", "alpha", "bg"):
        assert torch.equal(part[k][:, rows], full[k][:, rows]), k
        assert torch.all(part[k][:, :16] == 0) and torch.all(part[k][:, 48:] == 0), k
    uni = run(sc, sd, bg_grad=True, backward_mode=backward_mode, tile_rows=(1, 3))
    want = full["bg"][:, rows].double().reshape(3, -1).sum(1)
    assert _rel(uni["bg"].double().cpu().numpy(), want.cpu().numpy()) < 1e-5


def test_refusals():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import tile_shard
    sc = tiny()
    B = trb.weights(sc)[0]
    sd = settings_dict(**FULL_STP)
    with pytest.raises(RuntimeError, match=r"alpha output.*per-pixel background.*render_depth=True"):
        run(sc, sd, alpha=True, render_depth=True, backward=False)
    with pytest.raises(RuntimeError, match=r"alpha output.*per-pixel background.*render_depth=True"):
        run(sc, sd, bg=B, render_depth=True, backward=False)
    with pytest.raises(RuntimeError, match=r"background that requires grad.*render_depth=True"):   # (that image is not C + T * bg either)
        run(sc, sd, bg_grad=True, render_depth=True)
    # the refused forward left no request behind: the next plain forward is the plain image, and a render_depth one runs
    plain = run(sc, sd, backward=False)
    assert plain["alpha"] is None and torch.isfinite(plain["color"]).all()
    assert torch.isfinite(run(sc, sd, render_depth=True, backward=False)["color"]).all()
    dev = torch.device(DEV)
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    m = t(sc.means3D).requires_grad_(True)
    call = lambda rs: tile_shard.TileRowShardedRasterizer(rs, None, 0, 1)(m, torch.zeros_like(m), t(sc.opacities), shs=t(sc.shs),
                                                                          scales=t(sc.scales), rotations=t(sc.rotations))
    es = ext_settings(sd)
    es._alpha = True
    for rs in (api_settings(sc, es, dev), api_settings(sc, ext_settings(sd), dev, bg=t(B)),
               api_settings(sc, ext_settings(sd), dev, bg=t(sc.bg).requires_grad_(True))):
        with pytest.raises(RuntimeError, match=r"alpha output.*per-pixel background.*requires grad.*tile-row sharding.*not exchanged"):
            call(rs)
    # PPX_FULL: forward only, as without the request
    got = run(sc, settings_dict(1), bg=B, alpha=True, backward=False)
    assert got["alpha"] is not None and torch.isfinite(got["color"]).all()
    with pytest.raises(RuntimeError, match=r"[Bb]ackward not supported"):
        run(sc, settings_dict(1), bg=B, alpha=True, wA=np.ones((sc.H, sc.W), np.float32))


def test_trainer_example_with_a_mask_term():
    """examples/train_render.py --mask-weight: render() hands the alpha out, the 30-iteration fit takes a mask term on it and still descends."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_render", os.path.join(root, "examples", "train_render.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    first, last = mod.main(["--iters", "25", "--config", "full", "--points", "4000", "--size", "160", "112", "--mask-weight", "0.5"])
    assert last < 0.6 * first, (first, last)
    # render() itself: a (3, H, W) background, the alpha in the dict
    dev = torch.device(DEV)
    sc = sparse()
    cfg = mod.splat_config("full")
    cfg._alpha = True
    B = torch.tensor(trb.weights(sc)[0], device=dev)
    with torch.no_grad():
        out = mod.render(mod.camera_of(sc, dev), mod.ToyGaussians(sc, dev), B, cfg)
    assert out["alpha"].shape == (1, sc.H, sc.W) and out["render"].shape == (3, sc.H, sc.W)
    assert torch.equal(out["render"][:, out["alpha"][0] == 0], B[:, out["alpha"][0] == 0])
