"""GPU tests of the split SH inputs (GaussianRasterizer.forward's dc=; include/stp_raster.h: stp_set_forward_split_sh,
stp_set_backward_split_sh).  The reference is the concatenated path on the same values: only the staging between global memory and LDS
differs, so the forward and the per-Gaussian half of the backward must agree BIT FOR BIT; whole backwards, whose render half sums with
float atomics, agree to the bound the project uses for two product paths that differ in atomic order (tests/test_gpu_fused_gather.py)."""
import functools

import numpy as np
import pytest
import torch

import helpers
from helpers import FULL_STP, _rel, settings_dict
from diff_gaussian_rasterization import scenes

pytestmark = pytest.mark.gpu

# one row; a full block on the unrolled path; tails of 1, 44 and 255 rows, whose float counts are and are not multiples of 4; three blocks
PS = (1, 255, 256, 257, 300, 513)
MD = ((1, 0), (4, 1), (9, 2), (16, 3), (16, 1))   # (M, sh_degree)
MODES = {"global": settings_dict(0), "full_stp": settings_dict(**FULL_STP)}
SH = 16   # index of `sh` in the positional layout of _C.rasterize_gaussians_backward (helpers._direct)
NAMES8 = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")


@functools.lru_cache(maxsize=None)
def _base(P):
    return scenes.make_scene(P=P, W=48, H=32, sigma_min=1.0, sigma_max=9.0, seed=4)   # (as helpers._scene_a)


def scene(P, M, D):
    import copy
    sc = copy.copy(_base(P))
    sc.shs = np.ascontiguousarray(sc.shs[:, :M])
    sc.sh_degree = D
    return sc


def split(shs, misaligned=False):
    """dc = shs[:, :1], rest = shs[:, 1:], each contiguous; misaligned: as the [1:] slices of tensors one row longer (dc sits 12 bytes
    past its allocation, rest 12 (M - 1) bytes)."""
    dc, rest = shs[:, :1].contiguous(), shs[:, 1:].contiguous()
    if misaligned:
        pad = lambda t: torch.cat((torch.zeros_like(t[:1]), t))[1:]
        dc, rest = pad(dc), pad(rest)
        assert dc.is_contiguous() and rest.is_contiguous() and dc.data_ptr() % 16 != 0
    return dc, rest


def forward_pair(sc, sd, misaligned=False):
    """(the backward's positional arguments of the concatenated forward, the same with sh = rest, dc, the split forward's outputs)"""
    from diff_gaussian_rasterization import _C
    args = helpers._direct(sc, sd)
    dc, rest = split(args[SH], misaligned)
    out = _C.rasterize_gaussians(args[0], args[1], args[4], args[3], args[5], args[6], args[7], args[8], args[9], args[10], args[11],
                                 args[12], args[13], sc.H, sc.W, rest, sc.sh_degree, args[18], False, sd, False, False, dc=dc)
    return args, args[:SH] + (rest,) + args[SH + 1:], dc, out


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("M,D", MD)
@pytest.mark.parametrize("P", PS)
def test_forward_equals_the_concatenated_path(P, M, D, mode):
    sc, sd = scene(P, M, D), MODES[mode]
    args, _, dc, out = forward_pair(sc, sd)
    assert out[0] == args[20], "num_rendered"
    assert torch.equal(out[1], args[14]), "image"
    assert torch.equal(out[2], args[2]), "radii"
    assert args[20] > 0 and int((args[2] > 0).sum()) > 0   # (something is rendered: the colours are read)
    from diff_gaussian_rasterization import _C   # ... and dc as (P, 3)
    flat = _C.rasterize_gaussians(args[0], args[1], args[4], args[3], args[5], args[6], args[7], args[8], args[9], args[10], args[11], args[12],
                                  args[13], sc.H, sc.W, split(args[SH])[1], sc.sh_degree, args[18], False, sd, False, False, dc=dc.reshape(P, 3))
    assert flat[0] == args[20] and torch.equal(flat[1], args[14]) and torch.equal(flat[2], args[2])


def api(sc, sd, dc_mode, requires=True, frozen=(), camera=(), bg_grad=False, extras=False, dc_flat=False, no_grad=False):
    """Forward (+ backward) through the public API on cuda:0.  dc_mode False: shs = the concatenated tensor; True: dc= and shs = the rest.
    Returns {"out": the outputs, name: .grad} -- the concatenated run's "dc" and "rest" are the slices of shs.grad."""
    import diff_gaussian_rasterization as dgr
    dev = torch.device("cuda:0")
    t = lambda a, rg=False: torch.tensor(np.asarray(a, np.float32), device=dev).requires_grad_(rg)
    need = lambda n: requires and n not in frozen
    ten = {n: t(getattr(sc, n), need(n)) for n in ("means3D", "opacities", "scales", "rotations")}
    ten["means2D"] = torch.zeros_like(ten["means3D"], requires_grad=need("means2D"))
    shs = t(sc.shs)
    if dc_mode:
        dc, rest = split(shs)
        if dc_flat:
            dc = dc.reshape(-1, 3)
        ten["dc"], ten["rest"] = dc.requires_grad_(need("dc")), rest.requires_grad_(need("rest"))
    else:
        ten["shs"] = shs.requires_grad_(requires)
    cam = {n: t(getattr(sc, n), True) for n in camera}
    if bg_grad:
        cam["bg"] = t(sc.bg, True)
    es = helpers.ext_settings(sd)
    if extras:
        es._alpha = es._invdepth = es._absgrad = es._blend_stats = True
    rs = helpers.api_settings(sc, es, dev, **cam)
    rast = dgr.GaussianRasterizer(rs)
    kw = dict(scales=ten["scales"], rotations=ten["rotations"])
    with torch.no_grad() if no_grad else torch.enable_grad():
        if dc_mode:
            out = rast(ten["means3D"], ten["means2D"], ten["opacities"], shs=ten["rest"] if sc.shs.shape[1] > 1 else None, dc=ten["dc"], **kw)
        else:
            out = rast(ten["means3D"], ten["means2D"], ten["opacities"], shs=ten["shs"], **kw)
    res = {"out": [o.detach() for o in out], "grad_fn": type(out[0].grad_fn).__name__ if out[0].grad_fn is not None else None}
    if out[0].grad_fn is not None:
        res["saved"] = out[0].grad_fn.saved_tensors
        w = t(sc.dL_dout)
        loss = (out[0] * w).sum()
        for k, extra in enumerate(out[2:]):   # alpha, invdepth: weights of their own
            loss = loss + (extra * w[k:k + 1] * (0.5 + k)).sum()
        loss.backward()
    for n, x in list(ten.items()) + list(cam.items()):
        res[n] = x.grad
    if not dc_mode and ten["shs"].grad is not None:
        res["dc"], res["rest"] = ten["shs"].grad[:, :1], ten["shs"].grad[:, 1:]
    res["absgrad"], res["blend_stats"] = getattr(ten["means2D"], "absgrad", None), getattr(ten["means2D"], "blend_stats", None)
    return res


@pytest.mark.parametrize("mode", list(MODES))
def test_forward_under_no_grad(mode):
    sc, sd = scene(300, 16, 3), MODES[mode]
    a, b = api(sc, sd, False, no_grad=True), api(sc, sd, True, no_grad=True)
    assert a["grad_fn"] is None and b["grad_fn"] is None
    assert torch.equal(a["out"][0], b["out"][0]) and torch.equal(a["out"][1], b["out"][1])
    assert float(a["out"][0].abs().max()) > 0.0


def per_gaussian_pair(args, sargs, dc, **kw):
    """phases = 1 once, then the per-Gaussian half twice on clones of the same records: concatenated, and with dc="""
    from diff_gaussian_rasterization import _C
    records = _C.rasterize_gaussians_backward(*args, phases=1)
    ref = _C.rasterize_gaussians_backward(*args, phases=2, partial=records.clone(), **kw)
    got = _C.rasterize_gaussians_backward(*sargs, phases=2, partial=records.clone(), dc=dc, **kw)
    return records, ref, got


def assert_equal_outputs(ref, got, camera=False, D=0):
    assert len(got) == len(ref) + 1
    for k, n in enumerate(NAMES8):
        if n == "dL_dsh":
            assert got[k].shape == ref[k][:, 1:].shape and got[k].is_contiguous()
            assert torch.equal(got[k], ref[k][:, 1:]), "dL_drest"
            assert got[-1].shape == (ref[k].shape[0], 3) and got[-1].is_contiguous()
            assert torch.equal(got[-1], ref[k][:, 0]), "dL_ddc"
        else:
            assert torch.equal(got[k], ref[k]), n
    if camera:
        for k, n in ((8, "dL_dviewmatrix"), (9, "dL_dprojmatrix"), (10, "dL_dcampos")):
            assert torch.equal(got[k], ref[k]), n
        assert D == 0 or float(ref[10].abs().max()) > 0.0   # (campos flows through the SH view direction: the rest's coefficients are read)
    assert float(ref[5].abs().max()) > 0.0


@pytest.mark.parametrize("camera", [False, True])
@pytest.mark.parametrize("M,D", MD)
@pytest.mark.parametrize("P", PS)
def test_per_gaussian_backward_is_bit_identical(P, M, D, camera):
    sc, sd = scene(P, M, D), MODES["full_stp"]
    args, sargs, dc, _ = forward_pair(sc, sd)
    _, ref, got = per_gaussian_pair(args, sargs, dc, **({"camera_grads": True} if camera else {}))
    assert_equal_outputs(ref, got, camera, D)


@pytest.mark.parametrize("M,D", MD)
def test_chunked_per_gaussian_backward_is_bit_identical(M, D):
    """chunk = (k, K), K = 2, P = 600 (three 256-Gaussian blocks: chunk 0 gets one, chunk 1 two, the last a partial one)"""
    from diff_gaussian_rasterization import _C
    sc, sd = scene(600, M, D), MODES["full_stp"]
    args, sargs, dc, _ = forward_pair(sc, sd)
    records, ref, _ = per_gaussian_pair(args, sargs, dc)
    got = None
    for k in range(2):
        got = _C.rasterize_gaussians_backward(*sargs, phases=2, partial=records.clone(), chunk=(k, 2), outputs=got, dc=dc)
        if k == 0:   # (rows of the second chunk: not written yet -- poisoned, so that a chunk which skips its rows shows)
            got[5][256:] = float("nan")
            got[-1][256:] = float("nan")
    assert_equal_outputs(ref, got)


@pytest.mark.parametrize("M,D", [(4, 1), (16, 3)])   # rest[1:] sits 36 and 180 bytes past its allocation: neither is 16-byte aligned
@pytest.mark.parametrize("P", (256, 300))
def test_misaligned_views(P, M, D):
    from diff_gaussian_rasterization import _C
    sc, sd = scene(P, M, D), MODES["full_stp"]
    args, sargs, dc, out = forward_pair(sc, sd, misaligned=True)
    assert dc.data_ptr() % 16 != 0 and sargs[SH].data_ptr() % 16 != 0
    assert out[0] == args[20] and torch.equal(out[1], args[14]) and torch.equal(out[2], args[2])
    records, ref, got = per_gaussian_pair(args, sargs, dc)
    assert_equal_outputs(ref, got)
    # ... and misaligned OUTPUTS: the two SH gradients as [1:] views, handed in through `outputs`
    outs = list(got[:8]) + [got[-1]]
    outs[5] = torch.full((P + 1, M - 1, 3), float("nan"), device=dc.device)[1:]
    outs[8] = torch.full((P + 1, 3), float("nan"), device=dc.device)[1:]
    assert outs[5].data_ptr() % 16 != 0 and outs[8].data_ptr() % 16 != 0
    got2 = _C.rasterize_gaussians_backward(*sargs, phases=2, partial=records.clone(), outputs=outs, dc=dc)
    assert got2[5].data_ptr() == outs[5].data_ptr() and got2[-1].data_ptr() == outs[8].data_ptr()
    assert_equal_outputs(ref, got2)


KINDS = {"plain": dict(), "camera": dict(camera=("viewmatrix", "projmatrix", "campos")), "background": dict(bg_grad=True)}
FUNCTION = {"plain": "_RasterizeGaussiansBackward", "camera": "_RasterizeGaussiansCameraBackward", "background": "_RasterizeGaussiansBackgroundBackward"}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_autograd_end_to_end(kind, mode):
    sc, sd = scene(300, 16, 3), MODES[mode]
    a, b = api(sc, sd, False, **KINDS[kind]), api(sc, sd, True, **KINDS[kind])
    assert a["grad_fn"] == b["grad_fn"] == FUNCTION[kind]
    assert torch.equal(a["out"][0], b["out"][0]) and torch.equal(a["out"][1], b["out"][1])
    P = len(sc.means3D)
    assert b["dc"].shape == (P, 1, 3) and b["rest"].shape == (P, 15, 3) and b["dc"].is_contiguous() and b["rest"].is_contiguous()
    names = ["means3D", "means2D", "opacities", "scales", "rotations", "dc", "rest"] + list(KINDS[kind].get("camera", ())) + (["bg"] if kind == "background" else [])
    for n in names:
        assert a[n] is not None and b[n] is not None, n
        r = _rel(b[n].cpu().numpy(), a[n].cpu().numpy())
        print(f"{kind} {mode} {n}: rel {r:.2e}")
        assert r < 2e-5, (n, r)
        assert float(a[n].abs().max()) > 0.0 or n == "means2D", n
    # dc is saved behind the twelve tensors every Function saves (and the camera's / bg's), the buffers keep their places
    saved = b["saved"]
    assert saved[11].dtype == torch.uint8 and saved[7].shape == (P, 15, 3)
    assert saved[{"plain": 12, "camera": 15, "background": 16}[kind]].shape == (P, 1, 3)


def test_shapes_of_the_gradients_follow_the_inputs():
    sc, sd = scene(257, 4, 1), MODES["full_stp"]
    a = api(sc, sd, False)
    b = api(sc, sd, True, dc_flat=True)   # (P, 3) in -> (P, 3) out
    assert b["dc"].shape == (257, 3) and b["dc"].is_contiguous() and b["rest"].shape == (257, 3, 3) and b["rest"].is_contiguous()
    assert _rel(b["dc"].cpu().numpy(), a["dc"][:, 0].cpu().numpy()) < 2e-5 and _rel(b["rest"].cpu().numpy(), a["rest"].cpu().numpy()) < 2e-5
    # a degree-0 model: no rest at all
    sc = scene(257, 1, 0)
    a, b = api(sc, sd, False), api(sc, sd, True)
    assert torch.equal(a["out"][0], b["out"][0])
    assert b["dc"].shape == (257, 1, 3) and _rel(b["dc"].cpu().numpy(), a["dc"].cpu().numpy()) < 2e-5


@pytest.mark.parametrize("frozen", ["dc", "rest"])
def test_a_frozen_half_gets_no_gradient(frozen):
    sc, sd = scene(300, 16, 3), MODES["full_stp"]
    a, b = api(sc, sd, False), api(sc, sd, True, frozen=(frozen,))
    other = "rest" if frozen == "dc" else "dc"
    assert b[frozen] is None and b[other] is not None
    assert _rel(b[other].cpu().numpy(), a[other].cpu().numpy()) < 2e-5
    assert _rel(b["means3D"].cpu().numpy(), a["means3D"].cpu().numpy()) < 2e-5


def test_all_extras_together():
    """_alpha, _invdepth, _absgrad and _blend_stats switched on at once, with dc="""
    sc, sd = scene(300, 16, 3), MODES["full_stp"]
    a, b = api(sc, sd, False, extras=True), api(sc, sd, True, extras=True)
    assert len(a["out"]) == len(b["out"]) == 4
    for x, y in zip(a["out"], b["out"]):
        assert torch.equal(x, y)
    for n in ("means3D", "means2D", "opacities", "scales", "rotations", "dc", "rest", "absgrad", "blend_stats"):
        assert a[n] is not None and b[n] is not None, n
        r = _rel(b[n].cpu().numpy(), a[n].cpu().numpy())
        print(f"extras {n}: rel {r:.2e}")
        assert r < 2e-5, (n, r)


@pytest.mark.parametrize("extra", [[], ["--optimizer", "sparse_adam", "--strategy", "adc"], ["--optimizer", "sparse_adam", "--strategy", "mcmc"]],
                         ids=["adam", "sparse_adam-adc", "sparse_adam-mcmc"])
def test_example_trains_with_split_sh(extra):
    """examples/train_render.py --split-sh: two SH parameters in two optimizer groups, rendered with dc=; the short fit still descends, with
    the fused optimizer and through a densification / relocation step that replaces or rewrites both parameters."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_render", os.path.join(root, "examples", "train_render.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    first, last = mod.main(["--iters", "15", "--points", "3000", "--size", "96", "64", "--split-sh"] + extra)
    assert last < 0.8 * first, (first, last)
