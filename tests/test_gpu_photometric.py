"""GPU tests of the fused photometric loss (photometric_terms, fused_ssim, photometric_loss, _C.photometric_forward / _backward;
include/stp_raster.h: stp_photometric_forward / stp_photometric_backward) against the float64 yardstick tests/torch_ref_photometric.py.

Every element of out and of dL/dimage is held to the bounds counted from float32 roundings (torch_ref_photometric.bounds).  A workgroup of
the kernels owns a TW x TH tile of one plane (read from include/stp_raster.h): the shapes are one pixel, an image smaller than the window,
exactly one tile, one pixel more than a tile each way (four workgroups per plane), more than two tiles each way, a flat image of three
tiles with a ragged end, and a (B, C, H, W) batch; one case takes the image from a view that starts 4 bytes into its storage."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import torch_ref_photometric as ref
from helpers import FULL_STP, _rel, api_settings, ext_settings, settings_dict

pytestmark = pytest.mark.gpu

TW, TH = ref.tile()
SHAPES = [(1, 1, 1), (3, 7, 5), (3, TH, TW), (3, TH + 1, TW + 1), (3, 2 * TH + 3, 2 * TW + 3), (1, 5, 3 * TW - 1), (2, 3, 37, 53)]
FAMILIES = ("random", "smooth", "constant", "identical")
GRADS = ((0.8, -0.2), (0.35, 1.25), (1.0, 0.0), (0.0, 1.0))   # lambda = 0.2, a second pair, and each term without the other


def _dgr():
    import diff_gaussian_rasterization as dgr
    return dgr


def _planes(shape):
    return (int(np.prod(shape[:-2])),) + tuple(shape[-2:])


@functools.lru_cache(maxsize=None)
def yardstick(shape, family):
    """(x, y, out, out bound, {g: (grad, grad bound)}) of one case: computed once, shared, never modified.  x, y: float32 arrays of `shape`."""
    x, y = ref.images(family, *_planes(shape), seed=7)
    out = ref.terms(x, y)
    # the closed form and its bound are linear in (g0, g1) and in (|g0|, |g1|): two evaluations serve every pair
    g_l1, g_ssim = ref.grad(x, y, 1.0, 0.0), ref.grad(x, y, 0.0, 1.0)
    out_bound, b_l1 = ref.bounds(x, y, 1.0, 0.0)
    _, b_ssim = ref.bounds(x, y, 0.0, 1.0)
    per_g = {g: (g[0] * g_l1 + g[1] * g_ssim, abs(g[0]) * b_l1 + abs(g[1]) * b_ssim) for g in GRADS}
    return x.reshape(shape), y.reshape(shape), out, out_bound, per_g


def dev(a, offset_floats=0):
    """A contiguous cuda tensor of the array's values; offset_floats = 1: a view that starts 4 bytes into its storage."""
    a = np.ascontiguousarray(a, np.float32)
    if offset_floats == 0:
        return torch.from_numpy(a).cuda()
    base = torch.empty(a.size + offset_floats, dtype=torch.float32, device="cuda")
    view = base[offset_floats:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 * offset_floats and view.is_contiguous()
    return view


def run(x, y, g, offset_floats=0):
    """(out, dL/dimage) of the fused kernels for dL/dout = g, as float64 CPU tensors."""
    image, target = dev(x, offset_floats).detach().requires_grad_(True), dev(y)
    out = _dgr().photometric_terms(image, target)
    (g[0] * out[0] + g[1] * out[1]).backward()
    assert out.shape == (2,) and out.dtype == torch.float32 and image.grad.shape == image.shape and image.grad.dtype == torch.float32
    return out.detach().double().cpu(), image.grad.double().cpu()


def worst(err, bound):
    """The largest err / bound; an error of exactly 0 counts as 0 whatever the bound."""
    err, bound = err.reshape(-1), bound.reshape(-1)
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


def check(shape, family, offset_floats=0):
    x, y, out64, out_bound, per_g = yardstick(shape, family)
    ratios = {}
    for g, (grad64, grad_bound) in per_g.items():
        out, grad = run(x, y, g, offset_floats)
        ratios[g] = (worst((out - out64).abs(), out_bound), worst((grad.reshape(grad64.shape) - grad64).abs(), grad_bound))
        if family == "identical":
            assert float(out[0]) == 0.0
            if g[1] == 0.0:
                assert not grad.any()   # sign(0) = 0: the L1 part is exactly 0
    print(shape, family, "worst error / bound (out, gradient) per dL/dout:", {g: "%.3g, %.3g" % r for g, r in ratios.items()})
    top = max(max(r) for r in ratios.values())
    assert top <= 1.0, f"{shape} {family}: worst error / bound {top:.3g}; (out, gradient) per dL/dout: {ratios}"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_out_and_gradient_are_within_the_bounds(shape, family):
    check(shape, family)


@pytest.mark.parametrize("family", ("random", "smooth"))
def test_image_that_starts_4_bytes_into_its_storage(family):
    check((3, TH + 1, TW + 1), family, offset_floats=1)


def test_identical_images():
    """out[0] == 0 exactly, SSIM within its bound of 1, the L1 part of the gradient exactly 0 and the SSIM part within its bound."""
    shape = (3, 2 * TH + 3, 2 * TW + 3)
    x, y, out64, out_bound, per_g = yardstick(shape, "identical")
    assert np.array_equal(x, y) and float(out64[0]) == 0.0 and abs(float(out64[1]) - 1.0) < 1e-12
    out, grad = run(x, y, (1.0, 0.0))
    assert float(out[0]) == 0.0 and not grad.any()
    assert abs(float(out[1]) - float(out64[1])) <= float(out_bound[1])
    out, grad = run(x, y, (0.0, 1.0))
    grad64, grad_bound = per_g[(0.0, 1.0)]
    w = worst((grad.reshape(grad64.shape) - grad64).abs(), grad_bound)
    assert w <= 1.0, f"the SSIM part of the gradient: worst error / bound {w:.3g}"


def test_composition_and_gradient_rules():
    dgr = _dgr()
    x, y, *_ = yardstick((2, 3, 37, 53), "smooth")
    image, target = dev(x).requires_grad_(True), dev(y).requires_grad_(True)   # (a target that requires grad is accepted and gets none)
    terms = dgr.photometric_terms(image, target)
    loss = dgr.photometric_loss(image, target, lambda_dssim=0.2)
    assert loss.shape == () and torch.equal(loss, (1.0 - 0.2) * terms[0] + 0.2 * (1.0 - terms[1]))
    assert torch.equal(dgr.photometric_loss(image, target), loss)   # (0.2 is the default)
    ssim_train, ssim_eval = dgr.fused_ssim(image, target), dgr.fused_ssim(image, target, padding="same", train=False)
    assert ssim_train.shape == () and torch.equal(ssim_train, terms[1]) and torch.equal(ssim_eval, ssim_train)
    with torch.no_grad():
        assert torch.equal(dgr.photometric_terms(image, target), terms) and not dgr.photometric_loss(image, target).requires_grad
    loss.backward()
    assert image.grad is not None and image.grad.shape == image.shape and bool(image.grad.any()) and target.grad is None
    by_terms = torch.autograd.grad((1.0 - 0.2) * terms[0] + 0.2 * (1.0 - terms[1]), image)[0]
    assert torch.equal(by_terms, image.grad)
    with pytest.raises(RuntimeError, match="stored no derivative maps"):
        ssim_eval.backward()
    ssim_train.backward()   # (the gradient of the mean SSIM alone accumulates)
    # the binding's face: maps only on request, the same out either way
    from diff_gaussian_rasterization import _C
    out_a, maps = _C.photometric_forward(image.detach(), target.detach(), True)
    out_b, none = _C.photometric_forward(image.detach(), target.detach(), False)
    assert none is None and maps.shape == (3,) + image.shape and torch.equal(out_a, out_b) and torch.equal(out_a, terms.detach())
    # (C, H, W) planes of a batch are independent: the batch's terms are the means over its images'
    per_image = torch.stack([dgr.photometric_terms(image[b], target[b]) for b in range(2)]).double().mean(0)
    assert torch.allclose(per_image, terms.double(), rtol=1e-6, atol=0)


def test_non_contiguous_inputs_are_made_contiguous():
    dgr = _dgr()
    x, y, *_ = yardstick((3, TH + 1, TW + 1), "random")
    hwc, target_hwc = dev(x.transpose(1, 2, 0)), dev(y.transpose(1, 2, 0))   # (H, W, C) storage, (C, H, W) views
    image, target = hwc.permute(2, 0, 1).requires_grad_(True), target_hwc.permute(2, 0, 1)
    assert not image.is_contiguous()
    plain = dev(x).requires_grad_(True)
    a, b = dgr.photometric_loss(image, target), dgr.photometric_loss(plain, dev(y))
    a.backward()
    b.backward()
    assert torch.equal(a, b) and image.grad.shape == image.shape and torch.equal(image.grad, plain.grad)


def test_refusals_on_the_device():
    dgr = _dgr()
    a = torch.rand(3, 8, 8, device="cuda")
    with pytest.raises(RuntimeError, match="expected float32 tensor, got Half"):
        dgr.photometric_loss(a.half(), a.half())
    with pytest.raises(RuntimeError, match="image has shape"):
        dgr.photometric_loss(a, a[:, :7])
    with pytest.raises(RuntimeError, match="got 2 dimensions"):
        dgr.fused_ssim(a[0], a[0])
    with pytest.raises(RuntimeError, match="expected all tensors on cuda:0, got one on cpu"):
        dgr.photometric_terms(a, a.cpu())
    with pytest.raises(ValueError, match="valid"):
        dgr.fused_ssim(a, a, padding="valid")


def test_equal_inputs_give_equal_bits():
    x, y, *_ = yardstick((3, 2 * TH + 3, 2 * TW + 3), "random")
    first = run(x, y, GRADS[0])
    for _ in range(2):
        again = run(x, y, GRADS[0])
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def test_side_stream_without_host_synchronisation():
    """Issued on a non-default stream with torch's synchronisation check armed: nothing in the Python layer or the binding waits for the
    device or reads a value back (.item()); the results are those of the default stream, bit for bit."""
    dgr = _dgr()
    x, y, *_ = yardstick((3, 2 * TH + 3, 2 * TW + 3), "smooth")
    want_out, want_grad = run(x, y, (0.8, -0.2))
    image, target = dev(x).requires_grad_(True), dev(y)
    weights = torch.tensor([0.8, -0.2], device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(side):
            out = dgr.photometric_terms(image, target)
            (out * weights).sum().backward()
            loss = dgr.photometric_loss(image.detach(), target)   # (evaluation: no maps)
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    side.synchronize()
    assert torch.equal(out.detach().double().cpu(), want_out) and torch.equal(image.grad.double().cpu(), want_grad)
    assert torch.equal(loss, 0.8 * out[0].detach() + 0.2 * (1.0 - out[1].detach()))


def test_c_abi_on_a_stream_and_its_launch_counts():
    """The C calls with device pointers on a non-default stream: the documented launch counts (forward 2, backward 1), the binding's bits."""
    from diff_gaussian_rasterization import _C
    L = _C._load()
    shape = (3, TH + 1, TW + 1)
    x, y, *_ = yardstick(shape, "random")
    image, target = dev(x), dev(y)
    weights = torch.tensor([0.8, -0.2], device="cuda")
    want_out, want_maps = _C.photometric_forward(image, target, True)
    want_grad = _C.photometric_backward(image, target, want_maps, weights)
    floats = L.stp_photometric_workspace_floats(*shape)
    assert floats == 2 * 3 * 2 * 2
    out, out_eval = torch.full((2,), -1.0, device="cuda"), torch.full((2,), -1.0, device="cuda")
    maps, workspace, grad = torch.empty(3 * image.numel(), device="cuda"), torch.empty(floats, device="cuda"), torch.empty_like(image)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(side.cuda_stream)
    assert L.stp_photometric_forward(*shape, p(image), p(target), p(out), p(maps), p(workspace), st) == 2
    assert L.stp_photometric_backward(*shape, p(image), p(target), p(maps), p(weights), p(grad), st) == 1
    assert L.stp_photometric_forward(*shape, p(image), p(target), p(out_eval), None, p(workspace), st) == 2
    assert L.stp_photometric_forward(0, TH, TW, p(image), p(target), p(out), p(maps), p(workspace), st) == 0   # empty work
    side.synchronize()
    assert torch.equal(out, want_out) and torch.equal(out_eval, want_out) and torch.equal(maps.view_as(want_maps), want_maps) and torch.equal(grad, want_grad)


def upstream_loss(image, target, lambda_dssim=0.2):
    """The trainers' composition in float32 torch: l1_loss + ssim() with a depthwise 11 x 11 conv2d (window_size = 11, size_average = True)."""
    C = image.shape[0]
    w = torch.from_numpy(ref.WINDOW32).to(image.device)
    window = (w[:, None] * w[None, :]).expand(C, 1, 11, 11).contiguous()
    blur = lambda v: F.conv2d(v[None], window, padding=5, groups=C)[0]
    mu1, mu2 = blur(image), blur(target)
    s1, s2, s12 = blur(image * image) - mu1 * mu1, blur(target * target) - mu2 * mu2, blur(image * target) - mu1 * mu2
    ssim_map = ((2 * mu1 * mu2 + ref.C1) * (2 * s12 + ref.C2)) / ((mu1 * mu1 + mu2 * mu2 + ref.C1) * (s1 + s2 + ref.C2))
    return (1.0 - lambda_dssim) * (image - target).abs().mean() + lambda_dssim * (1.0 - ssim_map.mean())


def test_end_to_end_through_the_rasterizer():
    """render -> photometric_loss -> backward gives the Gaussians the gradients that the torch composition of the loss gives them on the
    same render, within the rasterizer tests' gradient tolerance (helpers._rel < 1e-4, the grad_tol of test_gpu_parity)."""
    dgr = _dgr()
    from diff_gaussian_rasterization import scenes
    sc = scenes.make_scene(P=500, W=64, H=48, sigma_min=1.5, sigma_max=10.0, seed=9)
    device = torch.device("cuda:0")
    rs = api_settings(sc, ext_settings(settings_dict(**FULL_STP)), device)
    names = ("means3D", "opacities", "shs", "scales", "rotations")

    def grads(loss_fn, target):
        ten = {n: torch.tensor(np.asarray(getattr(sc, n), np.float32), device=device).requires_grad_(True) for n in names}
        means2D = torch.zeros_like(ten["means3D"], requires_grad=True)
        color, _ = dgr.GaussianRasterizer(rs)(ten["means3D"], means2D, ten["opacities"], shs=ten["shs"], colors_precomp=None, scales=ten["scales"],
                                              rotations=ten["rotations"], cov3D_precomp=None)
        if target is None:   # what the scene is fitted to: its own render, dimmed and disturbed
            rng = np.random.default_rng(2)
            target = (0.8 * color.detach() + torch.from_numpy(0.1 * rng.random(color.shape, dtype=np.float32)).to(device)).clamp(0.0, 1.0)
        loss = loss_fn(color, target)
        loss.backward()
        return color.detach(), target, float(loss.detach()), {n: t.grad.cpu().numpy() for n, t in ten.items()}

    color_a, target, loss_a, fused = grads(dgr.photometric_loss, None)
    color_b, _, loss_b, composed = grads(upstream_loss, target)
    assert torch.equal(color_a, color_b) and abs(loss_a - loss_b) <= 1e-5 * abs(loss_b)
    assert np.abs(composed["means3D"]).max() > 0
    for n in names:
        assert _rel(fused[n], composed[n]) < 1e-4, (n, _rel(fused[n], composed[n]))
