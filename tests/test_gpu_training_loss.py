"""GPU tests of the training loss (training_terms, training_loss, _C.training_loss_forward / _backward; include/stp_raster.h:
stp_training_loss_forward / stp_training_loss_backward) against the validated photometric path and the float64 yardstick
tests/torch_ref_training_loss.py.  No tolerance is tuned: every check is a bit-equality, a bound counted from the kernel's roundings, or
the end-to-end tolerance of test_gpu_photometric.

The shapes: one pixel, an image smaller than the window, one pixel more than a tile each way (four workgroups per plane), more than two
tiles each way, and a (B, 3, H, W) batch with per-image exposure and masks."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import torch_ref_photometric as ref
import torch_ref_training_loss as trl
from helpers import FULL_STP, _rel, api_settings, ext_settings, settings_dict

pytestmark = pytest.mark.gpu

TW, TH = ref.tile()
SHAPES = [(3, 1, 1), (3, 7, 5), (3, TH + 1, TW + 1), (3, 2 * TH + 3, 2 * TW + 3), (2, 3, 37, 53)]
GRADS = ((0.8, -0.2, 0.5), (0.35, 1.25, -0.75), (1.0, 0.0, 0.0), (0.0, 1.0, 1.0))   # test_gpu_photometric.GRADS, each with a depth weight
ids = lambda s: "x".join(map(str, s))


def _dgr():
    import diff_gaussian_rasterization as dgr
    return dgr


def dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda().requires_grad_(grad)


@functools.lru_cache(maxsize=None)
def case(shape, clamp, bias=None):
    """One dyadic case, computed once and never modified: x, y, E, mask (float32 arrays), x'' (float32 array, exact), d, m, dmask."""
    x, y, E, mask = trl.dyadic(shape, seed=6, bias=bias)
    x4 = trl.batch4(x)
    xpp64 = trl.exposed(x4, trl.exposure3(E, x4.shape[0]), clamp, trl.batch4(mask))
    xpp = xpp64.to(torch.float32)
    assert torch.equal(xpp.double(), xpp64), "x'' must be exact in float32"
    if clamp and x.size >= 100 and bias is None:   # (three elements cannot be a twentieth at each end and half inside)
        below, above, inside = trl.clamp_fractions(x, E)
        assert below >= 0.05 and above >= 0.05 and inside >= 0.5, (below, above, inside)
    return (x, y, E, mask, xpp.reshape(x.shape).numpy()) + trl.depth_inputs(shape, seed=6)


def plain(xpp, y, g):
    """(out2, g'' = dL/dx'') of the validated path: photometric_terms on x''."""
    image = dev(xpp, True)
    out = _dgr().photometric_terms(image, dev(y))
    (g[0] * out[0] + g[1] * out[1]).backward()
    return out.detach(), image.grad


def fused(x, y, E, clamp, mask, depth=None, g=None):
    """(out3, dL/dimage, dL/dexposure, dL/dinvdepth) of the fused call (the gradients None without g)."""
    image, exposure = dev(x, g is not None), (dev(E, g is not None) if E is not None else None)
    kw = {}
    if depth is not None:
        kw = dict(invdepth=dev(depth[0], g is not None), mono_invdepth=dev(depth[1]), depth_mask=dev(depth[2]) if depth[2] is not None else None)
    out = _dgr().training_terms(image, dev(y), exposure=exposure, clamp=clamp, alpha_mask=dev(mask) if mask is not None else None, **kw)
    assert out.shape == (3,) and out.dtype == torch.float32
    if g is None:
        return out, None, None, None
    (g[0] * out[0] + g[1] * out[1] + g[2] * out[2]).backward()
    return out.detach(), image.grad, exposure.grad if exposure is not None else None, kw["invdepth"].grad if depth is not None else None


def worst(err, bound):
    """The largest err / bound; an error of exactly 0 counts as 0 whatever the bound."""
    err, bound = err.reshape(-1).double().cpu(), bound.reshape(-1).double().cpu()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


# ---- 1. exact inputs: the bits of the validated path -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", (False, True), ids=("noclamp", "clamp"))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_dyadic_inputs_give_the_bits_of_photometric_terms_on_the_exposed_image(shape, clamp):
    x, y, E, mask, xpp, *_ = case(shape, clamp)
    want, _ = plain(xpp, y, (1.0, 0.0))
    out, *_ = fused(x, y, E, clamp, mask)
    print(shape, clamp, out.tolist(), want.tolist())
    assert torch.equal(out[:2], want) and float(out[2]) == 0.0


# ---- 2. gradients against that path, with counted bounds -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_gradients_are_within_the_counted_bounds_of_the_formulas_on_the_plain_gradient(shape):
    x, y, E, mask, xpp, d, m, dmask = case(shape, True)
    x4, mask4 = trl.batch4(x), trl.batch4(mask)
    E3 = trl.exposure3(E, x4.shape[0])
    d64, m64, dm64 = (torch.from_numpy(a).double() for a in (d, m, dmask))
    ratios = {}
    for g in GRADS:
        _, gpp = plain(xpp, y, g)
        out, g_image, g_exposure, g_depth = fused(x, y, E, True, mask, (d, m, dmask), g)
        gpp64 = trl.batch4(gpp)
        dx, dE, _ = trl.chain(gpp64, x4, E3, True, mask4)
        bx, bE = trl.chain_bounds(gpp64, x4, E3, True, mask4)
        g2 = float(np.float32(g[2]))
        bo, bd = trl.depth_bounds(d64, m64, dm64, g2)
        ratios[g] = (worst((trl.batch4(g_image) - dx).abs(), bx), worst((g_exposure.double().cpu().reshape(dE.shape) - dE).abs(), bE),
                     worst((g_depth.double().cpu() - trl.depth_grad(d64, m64, dm64, g2)).abs(), bd),
                     worst((out[2].double().cpu() - trl.depth_term_t(d64, m64, dm64)).abs(), bo))
        assert g_image.shape == x.shape and g_exposure.shape == E.shape and g_depth.shape == d.shape
    print(shape, "worst error / bound (dL/dimage, dL/dexposure, dL/dinvdepth, out[2]) per dL/dout:", {g: "%.3g, %.3g, %.3g, %.3g" % r for g, r in ratios.items()})
    top = max(max(r) for r in ratios.values())
    assert top <= 1.0, f"{shape}: worst error / bound {top:.3g}: {ratios}"


# ---- 3. identity on arbitrary floats -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ("random", "smooth"))
@pytest.mark.parametrize("shape", [(3, TH + 1, TW + 1), (2, 3, 37, 53)], ids=ids)
def test_identity_exposure_and_unit_mask_give_the_plain_bits(shape, family):
    planes = int(np.prod(shape[:-2]))
    x, y = (a.reshape(shape) for a in ref.images(family, planes, *shape[-2:], seed=7))
    B = shape[0] if len(shape) == 4 else 1
    E = np.tile(np.eye(3, 4, dtype=np.float32), (B, 1, 1)).reshape((B, 3, 4) if len(shape) == 4 else (3, 4))
    mask = np.ones(shape[:-3] + (1,) + shape[-2:], np.float32)
    g = GRADS[0]
    want, gpp = plain(x, y, g)
    out, g_image, g_exposure, _ = fused(x, y, E, False, mask, None, g)
    assert torch.equal(out[:2], want) and torch.equal(g_image, gpp)
    x4, gpp64 = trl.batch4(x), trl.batch4(gpp)
    E3 = trl.exposure3(E, B)
    _, dE, _ = trl.chain(gpp64, x4, E3, False, None)
    _, bE = trl.chain_bounds(gpp64, x4, E3, False, None)
    w = worst((g_exposure.double().cpu().reshape(dE.shape) - dE).abs(), bE)
    print(shape, family, "dL/dexposure: worst error / bound %.3g" % w)
    assert w <= 1.0


# ---- 4. the depth term -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_depth_term_value_gradient_and_independence(shape):
    x, y, E, mask, xpp, d, m, dmask = case(shape, True)
    d64, m64, dm64 = (torch.from_numpy(a).double() for a in (d, m, dmask))
    g = (0.0, 0.0, 0.75)
    for mk, mk64 in ((dmask, dm64), (None, None)):
        out, _, _, g_depth = fused(x, y, None, False, None, (d, m, mk), g)   # the term alone
        bo, bd = trl.depth_bounds(d64, m64, mk64, g[2])
        want = trl.depth_grad(d64, m64, mk64, g[2])
        assert worst((out[2].double().cpu() - trl.depth_term_t(d64, m64, mk64)).abs(), bo) <= 1.0
        assert worst((g_depth.double().cpu() - want).abs(), bd) <= 1.0
        zero = (d == m) if mk is None else ((d == m) | (mk == 0))
        assert (zero.any() or d.size < 100) and not g_depth.cpu().numpy()[zero].any()   # exact zeros where d == m or the mask is 0
    colour, *_ = fused(x, y, E, True, mask)
    both, *_ = fused(x, y, E, True, mask, (d, m, dmask))
    alone, *_ = fused(x, y, None, False, None, (d, m, dmask))
    plain_two = _dgr().photometric_terms(dev(x), dev(y))
    assert torch.equal(both[:2], colour[:2]) and torch.equal(both[2], alone[2]) and torch.equal(alone[:2], plain_two) and float(colour[2]) == 0.0


# ---- 5. the halo -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 7, 5), (3, TH + 1, TW + 1)], ids=ids)
def test_halo_outside_the_image_is_zero_not_the_bias(shape):
    """The window's zero padding applies to x'': a halo pixel outside the image is 0, not E[j][3].  With a bias of 0.25 the bit-equality with
    photometric_terms on x'' fails if the outside of the image is staged through the transform (it would be 0.25 there)."""
    for clamp in (False, True):
        x, y, E, mask, xpp, *_ = case(shape, clamp, 0.25)
        assert (E[:, 3] == 0.25).all()
        unmasked = trl.exposed(trl.batch4(x), trl.exposure3(E, 1), clamp).to(torch.float32).reshape(x.shape).numpy()   # (exact, like x'')
        for m, image in ((mask, xpp), (None, unmasked)):
            want, _ = plain(image, y, (1.0, 0.0))
            out, *_ = fused(x, y, E, clamp, m)
            assert torch.equal(out[:2], want), (clamp, m is None)


# ---- 6. rules ----------------------------------------------------------------------------------------------------------------------------------------------
def test_no_extras_is_photometric_terms_bit_for_bit():
    dgr = _dgr()
    x, y = (a.reshape(3, 2 * TH + 3, 2 * TW + 3) for a in ref.images("smooth", 3, 2 * TH + 3, 2 * TW + 3, seed=7))
    a, b = dev(x, True), dev(x, True)
    t3, t2 = dgr.training_terms(a, dev(y)), dgr.photometric_terms(b, dev(y))
    assert torch.equal(t3[:2], t2) and float(t3[2].detach()) == 0.0
    (0.8 * t3[0] - 0.2 * t3[1] + 3.0 * t3[2]).backward()
    (0.8 * t2[0] - 0.2 * t2[1]).backward()
    assert torch.equal(a.grad, b.grad)
    assert torch.equal(dgr.training_loss(a, dev(y)), dgr.photometric_loss(b, dev(y)) + 0.0 * t3[2])
    assert torch.equal(dgr.training_loss(a, dev(y), 0.3, 0.5), (1.0 - 0.3) * t3[0] + 0.3 * (1.0 - t3[1]) + 0.5 * t3[2])


def test_equal_inputs_give_equal_bits():
    x, y, E, mask, xpp, d, m, dmask = case((2, 3, 37, 53), True)
    first = fused(x, y, E, True, mask, (d, m, dmask), GRADS[0])
    for _ in range(2):
        again = fused(x, y, E, True, mask, (d, m, dmask), GRADS[0])
        assert all(torch.equal(a, b) for a, b in zip(first, again))


def test_side_stream_without_host_synchronisation():
    """Issued on a non-default stream with torch's synchronisation check armed: nothing waits for the device or reads a value back."""
    dgr = _dgr()
    x, y, E, mask, xpp, d, m, dmask = case((3, 2 * TH + 3, 2 * TW + 3), True)
    want = fused(x, y, E, True, mask, (d, m, dmask), GRADS[0])
    image, exposure, invdepth = dev(x, True), dev(E, True), dev(d, True)
    target, alpha_mask, mono, depth_mask = dev(y), dev(mask), dev(m), dev(dmask)
    weights = torch.tensor(GRADS[0], device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(side):
            out = dgr.training_terms(image, target, exposure=exposure, clamp=True, alpha_mask=alpha_mask, invdepth=invdepth, mono_invdepth=mono, depth_mask=depth_mask)
            (out * weights).sum().backward()
            loss = dgr.training_loss(image.detach(), target, 0.2, 0.5, exposure=exposure.detach(), clamp=True, alpha_mask=alpha_mask, invdepth=invdepth.detach(),
                                     mono_invdepth=mono, depth_mask=depth_mask)
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    side.synchronize()
    assert torch.equal(out.detach(), want[0]) and torch.equal(image.grad, want[1]) and torch.equal(exposure.grad, want[2]) and torch.equal(invdepth.grad, want[3])
    assert torch.equal(loss, 0.8 * out[0].detach() + 0.2 * (1.0 - out[1].detach()) + 0.5 * out[2].detach())


def test_non_contiguous_inputs_and_none_gradients():
    dgr = _dgr()
    x, y, E, mask, xpp, d, m, dmask = case((3, TH + 1, TW + 1), True)
    want = fused(x, y, E, True, mask, (d, m, dmask), GRADS[0])
    image = dev(x.transpose(1, 2, 0)).permute(2, 0, 1).requires_grad_(True)      # (H, W, C) storage
    exposure = dev(E.T).t().requires_grad_(True)
    invdepth = dev(d.transpose(0, 2, 1)).permute(0, 2, 1).requires_grad_(True)
    alpha_mask = dev(mask[0].T).t()                                              # (H, W), transposed storage
    assert not image.is_contiguous() and not exposure.is_contiguous() and not invdepth.is_contiguous() and not alpha_mask.is_contiguous()
    others = [dev(y, True), alpha_mask.requires_grad_(True), dev(m, True), dev(dmask, True)]   # (requiring grad is accepted; they get none)
    out = dgr.training_terms(image, others[0], exposure=exposure, clamp=True, alpha_mask=others[1], invdepth=invdepth, mono_invdepth=others[2], depth_mask=others[3])
    (GRADS[0][0] * out[0] + GRADS[0][1] * out[1] + GRADS[0][2] * out[2]).backward()
    assert torch.equal(out.detach(), want[0]) and torch.equal(image.grad, want[1]) and torch.equal(exposure.grad, want[2]) and torch.equal(invdepth.grad, want[3])
    assert all(t.grad is None for t in others)


def test_each_option_alone():
    """exposure, clamp and alpha_mask one at a time, against the plain call on the float64-exact x''."""
    x, y, E, mask, *_ = case((3, TH + 1, TW + 1), True)
    for option in ("exposure", "clamp", "alpha_mask"):
        xin = x * np.float32(2.0) if option == "clamp" else x   # (values up to 2: the clamp alone has something to do)
        E_, clamp, mask_ = (E if option == "exposure" else None), option == "clamp", (mask if option == "alpha_mask" else None)
        x64, E64, mask64 = trl.batch4(xin), (trl.exposure3(E_, 1) if E_ is not None else None), (trl.batch4(mask_) if mask_ is not None else None)
        xpp = trl.exposed(x64, E64, clamp, mask64).to(torch.float32).reshape(x.shape).numpy()
        want, gpp = plain(xpp, y, GRADS[0])
        out, g_image, _, _ = fused(xin, y, E_, clamp, mask_, None, GRADS[0])
        assert torch.equal(out[:2], want), option
        dx, _, _ = trl.chain(trl.batch4(gpp), x64, E64, clamp, mask64)
        bx, _ = trl.chain_bounds(trl.batch4(gpp), x64, E64, clamp, mask64)
        assert worst((trl.batch4(g_image) - dx).abs(), bx) <= 1.0, option


def test_one_exposure_and_one_mask_shared_by_a_batch():
    """A (3, 4) exposure and a (1, H, W) mask beside a (B, 3, H, W) image: the bits of the call with both repeated per image; the shared
    exposure's gradient is the sum over the batch, within its counted bound (one chain over all the batch's workgroups)."""
    shape = (2, 3, 37, 53)
    x, y, E, mask, xpp, *_ = case(shape, True)
    E1, mask1 = E[0], mask[0]
    repeated = fused(x, y, np.stack([E1, E1]), True, np.stack([mask1, mask1]), None, GRADS[0])
    shared = fused(x, y, E1, True, mask1, None, GRADS[0])
    assert torch.equal(shared[0], repeated[0]) and torch.equal(shared[1], repeated[1]) and shared[2].shape == (3, 4)
    x4, mask4, E3 = trl.batch4(x), trl.batch4(np.stack([mask1, mask1])), trl.exposure3(E1, 2)
    xpp1 = trl.exposed(x4, E3, True, mask4).to(torch.float32).numpy()
    _, gpp = plain(xpp1, y, GRADS[0])
    _, dE, _ = trl.chain(trl.batch4(gpp), x4, E3, True, mask4)
    _, bE = trl.chain_bounds(trl.batch4(gpp), x4, E3, True, mask4, shared_exposure=True)
    w = worst((shared[2].double().cpu() - dE.sum(0)).abs(), bE.sum(0))
    print("shared exposure: worst error / bound %.3g" % w)
    assert w <= 1.0


def test_refusals_on_the_device():
    dgr = _dgr()
    a, E = torch.rand(3, 8, 8, device="cuda"), torch.eye(3, 4, device="cuda")
    plane = torch.rand(1, 8, 8, device="cuda")
    with pytest.raises(RuntimeError, match="expected float32 tensor, got Half"):
        dgr.training_loss(a.half(), a.half())
    with pytest.raises(RuntimeError, match="image has shape"):
        dgr.training_terms(a, a[:, :7])
    with pytest.raises(RuntimeError, match="expected all tensors on cuda:0, got one on cpu"):
        dgr.training_terms(a, a.cpu())
    with pytest.raises(RuntimeError, match="exposure needs an image of three channels, got C = 2"):
        dgr.training_terms(a[:2], a[:2], exposure=E)
    with pytest.raises(RuntimeError, match=r"exposure must be \(3, 4\)"):
        dgr.training_terms(a, a, exposure=E[:, :3])
    with pytest.raises(RuntimeError, match=r"exposure must be \(3, 4\)"):
        dgr.training_terms(a, a, exposure=E[None].expand(2, 3, 4))
    with pytest.raises(RuntimeError, match="exposure: expected float32 tensor, got Double"):
        dgr.training_terms(a, a, exposure=E.double())
    with pytest.raises(RuntimeError, match="alpha_mask must be .* got"):
        dgr.training_terms(a, a, alpha_mask=plane[:, :7])
    with pytest.raises(RuntimeError, match="invdepth must be .* got"):
        dgr.training_terms(a, a, invdepth=plane[:, :, :7], mono_invdepth=plane[:, :, :7])
    with pytest.raises(RuntimeError, match="depth_mask must be .* got"):
        dgr.training_terms(a, a, invdepth=plane, mono_invdepth=plane, depth_mask=plane[0])
    with pytest.raises(RuntimeError, match="come together or not at all"):
        dgr.training_terms(a, a, invdepth=plane)
    with pytest.raises(RuntimeError, match="come together or not at all"):
        dgr.training_terms(a, a, mono_invdepth=plane)
    with pytest.raises(RuntimeError, match="alpha_mask: expected all tensors on cuda:0, got one on cpu"):
        dgr.training_terms(a, a, alpha_mask=plane.cpu())
    with pytest.raises(RuntimeError, match="stored no derivative maps"):   # (unreachable through training_terms, which asks for the maps whenever a gradient can follow)
        dgr._TrainingTerms.apply(a.clone().requires_grad_(True), a, None, None, None, None, None, False, False).sum().backward()


def test_c_abi_on_a_stream_and_its_launch_counts():
    """The C calls with device pointers on a non-default stream: the documented launch counts (forward 2; backward 1, 2 with dL_dexposure; 0
    for empty work), the binding's bits."""
    from diff_gaussian_rasterization import _C
    L = _C._load()
    shape = (3, TH + 1, TW + 1)
    x, y, E, mask, xpp, d, m, dmask = case(shape, True)
    t = [dev(a) for a in (x, y, E, mask, d, m, dmask)]
    image, target, exposure, alpha_mask, invdepth, mono, depth_mask = t
    weights = torch.tensor(GRADS[0], device="cuda")
    want_out, want_maps = _C.training_loss_forward(image, target, exposure, True, alpha_mask, invdepth, mono, depth_mask, True)
    want = _C.training_loss_backward(image, target, exposure, True, alpha_mask, invdepth, mono, depth_mask, want_maps, weights, True, True)
    floats = L.stp_training_loss_workspace_floats(*shape, 1)
    assert floats == max(2 * 12 + 4, 12 * 12)
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    pod = _C.StpTrainingLoss(exposure=exposure.data_ptr(), alpha_mask=alpha_mask.data_ptr(), invdepth=invdepth.data_ptr(), mono_invdepth=mono.data_ptr(),
                             depth_mask=depth_mask.data_ptr(), clamp=1, exposure_batched=0, alpha_mask_batched=0, channels=3, depth_planes=1)
    out, out_plain = torch.full((3,), -1.0, device="cuda"), torch.full((3,), -1.0, device="cuda")
    maps, workspace = torch.empty(3 * image.numel(), device="cuda"), torch.empty(floats, device="cuda")
    g_image, g_image_only, g_exposure, g_depth = torch.empty_like(image), torch.empty_like(image), torch.empty_like(exposure), torch.empty_like(invdepth)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    st = ctypes.c_void_p(side.cuda_stream)
    fwd, bwd = L.stp_training_loss_forward, L.stp_training_loss_backward
    assert fwd(*shape, p(image), p(target), ctypes.byref(pod), p(out), p(maps), p(workspace), st) == 2
    assert bwd(*shape, p(image), p(target), ctypes.byref(pod), p(maps), p(weights), p(g_image), p(g_exposure), p(g_depth), p(workspace), st) == 2
    assert bwd(*shape, p(image), p(target), ctypes.byref(pod), p(maps), p(weights), p(g_image_only), None, None, None, st) == 1
    assert fwd(*shape, p(image), p(target), None, p(out_plain), None, p(workspace), st) == 2   # no extras: the plain kernels
    assert fwd(0, TH, TW, p(image), p(target), ctypes.byref(pod), p(out), p(maps), p(workspace), st) == 0   # empty work
    assert bwd(3, 0, TW, p(image), p(target), ctypes.byref(pod), p(maps), p(weights), p(g_image), p(g_exposure), p(g_depth), p(workspace), st) == 0
    side.synchronize()
    assert torch.equal(out, want_out) and torch.equal(maps.view_as(want_maps), want_maps)
    assert torch.equal(g_image, want[0]) and torch.equal(g_image_only, want[0]) and torch.equal(g_exposure, want[1]) and torch.equal(g_depth, want[2])
    assert torch.equal(out_plain[:2], _C.photometric_forward(image, target, False)[0]) and float(out_plain[2]) == 0.0


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------------------------------------
def upstream_training_loss(image, invdepth, target, exposure, alpha_mask, mono, depth_mask, lambda_dssim, depth_weight):
    """The official trainer's lines in float32 torch."""
    from test_gpu_photometric import upstream_loss
    image = torch.matmul(image.permute(1, 2, 0), exposure[:3, :3]).permute(2, 0, 1) + exposure[:3, 3, None, None]
    image = image.clamp(0, 1)
    image = image * alpha_mask
    return upstream_loss(image, target, lambda_dssim) + depth_weight * ((invdepth - mono) * depth_mask).abs().mean()


def test_end_to_end_through_the_rasterizer():
    """render (with the inverse depth) -> training_loss with exposure, clamp, mask and depth term -> backward gives the Gaussians and the
    exposure the gradients of the torch composition of upstream's lines on the same render: helpers._rel < 1e-4 (the tolerance of
    test_gpu_photometric's end-to-end test), the loss to 1e-5 relative."""
    dgr = _dgr()
    from diff_gaussian_rasterization import scenes
    sc = scenes.make_scene(P=500, W=64, H=48, sigma_min=1.5, sigma_max=10.0, seed=9)
    device = torch.device("cuda:0")
    es = ext_settings(settings_dict(**FULL_STP))
    es._invdepth = True
    rs = api_settings(sc, es, device)
    names = ("means3D", "opacities", "shs", "scales", "rotations")
    rng = np.random.default_rng(2)
    E0 = torch.tensor([[1.1, 0.05, -0.03, 0.02], [-0.04, 0.95, 0.06, -0.01], [0.02, -0.05, 1.2, 0.03]], device=device)
    alpha_mask = torch.from_numpy((rng.random((1, 48, 64)) > 0.15).astype(np.float32)).to(device)
    depth_mask = torch.from_numpy((rng.random((1, 48, 64)) > 0.3).astype(np.float32)).to(device)
    noise = torch.from_numpy(0.1 * rng.random((3, 48, 64), dtype=np.float32)).to(device)
    depth_noise = torch.from_numpy(rng.random((1, 48, 64), dtype=np.float32)).to(device)

    def grads(fused_path):
        ten = {n: torch.tensor(np.asarray(getattr(sc, n), np.float32), device=device).requires_grad_(True) for n in names}
        means2D = torch.zeros_like(ten["means3D"], requires_grad=True)
        exposure = E0.clone().requires_grad_(True)
        color, _, invdepth = dgr.GaussianRasterizer(rs)(ten["means3D"], means2D, ten["opacities"], shs=ten["shs"], colors_precomp=None, scales=ten["scales"],
                                                        rotations=ten["rotations"], cov3D_precomp=None)
        target = (0.8 * color.detach() + noise).clamp(0.0, 1.0)
        mono = invdepth.detach() * (0.8 + 0.4 * depth_noise)
        if fused_path:
            loss = dgr.training_loss(color, target, 0.2, 0.5, exposure=exposure, clamp=True, alpha_mask=alpha_mask, invdepth=invdepth, mono_invdepth=mono, depth_mask=depth_mask)
        else:
            loss = upstream_training_loss(color, invdepth, target, exposure, alpha_mask, mono, depth_mask, 0.2, 0.5)
        loss.backward()
        out = {n: t.grad.cpu().numpy() for n, t in ten.items()}
        out["exposure"] = exposure.grad.cpu().numpy()
        return color.detach(), float(loss.detach()), out

    color_a, loss_a, fused_g = grads(True)
    color_b, loss_b, composed = grads(False)
    print("loss", loss_a, loss_b, {n: _rel(fused_g[n], composed[n]) for n in composed})
    assert torch.equal(color_a, color_b) and abs(loss_a - loss_b) <= 1e-5 * abs(loss_b)
    assert np.abs(composed["means3D"]).max() > 0 and np.abs(composed["exposure"]).max() > 0
    for n in composed:
        assert _rel(fused_g[n], composed[n]) < 1e-4, (n, _rel(fused_g[n], composed[n]))


def test_trainer_example_with_exposure_ssim_and_depth_term(capsys):
    """examples/train_render.py --loss l1_ssim --exposure --depth-weight: all three go through training_loss; the short fit descends and the
    exposure, which gets its gradient from the fused backward alone, has left the identity."""
    import importlib.util
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_render", os.path.join(root, "examples", "train_render.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    first, last = mod.main(["--iters", "15", "--config", "full", "--points", "3000", "--size", "96", "64", "--loss", "l1_ssim", "--exposure", "--depth-weight", "0.5"])
    assert np.isfinite(first) and np.isfinite(last) and last < first, (first, last)
    moved = re.search(r"exposure: largest deviation from the identity ([0-9.]+)", capsys.readouterr().out)
    assert moved and float(moved.group(1)) > 0.0
