"""CPU tests of the training loss (training_terms, training_loss; include/stp_raster.h: stp_training_loss_forward / _backward): the float64
yardstick tests/torch_ref_training_loss.py against autograd of the plainly written composition and a hand-computed case, its bounds against
the same formulas in float32 (inside, with a factor 2 to spare) and against five broken versions (outside), the dyadic family's promises,
the Python surface and what it refuses, the C ABI's declarations, exports and argument validation (which runs before any launch, so without
a GPU), and the loader's message for a library without the symbols."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import torch_ref_photometric as ref
import torch_ref_training_loss as trl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 3, 37, 53)
G = (0.8, -0.2, 0.5)

_cache = {}


def _case():
    """The dyadic batch at SHAPE with its float64 tensors and plain gradient g'': computed once, shared, never modified."""
    if not _cache:
        x, y, E, mask = trl.dyadic(SHAPE, seed=6)
        d, m, dmask = trl.depth_inputs(SHAPE, seed=6)
        t = {k: trl.batch4(v) for k, v in dict(x=x, y=y, mask=mask, d=d, m=m, dmask=dmask).items()}
        t["E"] = trl.exposure3(E, 2)
        t["xpp"] = trl.exposed(t["x"], t["E"], True, t["mask"])
        t["gpp"] = ref.grad(t["xpp"].float().numpy(), y, G[0], G[1]).reshape(SHAPE)
        t["out_bound"], _ = ref.bounds(t["xpp"].float().numpy(), y, G[0], G[1])
        _cache.update(t)
    return _cache


def _worst(err, bound):
    err, bound = torch.as_tensor(err).reshape(-1), torch.as_tensor(bound).reshape(-1)
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


def upstream_lines(image, gt, exposure, alpha_mask, invdepth, mono, depth_mask):
    """The official trainer's lines for one image, plainly: -> (x'', depth term)."""
    image = torch.matmul(image.permute(1, 2, 0), exposure[:3, :3]).permute(2, 0, 1) + exposure[:3, 3, None, None]
    image = image.clamp(0, 1)
    image = image * alpha_mask
    return image, ((invdepth - mono) * depth_mask).abs().mean()


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------------------
def test_yardstick_is_autograd_of_the_plain_composition():
    """Values and the three closed-form gradients against float64 autograd of upstream's lines, image by image of a batch with per-image
    exposure: 1e-12 relative, as the photometric yardstick's own test."""
    rng = np.random.default_rng(5)
    B, H, W = 2, 16, 70
    x = torch.from_numpy(rng.uniform(-0.2, 1.2, (B, 3, H, W))).requires_grad_(True)
    y, mask = torch.from_numpy(rng.random((B, 3, H, W))), torch.from_numpy(rng.random((B, 1, H, W)))
    E = (torch.eye(3, 4, dtype=torch.float64)[None] + torch.from_numpy(rng.uniform(-0.2, 0.2, (B, 3, 4)))).requires_grad_(True)
    d = torch.from_numpy(rng.random((B, 1, H, W))).requires_grad_(True)
    m, dmask = torch.from_numpy(rng.random((B, 1, H, W))), torch.from_numpy(rng.random((B, 1, H, W)))
    images, depth_terms = zip(*[upstream_lines(x[b], y[b], E[b], mask[b], d[b], m[b], dmask[b]) for b in range(B)])
    xpp = torch.stack(images)
    two = ref.terms_t(xpp.reshape(-1, 1, H, W), y.reshape(-1, 1, H, W))
    plain = torch.cat([two, torch.stack(depth_terms).mean()[None]])
    out = trl.terms_t(x, y, E, True, mask, d, m, dmask)
    assert float((out - plain).detach().abs().max()) <= 1e-12
    (G[0] * plain[0] + G[1] * plain[1] + G[2] * plain[2]).backward()
    gpp = _gpp64(xpp.detach(), y)
    dx, dE, _ = trl.chain(gpp, x.detach(), E.detach(), True, mask)
    dd = trl.depth_grad(d.detach(), m, dmask, G[2])
    for closed, auto in ((dx, x.grad), (dE, E.grad), (dd, d.grad)):
        assert float((closed - auto).abs().max()) <= 1e-12 * float(auto.abs().max())


def _gpp64(xpp, y):
    """dL/dx'' by float64 autograd of the photometric terms (ref.grad rounds its inputs to float32 first; these are arbitrary doubles)."""
    xpp = xpp.clone().requires_grad_(True)
    two = ref.terms_t(xpp.reshape(-1, 1, *xpp.shape[-2:]), y.reshape(-1, 1, *y.shape[-2:]))
    (G[0] * two[0] + G[1] * two[1]).backward()
    return xpp.grad


def test_yardstick_on_a_hand_computed_case():
    """One pixel: x = (0.5, 0.25, 0.75), E rows = input channels, mask 0.5."""
    x = torch.tensor([0.5, 0.25, 0.75], dtype=torch.float64).reshape(1, 3, 1, 1)
    E = torch.tensor([[[1.0, 0.25, 0.0, 0.125], [0.0, 1.5, -0.25, -0.25], [0.5, 0.0, 1.0, 0.25]]], dtype=torch.float64)
    # v_0 = 0.5 * 1 + 0.25 * 0 + 0.75 * 0.5 + 0.125 = 1.0;  v_1 = 0.5 * 0.25 + 0.25 * 1.5 + 0 - 0.25 = 0.25;  v_2 = 0 - 0.0625 + 0.75 + 0.25 = 0.9375
    assert trl.pre_clamp(x, E).reshape(-1).tolist() == [1.0, 0.25, 0.9375]
    E[0, 0, 3] = 0.375   # v_0 = 1.25: clamped
    mask = torch.full((1, 1, 1, 1), 0.5, dtype=torch.float64)
    assert trl.exposed(x, E, True, mask).reshape(-1).tolist() == [0.5, 0.125, 0.46875]
    assert trl.exposed(x, E, False, mask).reshape(-1).tolist() == [0.625, 0.125, 0.46875]
    y = torch.tensor([0.25, 0.25, 0.5], dtype=torch.float64).reshape(1, 3, 1, 1)
    d, m, dm = (torch.full((1, 1, 1, 1), v, dtype=torch.float64) for v in (0.5, 0.75, 0.5))
    out = trl.terms_t(x, y, E, True, mask, d, m, dm)
    assert float(out[0]) == (0.25 + 0.125 + 0.03125) / 3 and float(out[2]) == 0.125
    # the L1 term alone: g'' = sign(x'' - y) / 3 = (1, -1, -1) / 3; g' = g'' * 0.5 where the clamp passes (not channel 0)
    gpp = torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64).reshape(1, 3, 1, 1) / 3
    dx, dE, g = trl.chain(gpp, x, E, True, mask)
    assert g.reshape(-1).tolist() == [0.0, -0.5 / 3, -0.5 / 3]
    assert dx.reshape(-1).tolist() == [0.25 * (-0.5 / 3) + 0.0, 1.5 * (-0.5 / 3) + -0.25 * (-0.5 / 3), 1.0 * (-0.5 / 3)]
    assert dE[0, :, 3].tolist() == [0.0, -0.5 / 3, -0.5 / 3] and dE[0, :, 1].tolist() == [0.5 * (-0.5 / 3), 0.25 * (-0.5 / 3), 0.75 * (-0.5 / 3)]
    assert float(trl.depth_grad(d, m, dm, 2.0)) == -1.0 and float(trl.depth_grad(d, d, dm, 2.0)) == 0.0


def test_dyadic_family_keeps_its_promises():
    for shape in ((3, 7, 5), (3, 17, 65), SHAPE):
        x, y, E, mask = trl.dyadic(shape, seed=6)
        assert x.dtype == np.float32 and x.shape == shape and E.shape == ((2, 3, 4) if len(shape) == 4 else (3, 4))
        for a, q in ((x, 256.0), (E, 64.0), (mask, 16.0)):
            assert np.array_equal(a * q, np.round(a * q))
        assert x.min() == 0.0 and x.max() == 1.0 and (mask == 0).mean() >= 0.1 and mask.max() <= 1.0
        below, above, inside = trl.clamp_fractions(x, E)
        assert below >= 0.05 and above >= 0.05 and inside >= 0.5, (shape, below, above, inside)
        for clamp in (False, True):
            xpp = trl.exposed(trl.batch4(x), trl.exposure3(E, 2 if len(shape) == 4 else 1), clamp, trl.batch4(mask))
            assert torch.equal(xpp.float().double(), xpp)
            # the kernel's chain in float32 gives the same bits
            x32, E32 = torch.from_numpy(x).reshape(-1, 3, *shape[-2:]), torch.from_numpy(E).reshape(-1, 3, 4)
            v = E32[:, None, None, :, 3].permute(0, 3, 1, 2).expand(-1, -1, *shape[-2:]).clone()
            for i in range(3):
                v = torch.addcmul(v, E32[:, i, :3][:, :, None, None], x32[:, i][:, None])
            if clamp:
                v = v.clamp(0, 1)
            assert torch.equal((v * torch.from_numpy(mask).reshape(-1, 1, *shape[-2:])).double(), xpp)


# ---- the bounds: wide enough for float32, too tight for a wrong formula -------------------------------------------------------------------------------
def test_float32_composition_stays_inside_the_bounds():
    """The chain formulas and the depth term in float32 torch on the CPU: inside every counted bound with a factor 2 to spare."""
    c = _case()
    f = lambda t: t.float()
    gpp32 = f(c["gpp"]).double()   # (the kernels start from the float32 g'')
    dx64, dE64, _ = trl.chain(gpp32, c["x"], c["E"], True, c["mask"])
    bx, bE = trl.chain_bounds(gpp32, c["x"], c["E"], True, c["mask"])
    dx32, dE32, _ = trl.chain(f(gpp32), f(c["x"]), f(c["E"]), True, f(c["mask"]))
    g2 = float(np.float32(G[2]))
    bo, bd = trl.depth_bounds(c["d"], c["m"], c["dmask"], g2)
    worst = [_worst((dx32.double() - dx64).abs(), bx), _worst((dE32.double() - dE64).abs(), bE),
             _worst((trl.depth_grad(f(c["d"]), f(c["m"]), f(c["dmask"]), g2).double() - trl.depth_grad(c["d"], c["m"], c["dmask"], g2)).abs(), bd),
             _worst((trl.depth_term_t(f(c["d"]), f(c["m"]), f(c["dmask"])).double() - trl.depth_term_t(c["d"], c["m"], c["dmask"])).abs(), bo)]
    print("worst error / bound: dL/dimage %.3g, dL/dexposure %.3g, dL/dinvdepth %.3g, out[2] %.3g" % tuple(worst))
    assert max(worst) <= 0.5, worst
    # the forward on the dyadic family: float32 x'' IS the float64 one
    assert torch.equal(trl.exposed(f(c["x"]), f(c["E"]), True, f(c["mask"])).double(), c["xpp"])


@pytest.mark.parametrize("mutation", ["E used transposed", "mask applied before the exposure", "halo filled with the bias", "clamp's gradient passed everywhere",
                                      "depth mask applied twice in the gradient"])
def test_mutated_versions_fall_outside_the_bounds(mutation):
    """Float64 evaluations of a WRONG formula on the dyadic family: the bounds (and the bit-equalities they stand beside) are not vacuous."""
    c = _case()
    gpp32 = c["gpp"].float().double()
    planes = lambda t: t.reshape(-1, 1, *t.shape[-2:])
    right = ref.terms_t(planes(c["xpp"]), planes(c["y"]))
    dx, dE, _ = trl.chain(gpp32, c["x"], c["E"], True, c["mask"])
    bx, bE = trl.chain_bounds(gpp32, c["x"], c["E"], True, c["mask"])
    if mutation in ("E used transposed", "mask applied before the exposure"):
        switch = dict(transpose=True) if "transposed" in mutation else dict(mask_first=True)
        wrong_xpp = trl.exposed(c["x"], c["E"], True, c["mask"], **switch)
        assert not torch.equal(wrong_xpp, c["xpp"])
        wrong = ref.terms_t(planes(wrong_xpp), planes(c["y"]))
        assert _worst((wrong - right).abs(), c["out_bound"]) > 1.0
        if "transposed" in mutation:
            g = trl.chain(gpp32, c["x"], c["E"], True, c["mask"])[2]
            wrong_dx = torch.einsum("bjhw,bji->bihw", g, c["E"][:, :, :3])
            assert _worst((wrong_dx - dx).abs(), bx) > 1.0
    elif mutation == "halo filled with the bias":
        wrong = trl.halo_bias_terms(c["x"], c["y"], c["E"], True)
        right_unmasked = ref.terms_t(planes(trl.exposed(c["x"], c["E"], True)), planes(c["y"]))
        assert float(wrong[0]) == float(right_unmasked[0]) and _worst((wrong - right_unmasked).abs()[1:], c["out_bound"][1:]) > 1.0
    elif mutation == "clamp's gradient passed everywhere":
        wrong_dx, wrong_dE, _ = trl.chain(gpp32, c["x"], c["E"], True, c["mask"], clamp_passes_all=True)
        assert _worst((wrong_dx - dx).abs(), bx) > 1.0 and _worst((wrong_dE - dE).abs(), bE) > 1.0
    else:
        _, bd = trl.depth_bounds(c["d"], c["m"], c["dmask"], G[2])
        wrong = trl.depth_grad(c["d"], c["m"], c["dmask"], G[2], mask_twice=True)
        assert _worst((wrong - trl.depth_grad(c["d"], c["m"], c["dmask"], G[2])).abs(), bd) > 1.0


def test_chain_lengths():
    TW, TH = ref.tile()
    assert trl.tiles_of(TH + 1, TW + 1) == 4 and trl.exposure_chain(4) == 4 + 6 + 3 + 1 + 6 + 3 and trl.exposure_chain(257) == 24


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------------------------
def test_names_are_exported():
    import diff_gaussian_rasterization as dgr
    for name in ("training_terms", "training_loss"):
        assert name in dgr.__all__ and callable(getattr(dgr, name))


def test_cpu_tensors_have_no_path():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    a, E, p = torch.rand(3, 8, 8), torch.eye(3, 4), torch.rand(1, 8, 8)
    for call in (lambda: dgr.training_terms(a, a), lambda: dgr.training_loss(a, a, 0.2, 0.5, exposure=E, clamp=True, alpha_mask=p, invdepth=p, mono_invdepth=p, depth_mask=p),
                 lambda: dgr.training_loss(a.clone().requires_grad_(True), a, exposure=E),
                 lambda: _C.training_loss_forward(a, a, E, True, p, p, p, p, True),
                 lambda: _C.training_loss_backward(a, a, E, True, p, p, p, p, torch.zeros(3, 3, 8, 8), torch.zeros(3), True, True)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_refusals():
    """Each a RuntimeError, raised before anything is looked at on a device: 3j's texts for image and target, the extras' own after them."""
    import diff_gaussian_rasterization as dgr
    a, E, p = torch.rand(3, 8, 8), torch.eye(3, 4), torch.rand(1, 8, 8)
    for fn in (dgr.training_terms, dgr.training_loss):
        with pytest.raises(RuntimeError, match="expected float32 tensor, got Double"):
            fn(a.double(), a.double())
        with pytest.raises(RuntimeError, match=r"image has shape \[3, 8, 8\], target has \[3, 8, 7\]"):
            fn(a, a[:, :, :7])
        with pytest.raises(RuntimeError, match=r"must be \(C, H, W\) or \(B, C, H, W\), got 2 dimensions"):
            fn(a[0], a[0])
        with pytest.raises(RuntimeError, match="exposure needs an image of three channels, got C = 2"):
            fn(a[:2], a[:2], exposure=E)
        with pytest.raises(RuntimeError, match=r"exposure must be \(3, 4\) or, with a \(B, 3, H, W\) image, \(B, 3, 4\), got \[4, 3\]"):
            fn(a, a, exposure=E.t())
        with pytest.raises(RuntimeError, match=r"exposure must be \(3, 4\)"):
            fn(a[None], a[None], exposure=E[None].expand(2, 3, 4))
        with pytest.raises(RuntimeError, match="exposure: expected float32 tensor, got Half"):
            fn(a, a, exposure=E.half())
        with pytest.raises(RuntimeError, match=r"alpha_mask must be \(H, W\), \(1, H, W\) or \(B, 1, H, W\) with the image's H = 8, W = 8, got \[1, 8, 7\]"):
            fn(a, a, alpha_mask=p[:, :, :7])
        with pytest.raises(RuntimeError, match="alpha_mask of 2 images beside an image batch of 1"):
            fn(a[None], a[None], alpha_mask=p[None].expand(2, 1, 8, 8))
        with pytest.raises(RuntimeError, match=r"invdepth must be \(1, H, W\) or \(B, 1, H, W\) .* got \[8, 8\]"):
            fn(a, a, invdepth=p[0], mono_invdepth=p[0])
        with pytest.raises(RuntimeError, match=r"mono_invdepth must be .* got \[1, 7, 8\]"):
            fn(a, a, invdepth=p, mono_invdepth=p[:, :7])
        with pytest.raises(RuntimeError, match="depth_mask: expected float32 tensor, got Bool"):
            fn(a, a, invdepth=p, mono_invdepth=p, depth_mask=p > 0.5)
        with pytest.raises(RuntimeError, match="invdepth and mono_invdepth come together or not at all"):
            fn(a, a, invdepth=p)
        with pytest.raises(RuntimeError, match="invdepth and mono_invdepth come together or not at all"):
            fn(a, a, mono_invdepth=p)
        with pytest.raises(RuntimeError, match="depth_mask without invdepth"):
            fn(a, a, depth_mask=p)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(a, a, exposure=E, alpha_mask=p, invdepth=p, mono_invdepth=p)
    with pytest.raises(TypeError):
        dgr.training_terms(a, a, E)   # the extras are keyword-only


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("stp_training_loss_workspace_floats", "stp_training_loss_forward", "stp_training_loss_backward")


def test_header_declares_the_calls_and_the_struct():
    h = open(os.path.join(ROOT, "include", "stp_raster.h")).read()
    assert int(re.search(r"#define\s+STP_ABI_VERSION\s+(\d+)\b", h).group(1)) == 7
    assert "fma(E[2][j], x_2, fma(E[1][j], x_1, fma(E[0][j], x_0, E[j][3])))" in h   # the chain the tests rest on, stated
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    struct = re.search(r"typedef\s+struct\s+StpTrainingLoss\s*\{(.*?)\}\s*StpTrainingLoss\s*;", h, re.S).group(1)
    fields = re.findall(r"(const\s+float\s*\*|int32_t)\s*(\w+)\s*;", struct)
    from diff_gaussian_rasterization import _C
    assert [n for _, n in fields] == [n for n, _ in _C.StpTrainingLoss._fields_]
    assert all((t == "int32_t") == (c is ctypes.c_int32) for (t, _), (_, c) in zip(fields, _C.StpTrainingLoss._fields_))
    assert re.search(r"size_t\s+stp_training_loss_workspace_floats\s*\(\s*int\s+planes\s*,\s*int\s+H\s*,\s*int\s+W\s*,\s*int\s+depth_planes\s*\)\s*;", h)
    assert re.search(r"int\s+stp_training_loss_forward\s*\(\s*int\s+planes\s*,\s*int\s+H\s*,\s*int\s+W\s*,\s*const\s+float\s*\*\s*image\s*,\s*const\s+float\s*\*\s*target\s*,"
                     r"\s*const\s+StpTrainingLoss\s*\*\s*extras\s*,\s*float\s*\*\s*out3\s*,\s*float\s*\*\s*maps\s*,\s*float\s*\*\s*workspace\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)
    assert re.search(r"int\s+stp_training_loss_backward\s*\(\s*int\s+planes\s*,\s*int\s+H\s*,\s*int\s+W\s*,\s*const\s+float\s*\*\s*image\s*,\s*const\s+float\s*\*\s*target\s*,"
                     r"\s*const\s+StpTrainingLoss\s*\*\s*extras\s*,\s*const\s+float\s*\*\s*maps\s*,\s*const\s+float\s*\*\s*dL_dout3\s*,\s*float\s*\*\s*dL_dimage\s*,"
                     r"\s*float\s*\*\s*dL_dexposure\s*,\s*float\s*\*\s*dL_dinvdepth\s*,\s*float\s*\*\s*workspace\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)
    src = open(os.path.join(ROOT, "stopthepop-rasterization_amd", "csrc", "stp_loss.hip")).read()
    assert "fma(E[2][j], x_2, fma(E[1][j], x_1, fma(E[0][j], x_0, E[j][3])))" in src


def test_library_exports_the_calls_and_the_abi_stays_7():
    from diff_gaussian_rasterization import _C
    L = _C._load()
    assert L.stp_abi_version() == 7
    nm = subprocess.run(["nm", "-D", "--defined-only", _C.library_path()], capture_output=True, text=True).stdout
    for name in SYMBOLS:
        assert hasattr(L, name) and _C._require(name) is not None
        assert re.search(r" T %s$" % name, nm, re.M)
        assert _C._SYMBOL_FEATURE[name] == "the training loss"
    assert callable(_C._native().training_loss_forward) and callable(_C._native().training_loss_backward)
    exports = open(os.path.join(ROOT, "stopthepop-rasterization_amd", "csrc", "host", "stp_exports.h")).read()
    for name in SYMBOLS:
        assert re.search(r'X\(%s, false, "the training loss"\)' % name[len("stp_"):], exports)


def test_loader_message_for_a_library_without_the_symbols(monkeypatch):
    from diff_gaussian_rasterization import _C
    import diff_gaussian_rasterization as dgr
    monkeypatch.setattr(_C, "_lib", types.SimpleNamespace())   # a loaded library that predates the exports
    for name in SYMBOLS:
        with pytest.raises(RuntimeError) as ex:
            _C._require(name)
        assert str(ex.value) == f"{_C.library_path()} does not export {name} (a library built before the training loss): rebuild it"
    z = torch.zeros(3, 4, 4)
    with pytest.raises(RuntimeError, match="does not export stp_training_loss_"):
        dgr.training_loss(z, z)
    with pytest.raises(RuntimeError, match="does not export stp_training_loss_backward"):
        _C.training_loss_backward(z, z, None, False, None, None, None, None, torch.zeros(3, 3, 4, 4), torch.zeros(3), False, False)


def test_c_abi_validates_before_any_launch():
    """The refusals come before the first launch, so they need no GPU; the pointers are never followed (they are host addresses here)."""
    from diff_gaussian_rasterization import _C
    L = _C._load()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    err = lambda: L.stp_last_error().decode()
    pod = lambda **kw: ctypes.byref(_C.StpTrainingLoss(**kw))
    full = dict(exposure=a, alpha_mask=a, invdepth=a, mono_invdepth=a, depth_mask=a, clamp=1, channels=3, depth_planes=1)
    fwd = lambda planes, H, W, x, image=a, out=a, ws=a: L.stp_training_loss_forward(planes, H, W, image, a, x, out, a, ws, None)
    bwd = lambda planes, H, W, x, maps=a, dE=None, dD=None, ws=a: L.stp_training_loss_backward(planes, H, W, a, a, x, maps, a, a, dE, dD, ws, None)
    assert fwd(-1, 4, 4, None) == -1 and "negative size" in err()
    assert bwd(3, 4, -4, pod(**full)) == -1 and "negative size" in err()
    assert fwd(2, 32768, 32768, None) == -1 and ">= 2^31" in err()
    assert fwd(3, 4, 4, pod(**dict(full, depth_planes=2 ** 30))) == -1 and ">= 2^31" in err()
    assert fwd(3, 4, 4, pod(**dict(full, depth_planes=-1))) == -1 and "negative size" in err()
    assert fwd(3, 4, 4, pod(**dict(full, clamp=2))) == -1 and "must be 0 or 1" in err()
    assert fwd(4, 4, 4, pod(**full)) == -1 and "exposure needs three channels" in err()
    assert fwd(3, 4, 4, pod(**dict(full, channels=1))) == -1 and "exposure needs three channels" in err()
    assert fwd(3, 4, 4, pod(alpha_mask=a, channels=2)) == -1 and "no multiple of channels" in err()
    assert fwd(3, 4, 4, pod(**dict(full, mono_invdepth=None))) == -1 and "come together" in err()
    assert bwd(3, 4, 4, pod(**dict(full, invdepth=None))) == -1 and "come together" in err()
    assert fwd(3, 4, 4, pod(depth_mask=a)) == -1 and "without invdepth" in err()
    assert fwd(3, 4, 4, pod(**dict(full, depth_planes=0))) == -1 and "depth_planes = 0" in err()
    assert bwd(3, 4, 4, None, dE=a) == -1 and "dL_dexposure without exposure" in err()
    assert bwd(3, 4, 4, pod(exposure=a), dD=a) == -1 and "dL_dinvdepth without invdepth" in err()
    assert fwd(3, 4, 4, pod(**full), image=None) == -1 and "null pointer" in err()
    assert fwd(3, 4, 4, None, out=None) == -1 and "null pointer" in err()
    assert fwd(3, 4, 4, pod(**full), ws=None) == -1 and "null pointer" in err()
    assert bwd(3, 4, 4, pod(**full), maps=None) == -1 and "null maps" in err()
    assert bwd(3, 4, 4, pod(**full), dE=a, ws=None) == -1 and "null pointer" in err()
    # empty work: no launch, 0, nothing touched
    assert fwd(0, 4, 4, None, image=None, out=None, ws=None) == 0 and fwd(3, 0, 4, pod(**full)) == 0 and fwd(3, 4, 0, None) == 0
    assert bwd(0, 4, 4, None, maps=None) == 0 and bwd(3, 0, 4, pod(**full), dE=a, dD=a) == 0 and bwd(3, 4, 0, pod(**full)) == 0
    assert all(v == 0.0 for v in buf)
    TW, TH = ref.tile()
    ws = L.stp_training_loss_workspace_floats
    assert ws(3, 1, 1, 0) == 36 and ws(3, TH + 1, TW + 1, 1) == 144 and ws(1, 5, 3 * TW - 1, 40) == 126
    assert ws(0, 4, 4, 0) == 0 and ws(3, 4, 4, -1) == 0 and ws(2, 32768, 32768, 0) == 0 and ws(3, 4, 4, 2 ** 30) == 0


def test_argument_check_program(tmp_path):
    """tests/cpp/training_loss_args_check.cpp: the same refusals and empty calls from a stand-alone C++ program, built with the command line
    of tests/cpp/Makefile's rule for api_smoke.bin (compiler, flags, include and library paths), into a temporary directory."""
    lib = os.path.join(ROOT, "stopthepop-rasterization_amd", "diff_gaussian_rasterization")
    exe = str(tmp_path / "training_loss_args_check.bin")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "training_loss_args_check.cpp"), "-o", exe, "-L", lib, "-lstp_raster", f"-Wl,-rpath,{lib}"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"ok \d+\n", r.stdout) and int(r.stdout.split()[1]) >= 45
