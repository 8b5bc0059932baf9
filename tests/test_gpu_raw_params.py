"""GPU tests (-m gpu) of the raw parameter inputs: GaussianRasterizer(..., raw=), _C.rasterize_gaussians(..., raw=mask),
_C.rasterize_gaussians_backward(..., raw=mask), activate_params (include/stp_raster.h: stp_set_forward_raw_params,
stp_set_backward_raw_params, stp_activate_params).  Frames of 40x36 pixels, P = 293 unless said otherwise.

  1. Forward, to the bit: the raw call against the plain call on activate_params(raw) -- num_rendered, image, radii and every array of the
     geometry buffer -- for P in 1, 255, 256, 257, 300, three sort modes, masks 7, 1, 2, 4 (the inputs of unset bits are fed activated),
     proper_ewa_scaling on and off.  Guards: something is rendered, and the plain call fed the RAW values gives other radii.
  2. activate_params against float64: relative error <= 4 * 2^-23 (expf's one ulp and at most three more roundings of the formulas of
     csrc/stp_activations.h: sigmoid = expf, add, divide; normalize = the norm's chain to within one ulp, divide).
  3. The per-Gaussian half alone on records of the test's (the Frame pattern of tests/test_gpu_per_gaussian.py, phases = 2, NaN rows for
     invisible Gaussians) against tests/torch_ref_raw_params.py: the gradient of every raw input is held to that module's T, every other
     tensor to pg.T of its family.
  4. Autograd end to end through the three Functions and three sort modes: raw leaves with raw=True against the plain call on
     activate_params(raw) whose gradients are carried to the raw leaves by the float64 chain rule; images equal, every gradient
     _rel < 2e-5 (tests/test_gpu_split_sh.py's bound for two whole backwards of one path: float atomics in the render half).
  5. _alpha, _invdepth, _absgrad, _blend_stats and dc= together with raw=True: the four outputs equal to the bit; so are the statistics the
     render half forms without atomics (maximum, count); its float atomic sums (absgrad, the statistics' sum), which the plain call does not
     reproduce bit for bit against itself, are held to the gradients' bound.
  6. The C ABI by ctypes: the refusals name the bit, and the request is one-shot.
  7. examples/train_render.py --raw-params in a child process.

Largest ratio of the kernel per family and tensor of a raw input over the record kinds, measured on MI355X (in brackets the bound,
torch_ref_raw_params.T; plain: with its single-bit masks, P = 1, 256, 257, 549 and every variant):

    family      opacity            scales             rotations
    plain       1.6e-07 (9.6e-07)  1.0e-06 (3.6e-06)  1.2e-06 (4.3e-06)
    clamped     1.4e-07 (9.6e-07)  1.1e-06 (5.9e-06)  9.2e-07 (6.1e-06)
    rawquat     1.3e-07 (9.6e-07)  3.2e-06 (3.1e-05)  2.2e-06 (5.2e-06)
    needles10   1.4e-07 (9.6e-07)  5.0e-06 (1.2e-05)  9.2e-05 (2.2e-04)
    plain_ewa   3.2e-07 (9.6e-07)  1.0e-06 (3.6e-06)  8.9e-07 (4.3e-06)

Every other tensor stayed within pg.T of its family (closest: dL_dcov3D of needles10, 1.3e-04 of 3.1e-04).  activate_params against
float64: at most 1.26 x 2^-23 (rotations), of the 4 x 2^-23 allowed.  Autograd end to end: every gradient within 4.6e-07 of the plain
call's, of the 2e-5 allowed.
"""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers
import torch_ref_per_gaussian as pg
import torch_ref_raw_params as rp
from helpers import FULL_STP, _rel, settings_dict
from diff_gaussian_rasterization import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"global": settings_dict(0), "full_stp": settings_dict(**FULL_STP), "kbuffer16": settings_dict(2, per_pixel=16)}
EIGHT = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")
INPUT = {1: "opacities", 2: "scales", 4: "rotations"}
DEV = "cuda:0"
ULP4 = 4 * 2.0 ** -23


def dev_t(a, rg=False):
    return torch.tensor(np.asarray(a, np.float32), device=DEV).requires_grad_(rg)


@functools.lru_cache(maxsize=None)
def family_and_raw(name, P=pg.BASE_P):
    sc = pg.family(name, P=P)
    return sc, rp.raw_inputs(sc)


def activated(raw):
    """activate_params of the three raw arrays: (scales, rotations, opacities) on the device"""
    import diff_gaussian_rasterization as dgr
    return dgr.activate_params(dev_t(raw["scales"]), dev_t(raw["rotations"]), dev_t(raw["opacities"]))


def mixed_inputs(raw, mask):
    """{name: tensor}: raw where `mask` says so, activate_params' values elsewhere"""
    s, q, o = activated(raw)
    act = {"scales": s, "rotations": q, "opacities": o}
    return {n: dev_t(raw[n]) if mask & bit else act[n] for bit, n in INPUT.items()}, act


def forward(sc, sd, ten, raw=0, **kw):
    from diff_gaussian_rasterization import _C
    empty = torch.Tensor([])
    return _C.rasterize_gaussians(dev_t(sc.bg), dev_t(sc.means3D), empty, ten["opacities"], ten["scales"], ten["rotations"], sc.scale_modifier, empty,
                                  dev_t(sc.viewmatrix), dev_t(sc.projmatrix), dev_t(sc.inv_viewprojmatrix), sc.tanfovx, sc.tanfovy, sc.H, sc.W,
                                  dev_t(sc.shs), sc.sh_degree, dev_t(sc.campos), False, sd, False, False, raw=raw, **kw)


def geometry_rows(geom, P, sd, visible):
    """{name: the rows of visible Gaussians} of every array the buffer has (rows of culled Gaussians are not written by every kernel)"""
    from diff_gaussian_rasterization import _C
    out = {}
    for name in _C._GEOM_TYPES:
        if name == "sh_stash" and not _C.has_sh_stash(geom, P, sd):
            continue
        if name in ("radii", "invz"):   # (the internal radii of a caller that passes none, and 1 / z of the inverse-depth request: not written here)
            continue
        try:
            a = _C.geometry_array(geom, P, sd, name)
        except KeyError:
            continue
        if name in ("tiles_touched", "point_offsets"):
            out[name] = a.clone()
        elif name == "sh_stash":
            out[name] = a.view(9, P)[:, visible].clone()
        else:
            out[name] = a.view(P, -1)[visible].clone()
    return out


# ---- 1. forward, to the bit ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("P", (1, 255, 256, 257, 300))
def test_forward_is_the_plain_call_on_the_activated_copies(P, mode):
    sc, raw = family_and_raw("plain", P)
    for ewa in (False, True):
        sd = dict(MODES[mode], proper_ewa_scaling=ewa)
        for mask in (7, 1, 2, 4):
            ten, act = mixed_inputs(raw, mask)
            a = forward(sc, sd, act)
            b = forward(sc, sd, ten, raw=mask)
            label = (P, mode, ewa, mask)
            assert a[0] == b[0], ("num_rendered",) + label
            assert torch.equal(a[1], b[1]), ("image",) + label
            assert torch.equal(a[2], b[2]), ("radii",) + label
            vis = a[2] > 0
            assert a[0] > 0 and int(vis.sum()) > 0 and float(a[1].abs().max()) > 0, label   # something is rendered
            ga, gb = geometry_rows(a[3], P, sd, vis), geometry_rows(b[3], P, sd, vis)
            assert set(ga) == set(gb) and {"depths", "means2D", "cov3D", "conic_opacity", "rgb", "clamped", "tiles_touched"} <= set(ga)
            for name in ga:
                assert torch.equal(ga[name], gb[name]), (name,) + label
            # a mask that was ignored cannot pass: the plain call on what the raw call was handed gives other radii
            c = forward(sc, sd, ten)
            assert not torch.equal(c[2], a[2]), ("the raw values render like the activated ones",) + label


def test_forward_under_no_grad_and_with_debug(tmp_path, monkeypatch):
    import diff_gaussian_rasterization as dgr
    sc, raw = family_and_raw("plain")
    s, q, o = activated(raw)
    monkeypatch.chdir(tmp_path)
    for debug in (False, True):
        rs = helpers.api_settings(sc, helpers.ext_settings(MODES["full_stp"]), DEV)._replace(debug=debug)
        m = dev_t(sc.means3D)
        with torch.no_grad():
            a = dgr.GaussianRasterizer(rs)(m, torch.zeros_like(m), o, shs=dev_t(sc.shs), scales=s, rotations=q)
            b = dgr.GaussianRasterizer(rs, raw=True)(m, torch.zeros_like(m), dev_t(raw["opacities"]), shs=dev_t(sc.shs), scales=dev_t(raw["scales"]),
                                                     rotations=dev_t(raw["rotations"]))
        assert b[0].grad_fn is None and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and float(a[0].abs().max()) > 0


# ---- 2. activate_params ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("P", (1, 255, 1003))
def test_activate_params_against_float64(P, misaligned):
    import diff_gaussian_rasterization as dgr
    g = torch.Generator().manual_seed(P)
    x_s = torch.rand(P, 3, generator=g) * 15.0 - 10.0
    x_o = torch.rand(P, 1, generator=g) * 15.0 - 10.0
    x_q = torch.randn(P, 4, generator=g)
    x_q = x_q / x_q.norm(dim=1, keepdim=True) * torch.exp(torch.rand(P, 1, generator=g) * 13.8 - 6.9)   # norms in [1e-3, 1e3]
    if P > 4:
        x_q[3] = 0.0
    def put(x):
        if not misaligned:
            return x.to(DEV)
        flat = torch.zeros(x.numel() + 1, device=DEV)
        flat[1:] = x.reshape(-1).to(DEV)
        v = flat[1:].view(x.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 != 0
        return v
    d_s, d_q, d_o = put(x_s).requires_grad_(True), put(x_q).requires_grad_(True), put(x_o).requires_grad_(True)
    s, q, o = dgr.activate_params(d_s, d_q, d_o)
    for got, x in ((s, x_s), (q, x_q), (o, x_o)):
        assert got.shape == x.shape and got.dtype == torch.float32 and got.is_contiguous() and not got.requires_grad and got.grad_fn is None
    x64 = lambda x: x.double()
    ref_s, ref_o, ref_q = rp.act_scale(x64(x_s)), rp.act_opacity(x64(x_o)), rp.act_rotation(x64(x_q))[0]
    for name, got, ref in (("scales", s, ref_s), ("opacities", o, ref_o), ("rotations", q, ref_q)):
        got = got.cpu().double()
        live = ref != 0
        err = float(((got - ref).abs()[live] / ref.abs()[live]).max())
        print(f"\n[activate_params] P {P} misaligned {misaligned} {name}: largest relative error {err / 2.0 ** -23:.2f} x 2^-23")
        assert err <= ULP4, (name, err)
        assert torch.all(got[~live] == 0)
    if P > 4:
        assert torch.all(q[3] == 0)   # a zero quaternion gives zeros
    # absent inputs give None
    only_s = dgr.activate_params(scaling=d_s)
    assert only_s[1] is None and only_s[2] is None and torch.equal(only_s[0], s)
    only_o = dgr.activate_params(opacity=d_o.reshape(-1))
    assert only_o[0] is None and only_o[1] is None and only_o[2].shape == (P,) and torch.equal(only_o[2], o.reshape(-1))
    assert torch.equal(dgr.activate_params(rotation=d_q)[1], q)


# ---- 3. the per-Gaussian half alone -------------------------------------------------------------------------------------------------------------------
class RawFrame:
    """tests/test_gpu_per_gaussian.py's Frame with raw inputs: one forward through _C directly, half() then runs the per-Gaussian half on
    records of the caller's.  The inputs of `mask` are the raw arrays, the others the family's own."""

    def __init__(self, sc, raw, mask, sd, stash=True, layout="cat"):
        from diff_gaussian_rasterization import _C
        self._C, self.sc, self.raw, self.mask = _C, sc, raw, mask
        d = dict(sd, _record_blend_log=True)
        if not stash:
            d["_no_sh_stash"] = True
        self.d = d
        empty = torch.Tensor([])
        ten = {n: dev_t(raw[n] if mask & bit else getattr(sc, n)) for bit, n in INPUT.items()}
        bg, m3, shs = dev_t(sc.bg), dev_t(sc.means3D), dev_t(sc.shs)
        view, proj, inv, cam, w = dev_t(sc.viewmatrix), dev_t(sc.projmatrix), dev_t(sc.inv_viewprojmatrix), dev_t(sc.campos), dev_t(sc.dL_dout)
        self.kw, sh_in = {"raw": mask}, shs
        if layout != "cat":
            dc, rest = shs[:, :1].contiguous(), shs[:, 1:].contiguous()
            if layout == "misaligned":
                pad = lambda x: torch.cat((torch.zeros_like(x[:1]), x))[1:]
                dc, rest = pad(dc), pad(rest)
                assert dc.data_ptr() % 16 != 0
            self.kw["dc"], sh_in = dc, rest
        out = _C.rasterize_gaussians(bg, m3, empty, ten["opacities"], ten["scales"], ten["rotations"], sc.scale_modifier, empty, view, proj, inv,
                                     sc.tanfovx, sc.tanfovy, sc.H, sc.W, sh_in, sc.sh_degree, cam, False, d, False, False, **self.kw)
        R, color, radii, geom, binning, img = out[:6]
        assert _C.has_sh_stash(geom, sc.P, d) == bool(stash)
        self.visible = (radii > 0).cpu().numpy()
        self.args = (bg, m3, radii, ten["opacities"], empty, ten["scales"], ten["rotations"], sc.scale_modifier, empty, view, proj, inv, sc.tanfovx,
                     sc.tanfovy, color, w, sh_in, sc.sh_degree, cam, geom, R, binning, img, d, False)
        self.clamped = _C.geometry_array(geom, sc.P, d, "clamped").view(sc.P, 3).cpu().numpy().astype(bool)

    def half(self, rec, compact=False, camera=False, chunks=None):
        r9 = torch.tensor(pg.with_nan_rows(rec, self.visible), device=DEV)
        if compact:
            partial, bits = r9.contiguous(), 4
        else:
            partial, bits = torch.zeros(self.sc.P, 16, device=DEV), 0
            partial[:, :9] = r9
        kw = dict(self.kw)
        if camera:
            kw["camera_grads"] = True
        if chunks:
            g = None
            for k in range(chunks):
                g = self._C.rasterize_gaussians_backward(*self.args, phases=2 | bits, partial=partial.clone(), chunk=(k, chunks), outputs=g, **kw)
        else:
            g = self._C.rasterize_gaussians_backward(*self.args, phases=2 | bits, partial=partial, **kw)
        out, rest = dict(zip(EIGHT, g[:8])), list(g[8:])
        if camera:
            out.update(dL_dview=rest.pop(0), dL_dproj=rest.pop(0), dL_dcam=rest.pop(0))
        if "dc" in self.kw:
            out["dL_ddc"] = rest.pop(0)
        assert not rest
        out = {n: a.detach().cpu().numpy() for n, a in out.items() if a is not None and a.numel() > 0}
        if "dL_ddc" in out:
            dc, rest_ = out.pop("dL_ddc").reshape(self.sc.P, 1, 3), out.get("dL_dsh", np.zeros((self.sc.P, 0, 3), np.float32))
            out["dL_dsh"] = np.concatenate([dc, rest_.reshape(self.sc.P, -1, 3)], 1)
        return out


def check(label, fr, rec, got, family, min_visible, camera=False):
    """The assertions of one case; prints the largest ratio per tensor.  family: a key of rp.T / pg.T ("plain_ewa": under proper_ewa_scaling)."""
    sc, vis, mask = fr.sc, fr.visible, fr.mask
    P = sc.P
    ewa = rp.split_family(family)[1]
    assert int(vis.sum()) >= min_visible, (label, int(vis.sum()))
    act = rp.activated_scene(sc, fr.raw, mask)
    _, _, clamped = pg.conditions(act, vis)
    assert np.array_equal(fr.clamped[vis], clamped[vis])
    kw = dict(proper_ewa_scaling=ewa, camera_leaves=camera)
    ref, S = rp.reference(sc, fr.raw, mask, rec, vis, key=(label, P, vis.tobytes(), rec.tobytes()), **kw)
    measured = lambda n: n != "dL_dopacity" or ewa or (mask & 1)
    names = [n for n in pg.MEASURED if n in ref and n in got and measured(n)]
    assert {"dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dsh"} <= set(names)
    r = pg.ratios(got, ref, S, names)
    for n in EIGHT:
        if n in got:
            assert np.all(got[n].reshape(P, -1)[~vis] == 0), (label, n)   # invisible Gaussians: exact zeros (their records are NaN)
    r32 = pg.with_nan_rows(rec, vis)
    assert np.array_equal(got["dL_dmeans2D"][vis][:, :2], r32[vis][:, 3:5]) and np.all(got["dL_dmeans2D"][:, 2] == 0)
    if not measured("dL_dopacity"):
        assert np.array_equal(got["dL_dopacity"].reshape(P)[vis], r32[vis][:, 8])   # what the kernel only copies
    if not np.any(rec):
        for n in got:
            assert np.all(got[n] == 0), (label, n)
    bound = lambda n: rp.T[family][n] if mask & rp.TENSOR_BIT.get(n, 0) else pg.T[family][n]
    line = " ".join(f"{n[4:]}{'*' if mask & rp.TENSOR_BIT.get(n, 0) else ''} {v:.1e}/{bound(n):.1e}" for n, v in r.items())
    if camera:
        rc = pg.ratios(got, ref, S, pg.CAMERA)
        line += " | " + " ".join(f"{n[4:]} {v:.1e}" for n, v in rc.items())
        for n in pg.CAMERA:
            assert np.all(np.isfinite(got[n])), (label, n)
            assert rc[n] <= pg.T["camera"][n], (label, n, rc[n])
    print(f"\n[raw per-gaussian] {label} mask {mask}: visible {int(vis.sum())}/{P} | {line}   (*: a raw input, ratio/bound)")
    for n in names:
        assert np.all(np.isfinite(got[n])), (label, n)
        assert r[n] <= bound(n), (label, n, r[n], bound(n))


_frames = {}


def raw_frame(family, mask=7, P=pg.BASE_P, **kw):
    name, ewa = rp.split_family(family)
    key = (family, mask, P, tuple(sorted(kw.items())))
    if key not in _frames:
        sc, raw = family_and_raw(name, P)
        _frames[key] = RawFrame(sc, raw, mask, settings_dict(0, ewa=ewa), **kw)
    return _frames[key]


@pytest.mark.parametrize("kind", ("normal", "wide", "zeros"))
@pytest.mark.parametrize("family", rp.FAMILIES)
def test_families(family, kind):
    fr = raw_frame(family)
    rec = pg.records(kind, fr.sc.P)
    check(f"{family} {kind}", fr, rec, fr.half(rec), family, rp.MIN_VISIBLE)


@pytest.mark.parametrize("mask", (1, 2, 4))
def test_single_bit_masks(mask):
    fr = raw_frame("plain", mask)
    rec = pg.records("normal", fr.sc.P)
    check(f"plain bit {mask}", fr, rec, fr.half(rec), "plain", rp.MIN_VISIBLE)


@pytest.mark.parametrize("P", (1, 256, 257))
def test_sizes(P):
    fr = raw_frame("plain", P=P)
    rec = pg.records("normal", P)
    check(f"plain P={P}", fr, rec, fr.half(rec), "plain", 1)


@pytest.mark.parametrize("variant", ["compact", "camera", "dc", "dc_misaligned", "no_stash", "chunks"])
def test_variants(variant):
    half_kw, frame_kw, P = {}, {}, pg.BASE_P
    if variant == "compact":
        half_kw = dict(compact=True)
    elif variant == "camera":
        half_kw = dict(camera=True)
    elif variant == "dc":
        frame_kw = dict(layout="split")
    elif variant == "dc_misaligned":
        frame_kw = dict(layout="misaligned")
    elif variant == "no_stash":
        frame_kw = dict(stash=False)
    elif variant == "chunks":
        half_kw, P = dict(chunks=3), 549
    fr = raw_frame("plain", P=P, **frame_kw)
    rec = pg.records("normal", P)
    check(f"plain {variant}", fr, rec, fr.half(rec, **half_kw), "plain", rp.MIN_VISIBLE, camera=variant == "camera")


# ---- 4., 5. autograd end to end ------------------------------------------------------------------------------------------------------------------------
def api(sc, raw, sd, use_raw, frozen=(), camera=(), bg_grad=False, extras=False, split=False, flat_opacity=False):
    """Forward + backward through the public API.  use_raw: the raw leaves through a rasterizer made with raw=True; otherwise activate_params(raw).requires_grad_().
    Returns {"out": outputs, name: .grad}; the plain run's gradients of the three activated tensors are carried to the raw leaves by the
    float64 chain rule of tests/torch_ref_raw_params.py ("opacities", "scales", "rotations" then mean the raw leaves in both runs)."""
    import diff_gaussian_rasterization as dgr
    need = lambda n: n not in frozen
    ten = {"means3D": dev_t(sc.means3D, need("means3D"))}
    ten["means2D"] = torch.zeros_like(ten["means3D"], requires_grad=True)
    if use_raw:
        for n in INPUT.values():
            ten[n] = dev_t(raw[n], need(n))
        if flat_opacity:
            ten["opacities"] = dev_t(raw["opacities"].reshape(-1), need("opacities"))
    else:
        s, q, o = activated(raw)
        ten.update(scales=s.requires_grad_(need("scales")), rotations=q.requires_grad_(need("rotations")), opacities=o.requires_grad_(need("opacities")))
    shs = dev_t(sc.shs)
    if split:
        ten["dc"], ten["rest"] = shs[:, :1].contiguous().requires_grad_(True), shs[:, 1:].contiguous().requires_grad_(True)
    else:
        ten["shs"] = shs.requires_grad_(True)
    cam = {n: dev_t(getattr(sc, n), True) for n in camera}
    if bg_grad:
        cam["bg"] = dev_t(sc.bg, True)
    es = helpers.ext_settings(sd)
    if extras:
        es._alpha = es._invdepth = es._absgrad = es._blend_stats = True
    rast = dgr.GaussianRasterizer(helpers.api_settings(sc, es, DEV, **cam), raw=bool(use_raw))
    kw = dict(scales=ten["scales"], rotations=ten["rotations"])
    kw.update(dict(shs=ten["rest"], dc=ten["dc"]) if split else dict(shs=ten["shs"]))
    out = rast(ten["means3D"], ten["means2D"], ten["opacities"], **kw)
    res = {"out": [o_.detach() for o_ in out], "grad_fn": type(out[0].grad_fn).__name__, "saved": out[0].grad_fn.saved_tensors}
    w = dev_t(sc.dL_dout)
    loss = (out[0] * w).sum()
    for k, extra in enumerate(out[2:]):   # alpha, invdepth: weights of their own
        loss = loss + (extra * w[k:k + 1] * (0.5 + k)).sum()
    loss.backward()
    for n, x in list(ten.items()) + list(cam.items()):
        res[n] = None if x.grad is None else x.grad.detach().cpu().double()
    if not use_raw:
        t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
        if res["opacities"] is not None:
            res["opacities"] = rp.vjp_opacity(res["opacities"], t64(raw["opacities"]))
        if res["scales"] is not None:
            res["scales"] = rp.vjp_scale(res["scales"], t64(raw["scales"]))
        if res["rotations"] is not None:
            res["rotations"] = rp.vjp_rotation(res["rotations"], t64(raw["rotations"]))
    res["absgrad"], res["blend_stats"] = getattr(ten["means2D"], "absgrad", None), getattr(ten["means2D"], "blend_stats", None)
    res["inputs"] = ten
    return res


KINDS = {"plain": dict(), "camera": dict(camera=("viewmatrix", "projmatrix", "campos")), "background": dict(bg_grad=True)}
FUNCTION = {"plain": "_RasterizeGaussiansBackward", "camera": "_RasterizeGaussiansCameraBackward", "background": "_RasterizeGaussiansBackgroundBackward"}


def compare_grads(label, a, b, names):
    for n in names:
        assert a[n] is not None and b[n] is not None, n
        x, y = (v.cpu().double().numpy() if isinstance(v, torch.Tensor) else v for v in (b[n], a[n]))
        r = _rel(x, y)
        print(f"{label} {n}: rel {r:.2e}")
        assert r < 2e-5, (label, n, r)
        assert float(np.abs(y).max()) > 0.0 or n == "means2D", n


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_autograd_end_to_end(kind, mode):
    sc, raw = family_and_raw("plain")
    sd = MODES[mode]
    a, b = api(sc, raw, sd, False, **KINDS[kind]), api(sc, raw, sd, True, **KINDS[kind])
    assert a["grad_fn"] == b["grad_fn"] == FUNCTION[kind]
    assert torch.equal(a["out"][0], b["out"][0]) and torch.equal(a["out"][1], b["out"][1])
    P = sc.P
    for n, shape in (("opacities", (P, 1)), ("scales", (P, 3)), ("rotations", (P, 4))):
        assert b["inputs"][n].grad.shape == shape and b["inputs"][n].grad.is_contiguous()
    names = ["means3D", "means2D", "opacities", "scales", "rotations", "shs"] + list(KINDS[kind].get("camera", ())) + (["bg"] if kind == "background" else [])
    compare_grads(f"{kind} {mode}", a, b, names)
    # the raw tensors are what is saved for the backward: no activated copy
    saved = b["saved"]
    for i, n in ((2, "opacities"), (3, "scales"), (4, "rotations")):
        assert saved[i].data_ptr() == b["inputs"][n].data_ptr(), n


@pytest.mark.parametrize("frozen", ["opacities", "scales", "rotations"])
def test_a_frozen_raw_input_gets_no_gradient(frozen):
    sc, raw = family_and_raw("plain")
    sd = MODES["full_stp"]
    a, b = api(sc, raw, sd, False), api(sc, raw, sd, True, frozen=(frozen,))
    assert b[frozen] is None
    compare_grads(f"frozen {frozen}", a, b, [n for n in ("means3D", "opacities", "scales", "rotations", "shs") if n != frozen])


def test_names_and_shapes():
    """raw as an iterable of names (the others are fed activated), and an opacity of shape (P,) gets its gradient in that shape"""
    import diff_gaussian_rasterization as dgr
    sc, raw = family_and_raw("plain")
    sd = MODES["global"]
    a = api(sc, raw, sd, False)
    b = api(sc, raw, sd, True, flat_opacity=True)
    assert b["inputs"]["opacities"].grad.shape == (sc.P,)
    assert _rel(b["opacities"].numpy().reshape(-1), a["opacities"].numpy().reshape(-1)) < 2e-5
    s, q, o = activated(raw)
    m = dev_t(sc.means3D)
    rs = helpers.api_settings(sc, helpers.ext_settings(sd), DEV)
    x = dev_t(raw["scales"], True)
    img, _ = dgr.GaussianRasterizer(rs, raw=("scales",))(m, torch.zeros_like(m), o, shs=dev_t(sc.shs), scales=x, rotations=q)
    assert torch.equal(img.detach(), a["out"][0])
    (img * dev_t(sc.dL_dout)).sum().backward()
    assert _rel(x.grad.cpu().double().numpy(), a["scales"].numpy()) < 2e-5


def test_everything_together():
    """_alpha, _invdepth, _absgrad, _blend_stats and dc= with raw=True"""
    sc, raw = family_and_raw("plain")
    sd = MODES["full_stp"]
    a, b = api(sc, raw, sd, False, extras=True, split=True), api(sc, raw, sd, True, extras=True, split=True)
    assert len(a["out"]) == len(b["out"]) == 4
    for x, y in zip(a["out"], b["out"]):
        assert torch.equal(x, y)
    # absgrad's two columns and the statistics' sum are float atomic sums of the render half: the plain call does not reproduce its own bits
    # in them from one run to the next (measured on MI355X, plain against plain: 6 to 26 of 293 rows differ, by up to 7.1e-08 of the largest
    # entry; plain against raw: the same figures).  What the render half computes without atomics is equal to the bit -- the maximum, the
    # count, absgrad's zero column -- and the sums are held to the bound of the gradients, which come from the same atomics.
    assert torch.equal(a["blend_stats"][:, 1:], b["blend_stats"][:, 1:]) and torch.equal(a["absgrad"][:, 2], b["absgrad"][:, 2])
    for name, x, y in (("absgrad", a["absgrad"][:, :2], b["absgrad"][:, :2]), ("blend_stats sum", a["blend_stats"][:, 0], b["blend_stats"][:, 0])):
        r = _rel(y.cpu().numpy(), x.cpu().numpy())
        print(f"extras {name}: rel {r:.2e}")
        assert r < 2e-5, (name, r)
    assert float(a["absgrad"].abs().max()) > 0 and float(a["blend_stats"].abs().max()) > 0
    compare_grads("extras", a, b, ["means3D", "means2D", "opacities", "scales", "rotations", "dc", "rest"])


# ---- 6. the C ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_and_one_shot():
    from diff_gaussian_rasterization import _C
    L = _C._load()
    sc, raw = family_and_raw("plain")
    sd = MODES["global"]
    _, act = mixed_inputs(raw, 0)
    before = forward(sc, sd, act)
    alloc_t = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
    called = []
    alloc = alloc_t(lambda user, n: called.append(n))   # (returns NULL; a refused call never asks)
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.stp_forward.argtypes = [alloc_t, vp] * 3 + [ci] * 3 + [vp, ci, ci, ctypes.POINTER(_C.StpSettings)] + [vp] * 5 + [cf] + [vp] * 6 + [cf, cf, ci, vp, vp, ci, vp]
    L.stp_forward.restype = ci
    s = _C.settings_from_dict(sd)
    keep = [dev_t(sc.bg), dev_t(sc.means3D), dev_t(sc.shs), dev_t(sc.viewmatrix), dev_t(sc.projmatrix), dev_t(sc.inv_viewprojmatrix), dev_t(sc.campos),
            torch.zeros(3, sc.H, sc.W, device=DEV), dev_t(scenes.covariance_from_scale_rotation(sc))]
    bg, m3, shs, view, proj, inv, cam, out, cov = (t.data_ptr() for t in keep)
    stream = torch.cuda.current_stream().cuda_stream

    def call(scales, rotations, cov3D):
        return L.stp_forward(alloc, None, alloc, None, alloc, None, sc.P, sc.sh_degree, sc.shs.shape[1], bg, sc.W, sc.H, ctypes.byref(s), m3, shs, None,
                             act["opacities"].data_ptr(), scales, sc.scale_modifier, rotations, cov3D, view, proj, inv, cam, sc.tanfovx, sc.tanfovy, 0,
                             out, None, 0, stream)
    sp, qp = act["scales"].data_ptr(), act["rotations"].data_ptr()
    L.stp_set_forward_raw_params(8)
    assert call(sp, qp, None) == -1 and "outside 0..7" in L.stp_last_error().decode()   # STP_ERR_INVALID_ARGUMENT
    L.stp_set_forward_raw_params(6)
    assert call(None, None, cov) == -1
    msg = L.stp_last_error().decode()
    assert "bit 1 (scales)" in msg and "NULL" in msg
    L.stp_set_forward_raw_params(4)
    assert call(sp, None, cov) == -1 and "bit 2 (rotations)" in L.stp_last_error().decode()
    assert not called                                   # refused before any allocation or launch
    torch.cuda.synchronize()
    # one-shot: each request was consumed by the call that refused it -- the next plain forward renders what it always rendered
    after = forward(sc, sd, act)
    assert after[0] == before[0] and torch.equal(after[1], before[1]) and torch.equal(after[2], before[2])
    # ... and a request is consumed by the forward that honours it, too
    ten, _ = mixed_inputs(raw, 7)
    r = forward(sc, sd, ten, raw=7)
    assert torch.equal(r[1], before[1])
    again = forward(sc, sd, act)
    assert torch.equal(again[1], before[1]) and torch.equal(again[2], before[2])


# ---- 7. the example -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--split-sh", "--optimizer", "sparse_adam", "--strategy", "adc"], ["--strategy", "mcmc"]],
                         ids=["plain", "split-sparse_adam-adc", "mcmc"])
def test_example_trains_with_raw_params(extra):
    """examples/train_render.py --raw-params in a child process: render() hands _scaling, _rotation and _opacity over with raw=True; the short
    fit still descends (the split-SH example test's condition)."""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_render.py"), "--raw-params", "--iters", "15", "--points", "3000", "--size", "96", "64"] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=170)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    m = re.search(r"^\S.* ([0-9.eE+-]+) -> ([0-9.eE+-]+); depth visualisation", p.stdout, re.M)
    assert m, p.stdout[-2000:]
    first, last = float(m.group(1)), float(m.group(2))
    assert last < 0.8 * first, (first, last)
