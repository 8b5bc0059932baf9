"""CPU tests of the raw parameter inputs (GaussianRasterizer's raw=; include/stp_raster.h: stp_set_forward_raw_params,
stp_set_backward_raw_params, stp_activate_params): the float64 yardstick's three VJPs against torch.autograd, its tolerance table measured
again, the C ABI's declarations, exports and refusals that need no device, the public signature, and the Python refusals, which are raised
before any device work.

Float32 evaluation of tests/torch_ref_raw_params.py, worst ratio per family over pg's four record kinds, measured on the CPU (not numbers of
the kernel):

    family      opacity  scales   rotations
    plain       1.4e-07  8.8e-07  1.1e-06
    clamped     1.6e-07  1.5e-06  1.5e-06
    rawquat     1.3e-07  7.5e-06  1.3e-06
    needles10   1.4e-07  2.9e-06  5.3e-05
    plain_ewa   2.3e-07  8.8e-07  1.1e-06
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import torch_ref_per_gaussian as pg
import torch_ref_raw_params as rp
from helpers import FULL_STP, settings_dict
from diff_gaussian_rasterization import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("stp_set_forward_raw_params", "stp_set_backward_raw_params", "stp_activate_params")


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------------------
def test_vjps_equal_autograd_in_float64():
    g = torch.Generator().manual_seed(3)
    P = 64
    x = (torch.rand(P, 3, generator=g, dtype=torch.float64) * 15.0 - 10.0).requires_grad_(True)
    up = torch.randn(P, 3, generator=g, dtype=torch.float64)
    for fn, vjp in ((torch.exp, rp.vjp_scale), (torch.sigmoid, rp.vjp_opacity)):
        ref, = torch.autograd.grad((fn(x) * up).sum(), x)
        got = vjp(up, x.detach())
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), fn
        assert float((fn(x.detach()) - (rp.act_scale if fn is torch.exp else rp.act_opacity)(x.detach())).abs().max()) <= 1e-12 * float(fn(x.detach()).abs().max())
    q = torch.randn(P, 4, generator=g, dtype=torch.float64) * torch.exp(torch.rand(P, 1, generator=g, dtype=torch.float64) * 13.8 - 6.9)
    q[5] = torch.tensor([3e-13, -2e-13, 1e-13, 4e-13], dtype=torch.float64)   # |q| < 1e-12: the clamp is active
    q[9] = 0.0                                                               # exactly zero
    q.requires_grad_(True)
    up = torch.randn(P, 4, generator=g, dtype=torch.float64)
    out = torch.nn.functional.normalize(q, dim=-1)
    ref, = torch.autograd.grad((out * up).sum(), q)
    got = rp.vjp_rotation(up, q.detach())
    assert torch.all(torch.isfinite(ref)) and torch.all(torch.isfinite(got))
    rows = (got - ref).abs().max(1).values / ref.abs().max(1).values
    assert float(rows.max()) <= 1e-12
    assert torch.equal(got[5], up[5] / 1e-12) and torch.equal(got[9], up[9] / 1e-12)
    qh, n = rp.act_rotation(q.detach())
    assert float((qh - out.detach()).abs().max()) <= 1e-12 and torch.all(qh[9] == 0) and float(n[5]) < 1e-12


def test_raw_inputs_invert_the_activations():
    sc = pg.family("rawquat")
    raw = rp.raw_inputs(sc)
    act = rp.activated_scene(sc, raw)
    for name in ("scales", "opacities"):
        a, b = np.asarray(getattr(act, name), np.float64), np.asarray(getattr(sc, name), np.float64)
        assert np.max(np.abs(a - b) / np.abs(b)) < 5e-7, name       # one float32 rounding of the logarithm / logit
    q = np.asarray(sc.rotations, np.float64)
    assert np.max(np.abs(act.rotations - q / np.linalg.norm(q, axis=1, keepdims=True))) < 2e-7
    norms = np.linalg.norm(raw["rotations"].astype(np.float64), axis=1) / np.linalg.norm(q, axis=1)
    assert norms.min() >= 0.5 - 1e-6 and norms.max() <= 3.0 + 1e-6 and norms.std() > 0.3
    # a mask leaves the other inputs the scene's own
    one = rp.activated_scene(sc, raw, mask=2)
    assert one.rotations is sc.rotations and one.opacities is sc.opacities and one.scales is not sc.scales


def test_table_conditions():
    assert set(rp.T) == set(rp.FAMILIES)
    for fam, row in rp.T.items():
        assert set(row) == set(rp.TENSOR_BIT), fam
        for n, t in row.items():
            assert pg.FLOOR <= t <= pg.CAP, (fam, n, t)
            assert pg.tolerance(t / 4) == pytest.approx(t, rel=1e-12)   # two significant digits


@pytest.mark.parametrize("name", rp.FAMILIES)
def test_float32_evaluation_stays_within_the_table(name):
    """the stored table covers the measurement made here, by pg's rule (tests/test_per_gaussian_cpu.py)"""
    worst, n_vis = rp.measure_float32(name)
    print(f"\n{name}: {n_vis} visible, float32 worst ratio " + " ".join(f"{n[4:]} {v:.1e}" for n, v in worst.items()))
    assert n_vis >= rp.MIN_VISIBLE
    assert set(worst) == set(rp.TENSOR_BIT)
    for n, v in worst.items():
        assert v <= rp.T[name][n] / 4 * 1.25, (n, v)


def test_single_bit_masks_touch_their_tensor_only():
    sc = pg.family("plain")
    raw = rp.raw_inputs(sc)
    vis, _ = rp.visible_and_conditions(sc, raw, False)
    rec = pg.records("normal", sc.P)
    for n, bit in rp.TENSOR_BIT.items():
        act = rp.activated_scene(sc, raw, bit)
        plain = pg.vjp(act, rec, vis, kernel=True)
        ref, S = rp.reference(sc, raw, bit, rec, vis)
        for m in plain:
            assert np.array_equal(ref[m], plain[m]) == (m != n), (n, m)
        assert np.all(S[n][~vis] == 0) and np.all(S[n][vis] > 0)


# ---- the C ABI without a device --------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_three_calls():
    h = open(os.path.join(ROOT, "include", "stp_raster.h")).read()
    assert int(re.search(r"#define\s+STP_ABI_VERSION\s+(\d+)\b", h).group(1)) == 7
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"void\s+stp_set_forward_raw_params\s*\(\s*int\s+mask\s*\)\s*;", h)
    assert re.search(r"void\s+stp_set_backward_raw_params\s*\(\s*int\s+mask\s*\)\s*;", h)
    assert re.search(r"int\s+stp_activate_params\s*\(\s*int\s+P\s*,\s*const\s+float\s*\*\s*scaling\s*,\s*const\s+float\s*\*\s*rotation\s*,\s*const\s+float\s*\*\s*opacity\s*,"
                     r"\s*float\s*\*\s*scales\s*,\s*float\s*\*\s*rotations\s*,\s*float\s*\*\s*opacities\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)
    x = open(os.path.join(ROOT, "stopthepop-rasterization_amd", "csrc", "host", "stp_exports.h")).read()
    for name in SYMBOLS:
        assert re.search(rf'X\({name[4:]}, false, "raw parameter inputs"\)', x), name


@pytest.mark.parametrize("lib", ["libstp_raster.so", "libstp_raster_fma.so"])
def test_both_libraries_export_the_three_calls(lib):
    from diff_gaussian_rasterization import _C
    path = os.path.join(os.path.dirname(_C.library_path()), lib)
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in SYMBOLS:
        assert name in exported, (lib, name)


def test_requests_are_checked_and_consumed_without_a_device():
    """A mask outside 0..7 and a bit whose array is NULL are refused on the request itself, naming the bit; the per-Gaussian call consumes
    the backward request whatever its outcome, a render-only call (phases = 1) leaves it pending; mask 0 clears."""
    from diff_gaussian_rasterization import _C
    L = _C._load()
    for name in SYMBOLS:
        assert hasattr(L, name) and _C._require(name) is not None
    call = lambda phases: L.stp_backward_phases(*([ctypes.c_int(phases)] + [ctypes.c_int(0)] * 4 + [None] * 35))
    err = lambda: L.stp_last_error().decode()
    L.stp_set_backward_raw_params(8)
    assert call(2) < 0 and "raw parameters" in err() and "outside 0..7" in err()
    assert call(2) < 0 and "raw parameters" not in err()          # consumed: the next call fails on its null settings
    for mask, word in ((1, "bit 0 (opacities)"), (2, "bit 1 (scales)"), (4, "bit 2 (rotations)"), (6, "bit 1 (scales)")):
        L.stp_set_backward_raw_params(mask)
        assert call(3) < 0 and "raw parameters" in err() and word in err(), mask
    L.stp_set_backward_raw_params(2)
    assert call(1) < 0 and "raw parameters" not in err()          # render-only: neither checked nor consumed ...
    assert call(2) < 0 and "bit 1 (scales)" in err()              # ... the per-Gaussian call finds it
    L.stp_set_backward_raw_params(2)
    L.stp_set_backward_raw_params(0)                               # mask 0 clears
    assert call(2) < 0 and "raw parameters" not in err()
    L.stp_set_forward_raw_params(5)
    L.stp_set_forward_raw_params(0)
    # stp_activate_params: refusals and the empty calls launch nothing
    buf = (ctypes.c_float * 4)()
    assert L.stp_activate_params(0, buf, None, None, buf, None, None, None) == 0
    assert L.stp_activate_params(0, None, None, None, None, None, None, None) == 0
    assert L.stp_activate_params(-1, None, None, None, None, None, None, None) < 0 and "negative P" in err()
    assert L.stp_activate_params(1, buf, None, None, None, None, None, None) < 0 and "together" in err()
    assert L.stp_activate_params(1 << 29, None, None, None, None, None, None, None) < 0 and "2^29" in err()


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------------------
def test_signatures():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C, tile_shard
    # raw is a keyword of the two constructors, their last; forward()'s signature stays the reference's plus dc (tests/test_split_sh_cpu.py)
    for cls in (dgr.GaussianRasterizer, tile_shard.TileRowShardedRasterizer):
        params = list(inspect.signature(cls.__init__).parameters.values())
        assert params[-1].name == "raw" and params[-1].default is False
        assert "raw" not in inspect.signature(cls.forward).parameters
    assert list(inspect.signature(dgr.GaussianRasterizer.__init__).parameters) == ["self", "raster_settings", "raw"]
    # the binding's wrappers: a keyword behind the positional arguments, in front of dc
    for fn, positional in ((_C.rasterize_gaussians, 22), (_C.rasterize_gaussians_backward, 25)):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-2].name == "raw" and params[-2].default == 0
        assert sum(p.default is inspect.Parameter.empty for p in params) == positional
    p = list(inspect.signature(dgr.rasterize_gaussians).parameters.values())[-1]
    assert p.name == "raw" and p.default == 0
    assert list(inspect.signature(dgr.activate_params).parameters) == ["scaling", "rotation", "opacity"]
    assert "activate_params" in dgr.__all__ and callable(_C.activate_params)
    assert dgr.activate_params() == (None, None, None)


def test_mask_of_the_raw_argument():
    from diff_gaussian_rasterization import _raw_mask
    o, s, q = object(), object(), object()
    assert _raw_mask(False, o, s, q) == 0 and _raw_mask(None, o, s, q) == 0 and _raw_mask((), o, s, q) == 0 and _raw_mask([], o, s, q) == 0
    assert _raw_mask(True, o, s, q) == 7 and _raw_mask(True, o, None, None) == 1
    assert _raw_mask(("opacities",), o, s, q) == 1 and _raw_mask(["scales"], o, s, q) == 2 and _raw_mask({"rotations"}, o, s, q) == 4
    assert _raw_mask(("rotations", "opacities"), o, s, q) == 5 and _raw_mask("scales", o, s, q) == 2
    assert _raw_mask(iter(("scales", "rotations", "opacities")), o, s, q) == 7


def _cpu_call(sc, raw, cov3D=False, sharded=False, spy=None):
    """The public forward on CPU tensors: a refusal that needs no device is raised before the binding asks for a GPU tensor."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import tile_shard
    t = lambda a: torch.tensor(np.asarray(a, np.float32))
    rs = dgr.GaussianRasterizationSettings(
        image_height=sc.H, image_width=sc.W, tanfovx=sc.tanfovx, tanfovy=sc.tanfovy, bg=t(sc.bg), scale_modifier=sc.scale_modifier,
        viewmatrix=t(sc.viewmatrix), projmatrix=t(sc.projmatrix), inv_viewprojmatrix=t(sc.inv_viewprojmatrix), sh_degree=sc.sh_degree,
        campos=t(sc.campos), prefiltered=False, settings=dgr.ExtendedSettings.from_dict(settings_dict(**FULL_STP)), render_depth=False,
        debug=False)
    m = t(sc.means3D)
    kw = {} if raw == "absent" else {"raw": raw}
    r = tile_shard.TileRowShardedRasterizer(rs, None, 0, 1, **kw) if sharded else dgr.GaussianRasterizer(rs, **kw)
    geo = dict(cov3D_precomp=t(scenes.covariance_from_scale_rotation(sc))) if cov3D else dict(scales=t(sc.scales), rotations=t(sc.rotations))
    return r(m, torch.zeros_like(m), t(sc.opacities), shs=t(sc.shs), **geo)


def tiny():
    return scenes.make_scene(P=40, W=48, H=32, sigma_min=1.0, sigma_max=9.0, seed=4)


def test_refusals_are_raised_before_any_device_work():
    sc = tiny()
    with pytest.raises(RuntimeError, match=r"raw: unknown name 'scale'"):
        _cpu_call(sc, ("opacities", "scale"))
    with pytest.raises(RuntimeError, match=r"raw: 'scales' is named but no scales are given"):
        _cpu_call(sc, ("scales",), cov3D=True)
    with pytest.raises(RuntimeError, match=r"raw: 'rotations' is named but no rotations are given"):
        _cpu_call(sc, ["opacities", "rotations"], cov3D=True)
    with pytest.raises(RuntimeError, match=r"raw must be True, False or an iterable of names.*got int"):
        _cpu_call(sc, 7)
    with pytest.raises(RuntimeError, match=r"raw=.*not wired through the tile-row shard"):
        _cpu_call(sc, True, sharded=True)
    with pytest.raises(RuntimeError, match=r"raw=.*not wired through the tile-row shard"):
        _cpu_call(sc, ("opacities",), sharded=True)
    # well-formed requests pass the checks and reach the binding, which has no CPU path
    for raw, cov in ((True, False), (("scales", "rotations"), False), (True, True), (("opacities",), True)):
        with pytest.raises(RuntimeError, match=r"needs tensors on a GPU device"):
            _cpu_call(sc, raw, cov3D=cov)
    # ... and so does the sharded rasterizer without a request (False, an empty iterable): it is not refused for raw=
    for raw in (False, ()):
        with pytest.raises(Exception) as ex:
            _cpu_call(sc, raw, sharded=True)
        assert "raw=" not in str(ex.value)


@pytest.mark.parametrize("raw", ["absent", False, (), None])
def test_no_request_takes_the_route_it_always_took(monkeypatch, raw):
    """raw=False and raw=() hand the Function the ten inputs it always received, the caller's own settings tuple among them: no mask rides along."""
    import diff_gaussian_rasterization as dgr
    seen = {}

    def spy(*args):
        seen["args"] = args
        raise RuntimeError("stop here")
    monkeypatch.setattr(dgr._RasterizeGaussians, "apply", staticmethod(spy))
    with pytest.raises(RuntimeError, match="stop here"):
        _cpu_call(tiny(), raw)
    assert len(seen["args"]) == 10 and seen["args"][9] is None
    assert type(seen["args"][8]) is dgr.GaussianRasterizationSettings and not hasattr(seen["args"][8], "raw_mask")


@pytest.mark.parametrize("raw, mask", [(True, 7), (("scales",), 2), (["rotations", "opacities"], 5)])
def test_a_request_rides_on_the_settings_tuple(monkeypatch, raw, mask):
    import diff_gaussian_rasterization as dgr
    seen = {}

    def spy(*args):
        seen["args"] = args
        raise RuntimeError("stop here")
    monkeypatch.setattr(dgr._RasterizeGaussians, "apply", staticmethod(spy))
    with pytest.raises(RuntimeError, match="stop here"):
        _cpu_call(tiny(), raw)
    rs = seen["args"][8]
    assert len(seen["args"]) == 10 and seen["args"][9] is None and isinstance(rs, dgr.GaussianRasterizationSettings) and rs.raw_mask == mask
    assert rs.image_height == 32 and rs.image_width == 48 and rs.debug is False and len(rs) == 15   # (the caller's fields, in their places)


def test_activate_params_refusals_without_a_device():
    import diff_gaussian_rasterization as dgr
    with pytest.raises(RuntimeError, match=r"activate_params: scaling must be \(5, 3\)"):
        dgr.activate_params(scaling=torch.zeros(5, 4))
    with pytest.raises(RuntimeError, match=r"activate_params: rotation must be \(5, 4\)"):
        dgr.activate_params(scaling=torch.zeros(5, 3), rotation=torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match=r"activate_params: opacity: expected float32"):
        dgr.activate_params(opacity=torch.zeros(5, 1, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"activate_params: scaling: .*needs tensors on a GPU device"):
        dgr.activate_params(scaling=torch.zeros(5, 3))
