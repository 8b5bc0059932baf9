"""GPU tests (-m gpu) of the per-Gaussian backward ALONE (csrc/stp_backward.hip: preprocess_backward_kernel) against a float64 yardstick,
Gaussian by Gaussian.

Each case is one forward through _C.rasterize_gaussians (the geometry buffer then holds radii, cov3D, the clamp bytes and, where asked, the
SH stash) followed by phases=2 on gradient records the TEST made: the kernel's rows are compared with tests/torch_ref_per_gaussian.py,
which differentiates the same per-Gaussian map in float64 (vjp) and supplies each row's scale S (scale).  The measure is
ratio = max over the row |got - float64| / S, the bound T[family][tensor] of that module: 4 x what the module itself reaches when it is
evaluated in float32 on the CPU (tests/test_per_gaussian_cpu.py measures it again) -- never a number of the kernel.  No summation order
and no threshold of the render half enters; the two decisions the kernel itself takes in float32 (the 1.3 tan_fov band, the colour clamp)
are kept 1e-4 away from every visible Gaussian by an assertion on the inputs.

What runs: eleven input families x four record kinds + the render half's own records, at P = 293 (a full 256-row workgroup on the unrolled
48-float route and a tail of 37), and 1, 256, 257; on two families with N(0,1) records the kernel's variants, each against the yardstick
(their mutual bit equality is tested elsewhere): M and the active degree, precomputed colours, concatenated / split / misaligned split SH,
the stash and the legacy path, padded and compact records, cov3D_precomp, proper_ewa_scaling, camera gradients, and a chunked half at
P = 549.  The inverse-depth request is left out (the binding wants both halves in one call with it; tests/test_gpu_invdepth.py has a
float64 yardstick of its own).  Last, the convention check: the render half's records of a low-density frame against the float64
cotangents of the same intermediates, which pins the NDC units and the halved conic-xy slot against something other than the kernel's
own second half.

Largest ratio of the kernel per family and tensor, measured on MI355X (the bounds: torch_ref_per_gaussian.T):

    family       means3D  scales   rotations sh       cov3D    opacity
    plain        1.4e-06  1.0e-06  2.5e-06   3.4e-07  8.5e-07  (copied)
    clamped      6.6e-07  1.0e-06  1.1e-06   3.3e-07  6.5e-07
    subpixel     1.9e-06  1.2e-06  8.5e-07   3.9e-07  6.2e-07
    huge         1.5e-06  1.2e-06  1.9e-06   3.6e-07  8.2e-07
    needles10    3.6e-05  6.7e-05  7.7e-05   3.7e-07  6.7e-05
    needles24    3.1e-04  5.6e-04  4.9e-04   3.7e-07  5.6e-04
    offband      1.6e-06  1.5e-06  3.0e-06   3.5e-07  1.0e-06
    rawquat      1.9e-05  1.6e-05  1.6e-05   3.8e-07  1.7e-05
    fxfy         1.3e-06  1.3e-06  4.1e-06   3.6e-07  1.2e-06
    near         1.2e-06  1.3e-06  1.7e-06   3.6e-07  1.6e-06
    far          1.6e-06  1.1e-06  8.3e-06   4.0e-07  1.2e-06
    plain_ewa    3.3e-07  8.4e-07  7.6e-07   3.4e-07  6.4e-07  1.5e-07
    clamped_ewa  3.1e-07  5.3e-07  6.5e-07   3.2e-07  5.6e-07  1.8e-07
    camera       view 2.2e-08  proj 1.6e-08  campos 1.8e-08   (bound 9.6e-07)

Closest to its bound: dL_dcov3D of rawquat, 1.7e-05 of 1.8e-05 (the covariance the kernel differentiates is the forward's float32
R S^2 R^T of a quaternion of norm up to 3); then dL_drotations of plain, 2.5e-06 of 5.2e-06; every other entry uses less than half of its
bound.  (plain / clamped: the family's five record kinds, P = 1, 256, 257, 549 and every variant.)  Records of the render half against the
float64 cotangents: colour 2.5e-07, mean2D 5.2e-06, conic 2.3e-07, opacity 3.5e-07.

One-line mutations of the kernel, in a scratch copy of the library: x_grad_mul forced to 1 fails offband x {normal, oneslot, wide, real};
dsh[45 + ch] * 1.001 fails all 77 cases with active degree 3; the + 0.0000001f of denom2inv removed fails subpixel x {normal, oneslot, wide,
real}.  The rest of the gpu suite notices the first (40 tests of the camera gradients and the camera model) and the second (239 tests, against
the oracle, the reference and the yardsticks) and passes on the third.
"""
import numpy as np
import pytest
import torch

import torch_ref
import torch_ref_per_gaussian as pg
from helpers import FULL_STP, _rel, settings_dict
from diff_gaussian_rasterization import scenes

pytestmark = pytest.mark.gpu

EIGHT = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")
GLOBAL, FULL = settings_dict(0), settings_dict(**FULL_STP)
MIN_VISIBLE = 200   # of 293, tests/test_per_gaussian_cpu.py


class Frame:
    """One forward through _C directly; half() then runs the per-Gaussian half on records of the caller's."""

    def __init__(self, sc, sd, stash=True, layout="cat", cov3D=None):
        from diff_gaussian_rasterization import _C
        self._C, self.sc = _C, sc
        d = dict(sd, _record_blend_log=True)
        if not stash:
            d["_no_sh_stash"] = True
        self.d = d
        empty, dev = torch.Tensor([]), torch.device("cuda:0")
        t = lambda a: empty if a is None else torch.tensor(np.asarray(a, np.float32), device=dev)
        bg, m3, op = t(sc.bg), t(sc.means3D), t(sc.opacities)
        sca, rot = (empty, empty) if cov3D is not None else (t(sc.scales), t(sc.rotations))
        shs, colors, cov = t(sc.shs), t(sc.colors_precomp), t(cov3D)
        view, proj, inv, cam, w = t(sc.viewmatrix), t(sc.projmatrix), t(sc.inv_viewprojmatrix), t(sc.campos), t(sc.dL_dout)
        self.kw, sh_in = {}, shs
        if layout != "cat":
            dc, rest = shs[:, :1].contiguous(), shs[:, 1:].contiguous()
            if layout == "misaligned":
                pad = lambda x: torch.cat((torch.zeros_like(x[:1]), x))[1:]
                dc, rest = pad(dc), pad(rest)
                assert dc.data_ptr() % 16 != 0
            self.kw["dc"], sh_in = dc, rest
        out = _C.rasterize_gaussians(bg, m3, colors, op, sca, rot, sc.scale_modifier, cov, view, proj, inv, sc.tanfovx, sc.tanfovy, sc.H, sc.W,
                                     sh_in, sc.sh_degree, cam, False, d, False, False, **self.kw)
        R, color, radii, geom, binning, img = out[:6]
        if sc.shs is not None:
            assert _C.has_sh_stash(geom, sc.P, d) == bool(stash)
        self.visible = (radii > 0).cpu().numpy()
        self.args = (bg, m3, radii, op, colors, sca, rot, sc.scale_modifier, cov, view, proj, inv, sc.tanfovx, sc.tanfovy,
                     color, w, sh_in, sc.sh_degree, cam, geom, R, binning, img, d, False)
        self.clamped = _C.geometry_array(geom, sc.P, d, "clamped").view(sc.P, 3).cpu().numpy().astype(bool)

    def render_records(self):
        """(P, 9) float32: the render half's own records of this frame"""
        return self._C.rasterize_gaussians_backward(*self.args, phases=1)[:, :9].cpu().numpy()

    def half(self, rec, compact=False, camera=False, chunks=None):
        """{name: numpy array} of the per-Gaussian half on records rec (P, 9); rows of invisible Gaussians are handed over as NaN"""
        r9 = torch.tensor(pg.with_nan_rows(rec, self.visible), device="cuda:0")
        if compact:
            partial, bits = r9.contiguous(), 4
        else:
            partial, bits = torch.zeros(self.sc.P, 16, device="cuda:0"), 0
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
        if "dL_ddc" in out:   # the two slices of the concatenated gradient
            dc, rest_ = out.pop("dL_ddc").reshape(self.sc.P, 1, 3), out.get("dL_dsh", np.zeros((self.sc.P, 0, 3), np.float32))
            out["dL_dsh"] = np.concatenate([dc, rest_.reshape(self.sc.P, -1, 3)], 1)
        return out


def check(label, fr, rec, got, table, min_visible, ewa=False, cov3D=False, camera=False):
    """The assertions of one case; prints the largest ratio per tensor."""
    sc, vis = fr.sc, fr.visible
    P = sc.P
    assert int(vis.sum()) >= min_visible, (label, int(vis.sum()))
    out_x, out_y, clamped = pg.conditions(sc, vis)
    if sc.shs is not None:
        assert np.array_equal(fr.clamped[vis], clamped[vis])   # the forward took the float64 decision on every visible channel
    kw = dict(proper_ewa_scaling=ewa, use_cov3D_precomp=cov3D, camera_leaves=camera)
    key = (label, P, vis.tobytes(), rec.tobytes())
    ref, S = pg.reference(sc, rec, vis, key=key, **kw)
    names = [n for n in pg.MEASURED if n in ref and (n != "dL_dopacity" or ewa)]
    assert set(names) <= set(got)
    r = pg.ratios(got, ref, S, names)
    # rows of invisible Gaussians: exact zeros in every output (the records there are NaN)
    for n in EIGHT:
        if n in got:
            assert np.all(got[n].reshape(P, -1)[~vis] == 0), (label, n)
    # what the kernel only copies
    r32 = pg.with_nan_rows(rec, vis)
    assert np.array_equal(got["dL_dmeans2D"][vis][:, :2], r32[vis][:, 3:5]) and np.all(got["dL_dmeans2D"][:, 2] == 0)
    if "dL_dcolors" in got:
        assert np.array_equal(got["dL_dcolors"][vis], r32[vis][:, :3])
    if not ewa:
        assert np.array_equal(got["dL_dopacity"].reshape(P)[vis], r32[vis][:, 8])
    if "dL_dsh" in got:
        assert np.all(got["dL_dsh"].reshape(P, -1, 3)[:, (sc.sh_degree + 1) ** 2:] == 0)
    if not np.any(rec):   # all-zero records: every output row is exactly zero
        for n in got:
            assert np.all(got[n] == 0), (label, n)
    line = " ".join(f"{n[4:]} {v:.1e}" for n, v in r.items())
    if camera:
        rc = pg.ratios(got, ref, S, pg.CAMERA)
        line += " | " + " ".join(f"{n[4:]} {v:.1e}" for n, v in rc.items())
        for n in pg.CAMERA:
            assert np.all(np.isfinite(got[n])), (label, n)
            assert rc[n] <= pg.T["camera"][n], (label, n, rc[n])
        assert np.all(got["dL_dview"].reshape(4, 4)[:, 3] == 0) and np.all(got["dL_dproj"].reshape(4, 4)[:, 2] == 0)
    print(f"\n[per-gaussian] {label}: visible {int(vis.sum())}/{P} | {line}")
    for n in names:
        assert r[n] <= table[n], (label, n, r[n], table[n])
    return out_x, out_y, clamped


_frames = {}


def _family_frame(name, P=pg.BASE_P):
    if (name, P) not in _frames:
        _frames[name, P] = Frame(pg.family(name, P=P), GLOBAL)
    return _frames[name, P]


# ---- the families x the record kinds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pg.KINDS + ("real",))
@pytest.mark.parametrize("name", pg.FAMILIES)
def test_families(name, kind):
    fr = _family_frame(name)
    rec = fr.render_records() if kind == "real" else pg.records(kind, fr.sc.P)
    if kind == "real":
        rec = np.where(fr.visible[:, None], rec, 0.0).astype(np.float32)
        assert np.all(np.isfinite(rec)) and np.count_nonzero(np.abs(rec).sum(1)) >= 10
    out_x, out_y, clamped = check(f"{name} {kind}", fr, rec, fr.half(rec), pg.T[name], MIN_VISIBLE)
    if name in ("plain", "clamped"):
        assert int((~fr.visible).sum()) >= 30   # Gaussians behind the camera, in both workgroups
        assert (~fr.visible)[:256].any() and (~fr.visible)[256:].any()
    if name == "clamped":
        assert int(clamped.sum()) >= 30 and int((~clamped & fr.visible[:, None]).sum()) >= 30
    if name == "offband":
        assert int(out_x.sum()) >= 20 and int(out_y.sum()) >= 20


@pytest.mark.parametrize("P", [1, 256, 257])
def test_workgroup_edges(P):
    fr = _family_frame("plain", P)
    rec = pg.records("normal", P)
    check(f"plain P={P}", fr, rec, fr.half(rec), pg.T["plain"], 1 if P == 1 else P // 2)


# ---- the variants, on two families with N(0,1) records ----------------------------------------------------------------------------------------
VARIANTS = {   # family() arguments, Frame arguments, half() arguments, vjp arguments
    "M16D3": ({}, {}, {}, {}),
    "M16D1": (dict(M=16, D=1), {}, {}, {}),
    "M9D2": (dict(M=9, D=2), {}, {}, {}),
    "M4D1": (dict(M=4, D=1), {}, {}, {}),
    "M1D0": (dict(M=1, D=0), {}, {}, {}),
    "colours": (dict(precomp=True), {}, {}, {}),
    "split": ({}, dict(layout="split"), {}, {}),
    "misaligned": ({}, dict(layout="misaligned"), {}, {}),
    "split-M4D1": (dict(M=4, D=1), dict(layout="split"), {}, {}),
    "misaligned-M9D2": (dict(M=9, D=2), dict(layout="misaligned"), {}, {}),
    "split-M1D0": (dict(M=1, D=0), dict(layout="split"), {}, {}),
    "legacy": ({}, dict(stash=False), {}, {}),
    "legacy-M9D2": (dict(M=9, D=2), dict(stash=False), {}, {}),
    "legacy-split": ({}, dict(stash=False, layout="split"), {}, {}),
    "legacy-misaligned": ({}, dict(stash=False, layout="misaligned"), {}, {}),
    "compact": ({}, {}, dict(compact=True), {}),
    "compact-legacy": ({}, dict(stash=False), dict(compact=True), {}),
    "cov3D": ({}, dict(cov3D=True), {}, dict(cov3D=True)),
    "ewa": ({}, dict(ewa=True), {}, dict(ewa=True)),
    "ewa-legacy": ({}, dict(ewa=True, stash=False), {}, dict(ewa=True)),
    "camera": ({}, {}, dict(camera=True), dict(camera=True)),
    "camera-legacy-split": ({}, dict(stash=False, layout="split"), dict(camera=True), dict(camera=True)),
    "camera-ewa-compact": ({}, dict(ewa=True), dict(camera=True, compact=True), dict(camera=True, ewa=True)),
    "camera-colours": (dict(precomp=True), {}, dict(camera=True), dict(camera=True)),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["plain", "clamped"])
def test_variants(name, variant):
    fkw, frame_kw, half_kw, ref_kw = VARIANTS[variant]
    sc = pg.family(name, **fkw)
    frame_kw = dict(frame_kw)
    ewa = frame_kw.pop("ewa", False)
    sd = settings_dict(**FULL_STP, ewa=ewa)
    if frame_kw.pop("cov3D", False):   # (a precomputed covariance: the global mode, the sorted modes need scales and rotations)
        sd = settings_dict(0)
        frame_kw["cov3D"] = sc.meta["cov3D_precomp"] = scenes.covariance_from_scale_rotation(sc)
    fr = Frame(sc, sd, **frame_kw)
    rec = pg.records("normal", sc.P)
    got = fr.half(rec, **half_kw)
    if variant == "colours":
        assert "dL_dsh" not in got
    check(f"{name} {variant}", fr, rec, got, pg.T[name + "_ewa" if ewa else name], sc.P // 2, **ref_kw)


@pytest.mark.parametrize("layout", ["cat", "split"])
def test_chunked_half(layout):
    sc = pg.family("plain", P=549)   # three workgroups: chunk 0 of 2 takes the first, chunk 1 the other two
    fr = Frame(sc, FULL, layout=layout)
    rec = pg.records("normal", sc.P)
    check(f"plain chunked {layout}", fr, rec, fr.half(rec, compact=True, chunks=2), pg.T["plain"], sc.P // 2)


# ---- the convention check ---------------------------------------------------------------------------------------------------------------------------
def test_render_half_records_are_the_float64_cotangents():
    """On the pin scene (P=150, 40x36, orbit; low density: the hierarchical mode's order is the exact per-pixel order) the render half's
    records against the cotangents of per_gaussian()'s intermediates under the same loss, the conic-xy slot halved; per slot group,
    relative to the group's largest entry, the suite's 1e-4 for quantities the render half sums with atomics."""
    sc = scenes.make_scene(P=150, W=40, H=36, sigma_min=1.0, sigma_max=8.0, seed=7, camera="orbit")

    def make():
        img, _, details = torch_ref.render_core(sc, "exact")
        p = details["per_gaussian"]
        loss = (img * torch.tensor(sc.dL_dout, dtype=torch.float64)).sum()
        gs = torch.autograd.grad(loss, [p["colour"], p["ndc"], *p["conic"], p["opacity"]])
        rec = torch.cat([gs[0], gs[1], torch.stack(gs[2:6], 1)], 1).numpy()
        rec[:, 6] *= 0.5
        return (rec,)
    want = torch_ref.cached("per_gaussian_cotangents", "pin-exact", make)[0]
    fr = Frame(sc, settings_dict(3))
    got, vis = fr.render_records(), fr.visible
    assert int(vis.sum()) >= 100
    for label, cols in (("colour", slice(0, 3)), ("mean2D", slice(3, 5)), ("conic", slice(5, 8)), ("opacity", slice(8, 9))):
        e = _rel(got[vis][:, cols], want[vis][:, cols])
        print(f"\n[per-gaussian] records vs float64 cotangents, {label}: {e:.2e}")
        assert e < 1e-4, label
