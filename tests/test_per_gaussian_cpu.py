"""CPU tests of the per-Gaussian yardstick (tests/torch_ref_per_gaussian.py), which tests/test_gpu_per_gaussian.py holds the kernel to.

  1. Consistency: fed with the cotangents of per_gaussian()'s intermediates from a whole render_core loss, vjp() with every switch off
     returns torch_ref.loss_and_grads, to 1e-10 of each row's largest entry -- both orders, with SH and with precomputed colours.
  2. The switches: the ewa closed form moves the scale gradients by more than 1e-2 (the figure tests/test_oracle_cpu.py::
     test_oracle_ewa_scaling_gradient_quirk asserts for the oracle), off it is plain autograd to 1e-10; each of the other four moves what
     it says and nothing else.
  3. The tolerance table: measured again here (the module in float32 against itself in float64) and held to T / 4 * 1.25; its
     conditions (floor, cap, rounding), and every family's visibility, band and clamp counts.

Float32 evaluation, worst ratio per family over the four record kinds, measured on the CPU (not numbers of the kernel):

    family       means3D  scales   rotations sh       cov3D    opacity
    plain        1.0e-06  1.2e-06  1.3e-06   3.4e-07  1.0e-06  0
    clamped      1.8e-06  1.0e-06  1.6e-06   3.3e-07  8.2e-07  0
    subpixel     4.4e-06  1.2e-06  1.2e-06   3.9e-07  7.1e-07  0
    huge         2.0e-06  1.3e-06  2.0e-06   3.6e-07  1.2e-06  0
    needles10    4.5e-05  7.6e-05  9.5e-05   3.7e-07  7.6e-05  0
    needles24    2.7e-04  4.4e-04  4.6e-04   3.7e-07  4.4e-04  0
    offband      1.1e-06  1.1e-06  2.4e-06   3.1e-07  1.1e-06  0
    rawquat      1.5e-05  1.0e-05  5.3e-06   3.8e-07  4.4e-06  0
    fxfy         1.2e-06  1.7e-06  4.6e-06   3.1e-07  9.5e-07  0
    near         1.6e-06  1.1e-06  2.2e-06   3.6e-07  9.4e-07  0
    far          1.4e-06  7.9e-07  9.5e-06   4.0e-07  7.9e-07  0
    plain_ewa    1.0e-06  1.0e-06  1.3e-06   3.4e-07  1.1e-06  2.0e-07
    clamped_ewa  1.8e-06  1.0e-06  1.6e-06   3.3e-07  8.2e-07  2.0e-07
    camera       view 3.0e-08  proj 7.1e-08  campos 5.4e-08
"""
import numpy as np
import pytest
import torch

import torch_ref
import torch_ref_per_gaussian as pg
from diff_gaussian_rasterization import scenes

PAIRS = (("dL_dmeans3D", "means3D"), ("dL_dscales", "scales"), ("dL_drotations", "rotations"), ("dL_dopacity", "opacities"),
         ("dL_dmeans2D", "means2D"), ("dL_dsh", "shs"), ("dL_dcolors", "colors_precomp"), ("dL_dcov3D", "cov3D_precomp"),
         ("dL_dview", "viewmatrix"), ("dL_dproj", "projmatrix"), ("dL_dcam", "campos"))


def _pin_scene(use_sh=True):
    return scenes.make_scene(P=150, W=40, H=36, sigma_min=1.0, sigma_max=8.0, seed=7, camera="orbit", use_sh=use_sh)


def _whole_render(sc, order, **kw):
    """(records (P,9): the cotangents of the carved intermediates under the scene's loss, {leaf: gradient})"""
    img, leaves, details = torch_ref.render_core(sc, order, **kw)
    p = details["per_gaussian"]
    loss = (img * torch.tensor(sc.dL_dout, dtype=torch.float64)).sum()
    inter = [p["colour"], p["ndc"], *p["conic"], p["opacity"]]
    names = list(leaves)
    gs = torch.autograd.grad(loss, inter + [leaves[n] for n in names], allow_unused=True)
    rec = torch.cat([gs[0], gs[1], torch.stack(gs[2:6], 1)], 1).numpy()
    return rec, {n: g.numpy() for n, g in zip(names, gs[6:]) if g is not None}


def _rows_rel(got, ref):
    """largest over the rows of max |got - ref| / max |ref| (rows of zeros must be zeros)"""
    got, ref = got.reshape(len(ref), -1), ref.reshape(len(ref), -1)
    err, top = np.abs(got - ref).max(1), np.abs(ref).max(1)
    assert np.all(err[top == 0] == 0)
    return float(np.max(err[top > 0] / top[top > 0]))


@pytest.mark.parametrize("kw", [{}, {"proper_ewa_scaling": True}, {"use_cov3D_precomp": True}, {"camera_leaves": True}],
                         ids=["", "ewa", "cov3D", "camera"])
@pytest.mark.parametrize("use_sh", [True, False], ids=["sh", "colours"])
@pytest.mark.parametrize("order", ["global", "exact"])
def test_vjp_of_the_cotangents_is_the_whole_gradient(order, use_sh, kw):
    sc = _pin_scene(use_sh)
    rec, ref = _whole_render(sc, order, **kw)
    assert np.abs(rec).max(0).min() > 0   # every slot is live
    got = pg.vjp(sc, rec, **kw)
    seen = 0
    for a, b in PAIRS:
        if b in ref:
            if a in pg.CAMERA:
                assert np.max(np.abs(got[a] - ref[b])) <= 1e-10 * np.max(np.abs(ref[b])), a
            else:
                assert _rows_rel(got[a], ref[b]) <= 1e-10, a
            seen += 1
    assert seen == len(ref)


def test_ewa_switch_is_the_quirk_and_nothing_else():
    sc = _pin_scene()
    rec, ref = _whole_render(sc, "global", proper_ewa_scaling=True)
    plain = pg.vjp(sc, rec, proper_ewa_scaling=True)
    quirk = pg.vjp(sc, rec, proper_ewa_scaling=True, ewa_closed_form=True)
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    assert _rows_rel(plain["dL_dscales"], ref["scales"]) <= 1e-10
    assert rel(quirk["dL_dscales"], ref["scales"]) > 1e-2
    for n in ("dL_dopacity", "dL_dsh", "dL_dmeans2D"):   # the factor's value and the other slots are untouched
        assert np.array_equal(quirk[n], plain[n]), n
    # without proper_ewa_scaling the switch has nothing to act on
    a, b = pg.vjp(sc, rec), pg.vjp(sc, rec, ewa_closed_form=True)
    assert all(np.array_equal(a[n], b[n]) for n in a)
    # the restatement against the oracle, which reproduces the reference: with the switch the covariance-path gradients are the oracle's
    # (test_oracle_cpu.py's bound for the oracle against a yardstick, 5e-5 of the largest entry), without it they are not
    from helpers import _rel, settings_dict
    from oracle import oracle as orc
    g = orc.forward_scene(sc, settings_dict(0, ewa=True)).backward(sc.dL_dout)
    rec_k = rec.copy(); rec_k[:, 6] *= 0.5   # (the record's convention: half the cotangent)
    full = pg.vjp(sc, rec_k, proper_ewa_scaling=True, kernel=True)
    for n in ("dL_dscales", "dL_drotations", "dL_dmeans3D"):
        assert _rel(g[n], full[n]) < 5e-5, n
    assert _rel(g["dL_dscales"], plain["dL_dscales"]) > 1e-2


def test_each_convention_switch_moves_what_it_says():
    sc = scenes.vary_inputs(_pin_scene(), scale_modifier=1.7)
    rec = pg.records("normal", sc.P)
    base = pg.vjp(sc, rec)
    # conic_xy_half: the same as doubling the record's xy slot
    rec2 = rec.copy(); rec2[:, 6] *= 2
    a, b = pg.vjp(sc, rec, conic_xy_half=True), pg.vjp(sc, rec2)
    assert all(np.allclose(a[n], b[n], rtol=1e-13, atol=0) for n in a)
    # inv_det_eps: every gradient that passes the conic is scaled by det^2 / (det^2 + 1e-7); with only conic slots live that is all of it
    rc = np.zeros_like(rec); rc[:, 5:8] = rec[:, 5:8]
    a, b = pg.vjp(sc, rc, inv_det_eps=True), pg.vjp(sc, rc)
    _, p = torch_ref.per_gaussian(sc)
    k = (p["det"] ** 2 / (p["det"] ** 2 + 1e-7)).detach().numpy()
    assert k.min() < 1 - 1e-9
    for n in ("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dcov3D"):
        assert np.allclose(a[n], b[n] * k[:, None], rtol=1e-12, atol=0), n
    # scale_modifier_omitted
    a = pg.vjp(sc, rec, scale_modifier_omitted=True)
    assert np.allclose(a["dL_dscales"] * 1.7, base["dL_dscales"], rtol=1e-14, atol=0)
    assert all(np.array_equal(a[n], base[n]) for n in a if n != "dL_dscales")
    # clamp_constant: moves Gaussians outside the 1.3 tan_fov band only
    so = pg.family("offband")
    ro, vis = pg.records("normal", so.P), np.ones(so.P, bool)
    out_x, out_y, _ = pg.conditions(so, vis)
    a, b = pg.vjp(so, ro), pg.vjp(so, ro, clamp_constant=True)
    moved = np.abs(a["dL_dmeans3D"] - b["dL_dmeans3D"]).max(1) > 1e-9 * np.abs(a["dL_dmeans3D"]).max(1)
    assert moved[out_x | out_y].all() and not moved[~(out_x | out_y)].any()
    # kernel=True is all five
    a = pg.vjp(sc, rec, kernel=True)
    b = pg.vjp(sc, rec, conic_xy_half=True, inv_det_eps=True, ewa_closed_form=True, scale_modifier_omitted=True, clamp_constant=True)
    assert all(np.array_equal(a[n], b[n]) for n in a)


def test_scale_is_the_sum_of_the_absolute_slot_terms():
    """S >= |gradient| row maximum (triangle inequality), with equality for one-live-slot records; zero records give zero scale."""
    sc = pg.family("plain")
    vis = pg.yardstick_visible(sc)
    for kind in ("normal", "oneslot"):
        rec = pg.records(kind, sc.P)
        g, S = pg.reference(sc, rec, vis)
        for n in S:
            top = np.abs(g[n]).reshape(sc.P, -1).max(1)
            assert np.all(top <= S[n] * (1 + 1e-12)), n
            if kind == "oneslot":
                assert np.allclose(top, S[n], rtol=1e-12, atol=0), n
            assert np.all(S[n][~vis] == 0)
    _, S = pg.reference(sc, pg.records("zeros", sc.P), vis)
    assert all(np.all(s == 0) for s in S.values())
    assert pg.ratio(np.zeros((sc.P, 3)), np.zeros((sc.P, 3)), S["dL_dmeans3D"]) == 0.0


# ---- the tolerance table ------------------------------------------------------------------------------------------------------------------------
def test_table_conditions():
    assert set(pg.T) == set(pg.FAMILIES) | {"plain_ewa", "clamped_ewa", "camera"}
    for fam, row in pg.T.items():
        assert set(row) == (set(pg.CAMERA) if fam == "camera" else set(pg.MEASURED)), fam
        for n, t in row.items():
            assert pg.FLOOR <= t <= pg.CAP, (fam, n, t)
            assert pg.tolerance(t / 4) == pytest.approx(t, rel=1e-12)   # two significant digits
    assert pg.tolerance(0.0) == 9.6e-7 and pg.tolerance(1.0e-6) == pytest.approx(4.0e-6) and pg.tolerance(1.01e-6) == pytest.approx(4.1e-6)


MIN_VISIBLE = 200   # of 293 (measured: 251 with every seventh hidden, 284 on the narrowed frustum, else 293)


@pytest.mark.parametrize("name", pg.FAMILIES)
def test_float32_evaluation_stays_within_the_table(name):
    worst, n_vis, (out_x, out_y, clamped) = pg.measure_float32(name)
    print(f"\n{name}: {n_vis} visible, float32 worst ratio " + " ".join(f"{n[4:]} {v:.1e}" for n, v in worst.items()))
    assert n_vis >= MIN_VISIBLE
    if name == "offband":
        assert int(out_x.sum()) >= 20 and int(out_y.sum()) >= 20
    if name == "clamped":
        sc = pg.family(name)
        vis = pg.yardstick_visible(sc)
        assert int(clamped.sum()) >= 30 and int((~clamped & vis[:, None]).sum()) >= 30
    for n, v in worst.items():
        assert v <= pg.T[name][n] / 4 * 1.25, (n, v)


@pytest.mark.parametrize("name", ["plain", "clamped"])
def test_float32_evaluation_of_the_variants_stays_within_the_table(name):
    for fkw, kw in pg.VARIANT_MEASUREMENTS:
        kinds = pg.KINDS if kw == dict(proper_ewa_scaling=True) else ("normal",)
        worst, n_vis, _ = pg.measure_float32(name, kinds=kinds, family_kw=fkw, **kw)
        assert n_vis >= MIN_VISIBLE
        row = pg.T[name + "_ewa" if kw.get("proper_ewa_scaling") else name]
        for n, v in worst.items():
            t = pg.T["camera"][n] if n in pg.CAMERA else row[n]
            assert v <= t / 4 * 1.25, (fkw, kw, n, v)
