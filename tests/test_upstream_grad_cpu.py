"""CPU tests of the per-Gaussian bound on dL/dcolors_precomp under structured upstream gradients (torch_ref_colour_bound.py,
upstream_patterns.py): the hook is autograd's gradient, the CPU oracle's constant against it is small and the same whatever the pattern,
and the bound B = K u A + Q tells a right kernel from four modelled faults, two of which the suite's whole-tensor measure lets pass as soon
as one tile's upstream gradient is large."""
import os

import numpy as np
import pytest

from helpers import _rel
import torch_ref
import torch_ref_colour_bound as cb
import upstream_patterns as up

PIN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colour_bound_pin.npz"))
ORDERS = ("global", "exact")
PIN_PATTERNS = ("hot_pixel", "trainer", "one_tile")


def _terms(camera, order, name):
    sc = up.yard_scene(camera)
    _, w = cb.weights(sc, order=order, key=(camera, order))
    dL = up.patterns(sc)[name]
    return sc, w, dL, cb.bound_terms(w, dL, sc.W, sc.H)


def test_patterns_are_what_they_say():
    sc = up.yard_scene("orbit")
    p, base = up.patterns(sc), sc.dL_dout
    assert tuple(p) == up.PATTERNS and all(a.shape == base.shape and a.dtype == np.float32 for a in p.values())
    assert np.array_equal(p["n01"], base)
    M = {n: cb.tile_exponents(a, sc.W, sc.H) for n, a in p.items()}
    assert len(M["n01"][0]) == 9 and set(M["n01"][1]) <= {2, 3}
    assert np.array_equal(M["hot_tile"][1], M["n01"][1] + 20 * (np.arange(9) == 0))
    assert M["hot_pixel"][1][0] >= 18 and np.array_equal(M["hot_pixel"][1][1:], M["n01"][1][1:])
    # (small and heavy-tailed: every tile's scale is below 1, the tiles differ, and the typical pixel lies a hundred times below its tile's)
    assert M["trainer"][1].max() <= -1 and len(set(M["trainer"][1])) >= 3, M["trainer"][1]
    assert np.median(np.abs(p["trainer"])) < 2.0 ** -7 * M["trainer"][0].min()
    assert M["one_tile"][0][0] > 0 and not M["one_tile"][0][1:].any() and not M["one_tile"][1][1:].any()
    assert np.array_equal(M["pow-60"][1], M["n01"][1] - 60) and np.array_equal(M["pow+60"][1], M["n01"][1] + 60)
    for n, s in (("pow-60", 2.0 ** 60), ("pow+60", 2.0 ** -60)):   # exact in float32
        assert np.array_equal(p[n].astype(np.float64) * s, base.astype(np.float64))
    p2 = up.patterns(up.yard_scene("orbit"))
    assert all(np.array_equal(p[n], p2[n]) for n in p)


@pytest.mark.parametrize("camera", up.CAMERAS)
@pytest.mark.parametrize("order", ORDERS)
def test_hook_is_autograds_colour_gradient(camera, order):
    """grad = w^T dL equals autograd's colors_precomp gradient to 1e-12 of the largest entry, under a pattern with structure; |grad| <= A."""
    for name in ("hot_pixel", "trainer"):
        sc, w, dL, t = _terms(camera, order, name)
        img, g = torch_ref.loss_and_grads(up.with_upstream(up.yard_scene(camera), dL), order=order)
        assert np.max(np.abs(img - cb.weights(sc, order=order, key=(camera, order))[0])) < 1e-12
        assert t["grad"].shape == g["colors_precomp"].shape == (sc.P, 3)
        assert _rel(t["grad"], g["colors_precomp"]) <= 1e-12, name
        assert np.all(np.abs(t["grad"]) <= t["A"] * (1 + 1e-12))


@pytest.mark.parametrize("mode", list(up.MODES))
def test_oracle_constant_is_small_under_every_pattern(mode):
    """K_orc is finite and below 200 on every case, and the oracle returns exact zeros wherever A = 0 (asserted in oracle_constants)."""
    k = up.oracle_constants(mode)
    assert set(k) == {(c, n) for c in up.CAMERAS for n in up.PATTERNS}
    for camera in up.CAMERAS:
        print(f"\nK_orc {mode} {camera}: " + ", ".join(f"{n} {k[camera, n]:.1f}" for n in up.PATTERNS))
    assert all(np.isfinite(v) and v < 200 for v in k.values()), k
    for camera in up.CAMERAS:   # a power of two is exact in both precisions
        assert k[camera, "pow-60"] == k[camera, "n01"] == k[camera, "pow+60"]
    print(f"K of the bound, {mode}: {up.K_of(mode):.0f}")


def _fixed_point(terms, e_of_pixel):
    """The float64 terms (N, P, 3) rounded to whole units of 2^(e - 31), e per pixel, and summed."""
    q = np.exp2(e_of_pixel.astype(np.float64) - cb.FX_BITS)[:, None, None]
    return (np.rint(terms / q) * q).sum(0)


@pytest.mark.parametrize("camera", up.CAMERAS)
@pytest.mark.parametrize("mode", ["kbuffer16", "hier"])
def test_bound_discriminates(mode, camera):
    """Four numpy models of a kernel, applied to the yardstick's float64 terms, against B with K = 4 K_orc:
    (a) the fixed point with the tile's own scale stays inside B under every pattern;
    (b) the same with the FRAME's scale exceeds B under hot_tile and hot_pixel;
    (c) every entry off by the suite's present 1e-4, relative to itself, exceeds B;
    (d) one lost add exceeds B, for EVERY Gaussian that does not blend in the hot tile and every channel: the smallest ratio of such a
        Gaussian's largest term to its B is what is asserted.
    "Exceeds": by 2 x at least.  Under the hot patterns (b), and (d) with every such Gaussian losing its add at once, pass the whole-tensor
    measure _rel < 1e-4, which is the point; under the other patterns that measure does see (d) (0.14 under n01, 0.98 under trainer), and (c) is its own bound."""
    order = up.MODES[mode][1]
    K = up.K_of(mode)
    hot = up.hot_tile_mask(up.yard_scene(camera))
    for name in up.PATTERNS:
        sc, w, dL, t = _terms(camera, order, name)
        B = cb.bound(t, K, True)
        assert np.array_equal(B == 0, t["A"] == 0)
        dl = np.asarray(dL, np.float64).reshape(3, -1)
        terms = w[:, :, None] * dl.T[:, None, :]                      # (N, P, 3)
        M, e = cb.tile_exponents(dL, sc.W, sc.H)
        live = (M > 0)[cb.tile_index(sc.W, sc.H)]
        assert not terms[~live].any()
        # (a)
        a = cb.use_of_bound(_fixed_point(terms, e[cb.tile_index(sc.W, sc.H)]), t, B)
        # (b)
        e_frame = np.frexp(np.float32(np.max(np.abs(dL))))[1]
        got_b = _fixed_point(terms, np.full(sc.W * sc.H, e_frame))
        b = cb.use_of_bound(got_b, t, B)
        # (c)
        got_c = t["grad"] * (1.0 + 1e-4)
        c = cb.use_of_bound(got_c, t, B)
        # (d)
        cold = (t["A"] > 0).any(1) & ~(w[hot] > 0).any(0)
        idx = np.flatnonzero(cold)
        mine = terms[:, idx, :]
        lost = np.take_along_axis(mine, np.abs(mine).argmax(0)[None], 0)[0]   # (cold Gaussians, 3): each one's largest term per channel
        ratio = (np.abs(lost) / np.where(lost != 0, B[idx], 1.0))[lost != 0]
        d = float(ratio.min()) if ratio.size else 0.0
        got_d = t["grad"].copy()
        got_d[idx] -= lost                                                    # (every cold Gaussian loses its add at once)
        print(f"\n{mode} {camera} {name}: K {K:.0f}; share of B: (a) tile scale {a:.3g}, (b) frame scale {b:.3g}, (c) 1e-4 off {c:.3g}, "
              f"(d) lost add {d:.3g} at least ({int(cold.sum())} cold); whole-tensor _rel of (b) {_rel(got_b, t['grad']):.1e}, "
              f"(d) {_rel(got_d, t['grad']):.1e}")
        assert a <= 1.0, (name, a)
        if name in up.HOT_PATTERNS:
            assert b >= 2.0, (name, b)
            assert _rel(got_b, t["grad"]) < 1e-4 and int(cold.sum()) >= 50
        assert c >= 2.0, (name, c)
        if name != "one_tile":   # (there a Gaussian outside the hot tile has no term at all)
            assert d >= 2.0, (name, d)
            if name in up.HOT_PATTERNS:
                assert _rel(got_d, t["grad"]) < 1e-4
        else:
            assert not cold.any() and int(((t["A"] == 0).all(1) & (w > 0).any(0)).sum()) >= 40


@pytest.mark.parametrize("order", ORDERS)
def test_colour_bound_reproduces_the_pin(order):
    """grad, A and Q of the orbit scene as recorded in tests/golden/colour_bound_pin.npz (written by this module's _write_pin() when
    the hook was added): float arrays to 1e-12 of the largest entry, as test_yardstick_pin_cpu.py asks of the other four hooks; Q, a
    count times a power of two, exactly."""
    for name in PIN_PATTERNS:
        _, _, _, t = _terms("orbit", order, name)
        for k in ("grad", "A", "Q"):
            want = PIN[f"{order}/{name}/{k}"]
            assert t[k].shape == want.shape and want.dtype == np.float64
            if k == "Q":
                assert np.array_equal(t[k], want), (name, k)
            else:
                assert np.max(np.abs(t[k] - want)) <= 1e-12 * np.max(np.abs(want)), (name, k)


def _write_pin(path):
    d = {}
    for order in ORDERS:
        for name in PIN_PATTERNS:
            t = _terms("orbit", order, name)[3]
            d.update({f"{order}/{name}/{k}": t[k] for k in ("grad", "A", "Q")})
    np.savez_compressed(path, **d)
