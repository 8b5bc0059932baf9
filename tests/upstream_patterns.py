"""Structured upstream gradients dL/dpixel for the tests of the render backwards (test_upstream_grad_cpu.py, test_gpu_upstream_grad.py).

Every other gradient test feeds scene.dL_dout, a dense N(0,1) image: every tile's largest |dL/dpixel| is 3 .. 4, so the per-tile scale of
the kernels' on-chip fixed point (stp_render_hier.inc: "on-chip gradient window") always has the exponent 2, no tile is all zero, and
no pixel differs from its tile's largest by more than a few bits.  patterns() varies exactly that, on scenes the suite already trusts.

Deterministic: scenes.normal with a fixed seed, no numpy.random.  Also the cases of the float64 yardstick that both test files share:
the scene (yard_scene), the three settings (MODES) and the CPU oracle's constant against the yardstick (oracle_constants).
"""
from __future__ import annotations

import numpy as np

from helpers import _precomp, oracle_run
from diff_gaussian_rasterization import scenes
from test_gpu_absgrad import YARD
import torch_ref_colour_bound as cb

TILE = 16
HOT = 2.0 ** 20
N2_SEED, N2_STREAM = 1234, 301   # the second normal image of `trainer`


def patterns(scene):
    """{name: (3, H, W) float32}.  base = scene.dL_dout:
      n01        base: what every other test feeds;
      hot_tile   tile (0, 0) -- the first 16 x 16 pixels -- times 2^20: a per-tile scale, cold tiles beside a hot one;
      hot_pixel  pixel (8, 8) times 2^20 in all channels: dynamic range inside a tile;
      trainer    base * exp(2 n2) / (3 H W), n2 a second normal image: small, heavy-tailed magnitudes (on the 40 x 36 scene the tiles' scales
                 have exponents -2 .. -5, the typical pixel lies at 2^-13);
      one_tile   base inside tile (0, 0), zero elsewhere: tiles whose largest |dL/dpixel| is 0, Gaussians that must get exact zeros;
      pow-60, pow+60   base * 2^-60, base * 2^60: the exponent arithmetic far from 2 (a power of two is exact: every bound scales with it)."""
    base = np.asarray(scene.dL_dout, np.float32)
    H, W = scene.H, scene.W
    assert base.shape == (3, H, W)
    out = {"n01": base.copy()}
    hot_tile = base.copy()
    hot_tile[:, :TILE, :TILE] *= np.float32(HOT)
    out["hot_tile"] = hot_tile
    hot_pixel = base.copy()
    hot_pixel[:, 8, 8] *= np.float32(HOT)
    out["hot_pixel"] = hot_pixel
    n2 = scenes.normal(N2_SEED, N2_STREAM, 3 * H * W).reshape(3, H, W)
    out["trainer"] = (base.astype(np.float64) * np.exp(2.0 * n2) / (3.0 * H * W)).astype(np.float32)
    one_tile = np.zeros_like(base)
    one_tile[:, :TILE, :TILE] = base[:, :TILE, :TILE]
    out["one_tile"] = one_tile
    out["pow-60"] = base * np.float32(2.0 ** -60)
    out["pow+60"] = base * np.float32(2.0 ** 60)
    for a in out.values():
        a.setflags(write=False)
    return out


PATTERNS = ("n01", "hot_tile", "hot_pixel", "trainer", "one_tile", "pow-60", "pow+60")
HOT_PATTERNS = ("hot_tile", "hot_pixel")

# the yardstick's cases: test_gpu_absgrad.YARD's settings and orders; per backward mode, does the kernel keep its sums in the fixed point
FIXED_POINT = {"global": {None: False}, "kbuffer16": {"replay": True, "resort": False}, "hier": {"replay": True, "resort": True}}
MODES = {m: (sd, order, FIXED_POINT[m]) for m, (sd, order, _) in YARD.items()}
CAMERAS = ("origin", "orbit")


def yard_scene(camera):
    """The P = 150, 40 x 36 scene of the float64 comparisons, its colours given directly."""
    return _precomp(scenes.make_scene(P=150, W=40, H=36, sigma_min=1.0, sigma_max=8.0, seed=7, camera=camera))


def with_upstream(scene, dL):
    scene.dL_dout = np.ascontiguousarray(dL, np.float32)
    return scene


def hot_tile_mask(scene):
    """(N,) bool: the pixels of tile (0, 0)."""
    m = np.zeros((scene.H, scene.W), bool)
    m[:TILE, :TILE] = True
    return m.reshape(-1)


_consts = {}


def oracle_constants(mode):
    """{(camera, pattern): K_orc} of settings `mode`: the CPU oracle's own constant against the yardstick,
    K_orc = max over (Gaussian, channel) with A > 0 of |oracle - grad| / (u A).  Also asserts that the oracle returns exact zeros wherever
    A = 0.  Computed once per session."""
    if mode not in _consts:
        sd, order, _ = MODES[mode]
        out = {}
        for camera in CAMERAS:
            sc = yard_scene(camera)
            _, w = cb.weights(sc, order=order, key=(camera, order))
            for name, dL in patterns(sc).items():
                t = cb.bound_terms(w, dL, sc.W, sc.H)
                f, g = oracle_run(with_upstream(yard_scene(camera), dL), sd)
                err = np.abs(g["dL_dcolors"].astype(np.float64) - t["grad"])
                pos = t["A"] > 0
                assert not err[~pos].any(), (mode, camera, name, "the oracle is not exactly zero where A = 0")
                out[camera, name] = float(np.max(err[pos] / (cb.U * t["A"][pos])))
                f.free()
        _consts[mode] = out
    return _consts[mode]


def K_of(mode):
    """The constant of the bound for settings `mode`: four times the oracle's own, over all patterns and both cameras."""
    return cb.MARGIN * max(oracle_constants(mode).values())
