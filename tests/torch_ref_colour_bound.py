"""Float64 yardstick of dL/dcolors_precomp Gaussian by Gaussian, with a bound per entry: a further hook on torch_ref.render_core.

Of the nine gradient sums, the colour gradient is the one whose terms do not cancel inside a pixel:

    grad[i, ch] = sum_p w[p, i] dL[ch, p]          w = alpha T, the pair's blend weight (render_core's details["w"])

so the sum of the terms' magnitudes, A[i, ch] = sum_p w[p, i] |dL[ch, p]|, is what float32 rounding of the terms and of their sum is
relative to, and a bound per (Gaussian, channel) can be stated:

    |kernel - grad| <= B = K u A + Q        u = 2^-24

K is the CPU oracle's own constant against this yardstick times MARGIN (tests/upstream_patterns.py: oracle_constants), never the
kernels'.  Q is the quantum of the kernels' on-chip fixed point (stp_render_hier.inc: "on-chip gradient window"): a workgroup stores a
term as round(t 2^31 / 2^e), 2^e >= M = the tile's largest |dL/dpixel| over the three channels, e from frexp; each add is off by at most
half a unit, 2^(e - 32):

    Q[i, ch] = sum over tiles of  n(tile, i, ch) 2^(e(tile) - 32),    n = #{p in tile: w[p, i] > 0 and dL[ch, p] != 0}

(an upper bound: lanes merged in registers add once).  A tile with M = 0 adds nothing.  A = 0 gives B = 0: a Gaussian that blends only
where the upstream gradient is zero must come out as exact zeros.

Q describes finite upstream gradients only.  The kernels take M with fmaxf, which drops a NaN: a NaN pixel leaves M the largest of
the tile's other pixels and the fixed point in use, and it is the range check in front of each add that sends a non-finite term to
memory.  With M = inf the replay keeps nothing on the chip (its cap is 0), the re-sorting hierarchical backward keeps e = 0 and a cap of
2^20.  tile_exponents() leaves a NaN out as the kernels do; a tile with M = inf gets e = 0 and no Q.  The non-finite test of
test_gpu_upstream_grad.py takes its bound from the run without the poison.

Shares no code with the kernels or the oracle.  Colours given directly (helpers._precomp), scales and rotations only.
"""
from __future__ import annotations

import numpy as np
import torch

import torch_ref

U = 2.0 ** -24
MARGIN = 4.0
TILE = 16
FX_BITS = 31


def weights(scene, order="global", key=None):
    """(image (3, H, W), w (N, P)) float64, read-only: the yardstick's image and blend weights.  Neither depends on the upstream gradient.
    key: see torch_ref.cached."""
    def make():
        with torch.no_grad():
            img, _, d = torch_ref.render_core(scene, order=order)
        return (img.numpy(), d["w"].numpy())
    return torch_ref.cached("colour_bound", key, make)


def tile_index(W, H):
    """(N,) index of every pixel's 16 x 16 tile, row-major."""
    ys, xs = np.divmod(np.arange(W * H), W)
    return (ys // TILE) * ((W + TILE - 1) // TILE) + xs // TILE


def tile_exponents(dL, W, H):
    """(M (tiles,) float32, e (tiles,) int): the largest |dL| of every tile over the three channels, a NaN left out as fmaxf leaves it
    out, and its frexp exponent (M <= 2^e); e is 0 where M is zero or infinite (see the module's text)."""
    mag = np.nan_to_num(np.abs(np.asarray(dL, np.float32).reshape(3, -1)), nan=0.0, posinf=np.inf).max(axis=0)
    tid = tile_index(W, H)
    M = np.array([np.max(mag[tid == t]) for t in range(int(tid.max()) + 1)], np.float32)
    ok = np.isfinite(M) & (M > 0) & (M < np.float32(3.0e38))
    e = np.where(ok, np.frexp(np.where(ok, M, np.float32(1.0)))[1], 0).astype(np.int64)
    return M, e


def bound_terms(w, dL, W, H):
    """{"grad", "A", "Q"}: (P, 3) float64 each, for the blend weights w (N, P) and the upstream gradient dL (3, H, W)."""
    dl = np.asarray(dL, np.float32).astype(np.float64).reshape(3, -1)
    grad = w.T @ dl.T
    A = w.T @ np.abs(dl).T
    M, e = tile_exponents(dL, W, H)
    tid = tile_index(W, H)
    Q = np.zeros_like(A)
    for t in range(len(M)):
        if not (np.isfinite(M[t]) and M[t] > 0):
            continue
        pix = tid == t
        n = (w[pix] > 0).astype(np.float64).T @ (dl[:, pix] != 0).astype(np.float64).T
        Q += n * 2.0 ** float(e[t] - FX_BITS - 1)
    return {"grad": grad, "A": A, "Q": Q}


def bound(terms, K, fixed_point):
    """B = K u A + Q (Q only for a kernel that keeps its sums in the fixed point)."""
    return K * U * terms["A"] + (terms["Q"] if fixed_point else 0.0)


def use_of_bound(got, terms, B):
    """The largest |got - grad| / B over the entries with B > 0; inf if an entry with B = 0 is not exactly zero."""
    err = np.abs(np.asarray(got, np.float64) - terms["grad"])
    zero = B == 0
    if np.any(err[zero] != 0):
        return float("inf")
    return float(np.max(err[~zero] / B[~zero])) if (~zero).any() else 0.0
