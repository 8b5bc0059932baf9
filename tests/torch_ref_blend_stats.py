"""Float64 yardstick of the blend statistics, from the N x P matrix of blend weights that torch_ref's renderer returns in its details.

The blend weight of a (pixel, Gaussian) pair is w = alpha * T, T the pixel's transmittance in front of the blend (include/stp_raster.h:
stp_set_backward_blend_stats).  blend_stats[i] = (sum_p w[p, i], max_p w[p, i], #{p : pair (p, i) blended}) over the pairs the
rasterizer blends: alpha >= 1/255, in front of the entry whose blend would take the pixel's transmittance below 1e-4.

Shares no code with the kernels or the oracle.  No autograd: the statistics do not depend on the loss.  Scales and rotations only (no
precomputed covariance, no proper_ewa_scaling).
"""
from __future__ import annotations

import torch

import torch_ref

ALPHA_MIN, T_MIN = 1.0 / 255.0, 1e-4
YARD_SEED = 9   # seed of the P = 150, 40 x 36 scene the kernels are compared on: at most 1 % of its Gaussians are marked `near` (see weights())


def weights(scene, order="global", depth_key="z"):
    """Returns a dict of float64 / bool tensors:
    w (N, P): the blend weight of every pair, 0 where the pair is not blended;  blended (N, P): the pairs;  T_final (N,);
    near (N, P): pairs whose membership hangs on a rounding -- a candidate whose alpha lies within 1e-6 of 1/255, or an entry reached
    by its pixel whose T * (1 - alpha) lies within 1e-6 (relative) of 1e-4."""
    with torch.no_grad():
        d = torch_ref.render_core(scene, order=order, depth_key=depth_key)[2]
    near_T_s = d["reached"] & ((d["test_T"] - T_MIN).abs() <= 1e-6 * T_MIN)
    near = (d["cand"] & ((d["alpha"] - ALPHA_MIN).abs() <= 1e-6)) | torch.zeros_like(near_T_s).scatter(1, d["idx"], near_T_s)
    return {"w": d["w"], "blended": d["blended"], "T_final": d["T_final"], "near": near}


def blend_stats(scene, order="global", depth_key="z", key=None):
    """(stats (P, 3), explained (P,) bool, T_final (N,)) as numpy arrays (float64 / bool): per Gaussian the sum, the maximum and the count
    of its blend weights, and whether a pair of its hangs on a rounding (see weights()).  key: a hashable name under which the (read-only)
    result is kept for the other tests of the session that need the same scene and order."""
    def make():
        r = weights(scene, order=order, depth_key=depth_key)
        w = r["w"]
        stats = torch.stack([w.sum(0), w.max(0).values, r["blended"].sum(0).to(torch.float64)], 1)
        return (stats.numpy(), r["near"].any(0).numpy(), r["T_final"].numpy())
    return torch_ref.cached("blend_stats", key, make)
