"""Float64 autograd yardstick of absgrad: torch_ref's renderer with the per-pixel screen offsets as a leaf.

absgrad[i] = (sum_p |g_x,p(i)|, sum_p |g_y,p(i)|, 0), where g_p(i) is what pixel p adds to dL/dmeans2D[i] (include/stp_raster.h:
stp_set_backward_absgrad).  A Gaussian's 2D mean reaches pixel p only through the offsets dx[p, i] = mx[i] - px, dy[p, i] = my[i] - py,
so with an N x P leaf added to each offset matrix, dL/d(dx[p, i]) IS pixel p's contribution in pixel units, and the NDC shift that
means2D stands for (torch_ref.render: mx = ((ndc + 1) W - 1) / 2) scales it by W / 2 (H / 2 for y):

    absgrad_x[i] = 0.5 W sum_p |dL/d(dx[p, i])|        means2D.grad_x[i] = 0.5 W sum_p dL/d(dx[p, i])

The offsets are torch_ref.render_core's offset leaves; this module is the reduction.  Shares no code with the kernels or the oracle.
Scales and rotations only (no precomputed covariance, no proper_ewa_scaling): the offsets' path does not depend on either.
"""
from __future__ import annotations

import torch

import torch_ref


def absgrad(scene, order="global", depth_key="z", key=None):
    """(image, absgrad (P, 2), signed (P, 2)) as float64 numpy arrays for the loss sum(scene.dL_dout * image): the sums over pixels of
    the absolute and of the signed per-pixel contributions, both in means2D's units.  key: a hashable name under which the (read-only)
    result is kept for the other tests of the session that need the same scene and order."""
    def make():
        img, leaves, _ = torch_ref.render_core(scene, order=order, depth_key=depth_key, offset_leaves=True)
        loss = (img * torch.tensor(scene.dL_dout, dtype=torch.float64)).sum()
        gx, gy = torch.autograd.grad(loss, [leaves["offsets_x"], leaves["offsets_y"]])
        sx, sy = 0.5 * scene.W, 0.5 * scene.H
        return (img.detach().numpy(),
                torch.stack([sx * gx.abs().sum(0), sy * gy.abs().sum(0)], 1).numpy(),
                torch.stack([sx * gx.sum(0), sy * gy.sum(0)], 1).numpy())
    return torch_ref.cached("absgrad", key, make)
