"""Float64 yardstick of the inverse-depth output (settings._invdepth; include/stp_raster.h: stp_set_forward_invdepth,
stp_set_backward_invdepth), from torch_ref.render_core as it is.

The output is  invdepth[p] = sum_i w_i(p) / z_i  over the pairs the colour blends, w_i = alpha_i T_i, z_i the view-space z of Gaussian i's
centre: a fourth colour channel with a zero background.  So, with c_i = 1 / z_i, the CHANNEL RUN of a scene -- the same geometry with
shs = None, colors_precomp = (c, 0, 0), bg = 0 -- has

    invdepth = color[0] of the channel run

and for the loss  sum(w * color) + sum(wD * invdepth)

    gradients = g_plain(dL = w) + g_channel(dL = (wD, 0, 0))                 (shs: the plain run's alone)
    means3D, viewmatrix += the channel run's colors_precomp.grad[:, 0] chained through  c = 1 / (means3D @ V[:3, 2] + V[3, 2])

The same decomposition runs on any renderer that takes colors_precomp and a dL_dout: decompose() is handed the two images and two
gradient functions, which is how test_invdepth_cpu.py holds the CPU oracle, and test_gpu_invdepth.py the product's own channel run,
against it.  The chain through c is taken by autograd in float64 in every case.
"""
from __future__ import annotations

import copy

import numpy as np
import torch

import torch_ref


def inv_z(scene, dtype=np.float64):
    """c_i = 1 / z_i, z_i = (means3D @ viewmatrix)[2] in the row-vector layout, in `dtype` arithmetic on the scene's float32 values"""
    m, V = np.asarray(scene.means3D, dtype), np.asarray(scene.viewmatrix, dtype).reshape(4, 4)
    z = m[:, 0] * V[0, 2] + m[:, 1] * V[1, 2] + m[:, 2] * V[2, 2] + V[3, 2]
    return (dtype(1.0) / z).astype(dtype)


def channel_scene(scene, dtype=np.float64):
    """The channel run's scene: colours (c, 0, 0) given directly, no SH, a zero background."""
    sc = copy.copy(scene)
    c = inv_z(scene, dtype)
    sc.colors_precomp = np.stack([c, np.zeros_like(c), np.zeros_like(c)], 1)
    sc.shs = None
    sc.bg = np.zeros(3, np.float32)
    return sc


def weights(scene, seed=9):
    """The random inputs of a case: the image weights w (the scene's own dL_dout) and the inverse-depth weights wD (H, W)."""
    rng = np.random.default_rng(seed)
    return np.asarray(scene.dL_dout, np.float32), rng.standard_normal((scene.H, scene.W)).astype(np.float32)


def chain_through_c(scene, dL_dc):
    """(dL/dmeans3D (P, 3), dL/dviewmatrix (4, 4)) of  sum(dL_dc * c),  c = 1 / (means3D @ V[:3, 2] + V[3, 2]),  by autograd in float64"""
    m = torch.tensor(np.asarray(scene.means3D, np.float64), requires_grad=True)
    V = torch.tensor(np.asarray(scene.viewmatrix, np.float64).reshape(4, 4), requires_grad=True)
    c = 1.0 / (m @ V[:3, 2] + V[3, 2])
    gm, gV = torch.autograd.grad((c * torch.tensor(np.asarray(dL_dc, np.float64))).sum(), [m, V])
    return gm.numpy(), gV.numpy()


def decompose(scene, img_plain, img_chan, grads_plain, grads_chan, w, wD, dtype=np.float64):
    """img_plain, img_chan: the images of the scene and of its channel run; grads_plain(dL) / grads_chan(dL) -> {name: gradient of
    sum(dL * image)} of the two runs (None where a run has no such input; the channel run's must hold "colors_precomp").  w: (3, H, W) or
    None (no colour term).  Returns image, invdepth and the summed gradients; "shs" is the plain run's, "colors_precomp" -- the plain
    run's where it has one -- gets nothing from the channel."""
    wD = np.asarray(wD, dtype)
    dL_c = np.zeros((3,) + wD.shape, dtype)
    dL_c[0] = wD
    gc = grads_chan(dL_c)
    gp = grads_plain(np.asarray(w, dtype)) if w is not None else {}
    out = {}
    for n in set(gc) | set(gp):
        a, b = gp.get(n), (None if n in ("shs", "colors_precomp") else gc.get(n))
        parts = [np.asarray(x, np.float64) for x in (a, b) if x is not None]
        out[n] = sum(parts[1:], parts[0]) if parts else None
    gm, gV = chain_through_c(scene, np.asarray(gc["colors_precomp"], np.float64)[:, 0])
    out["means3D"] = out["means3D"] + gm
    if out.get("viewmatrix") is not None:
        out["viewmatrix"] = out["viewmatrix"] + gV.reshape(np.shape(out["viewmatrix"]))
    return dict(image=np.asarray(img_plain, dtype), invdepth=np.asarray(img_chan, dtype)[0], grads=out, chain=(gm, gV))


def reference(scene, w, wD, **kw):
    """The yardstick in float64; kw: render_core's (order, depth_key, camera_leaves, ...)."""
    runs = [torch_ref.render_core(sc, **kw)[:2] for sc in (scene, channel_scene(scene))]

    def grads_of(k):
        def grads(dL):
            img, leaves = runs[k]
            names = list(leaves)
            g = torch.autograd.grad((img * torch.tensor(np.asarray(dL), dtype=torch.float64)).sum(), [leaves[n] for n in names],
                                    allow_unused=True, retain_graph=True)
            return {n: (None if x is None else x.detach().numpy()) for n, x in zip(names, g)}
        return grads

    return decompose(scene, runs[0][0].detach().numpy(), runs[1][0].detach().numpy(), grads_of(0), grads_of(1), w, wD)
