"""Float64 yardstick of the alpha output, the per-pixel background and the background gradients, from torch_ref.render_core as it is.

render_core's image is C + T * bg with one bg for the frame, and linear in it: two renders of a scene, with bg = 0 and with bg = e0 =
(1, 0, 0), give everything a per-pixel background B (3, H, W) and an alpha output need:

    T     = img(bg = e0)[0] - img(bg = 0)[0]          the transmittance behind the last blend
    alpha = 1 - T
    image = img(bg = 0) + T * B

and, for the loss  sum(w * image) + sum(wA * alpha)  =  sum(w * img(0)) + sum(s * T) + const  with  s = sum_ch B * w - wA,

    gradients = g(bg = 0, dL = w) + g(bg = e0, dL = (s, 0, 0)) - g(bg = 0, dL = (s, 0, 0))
    dL/dB     = T * w            (uniform background: its sum over the pixels, per channel)

The same decomposition runs on any renderer that takes a uniform background and a dL_dout: decompose() is handed the two images and a
gradient function, which is how test_background_cpu.py holds the CPU oracle against this yardstick.
"""
from __future__ import annotations

import copy

import numpy as np
import torch

import torch_ref

E0 = np.array([1.0, 0.0, 0.0], np.float32)


def with_bg(scene, bg):
    sc = copy.copy(scene)
    sc.bg = np.asarray(bg, np.float32)
    return sc


def weights(scene, seed=5):
    """The random inputs of a case: B in [0, 1] (3, H, W), the image weights w (the scene's own dL_dout) and alpha weights wA (H, W)."""
    rng = np.random.default_rng(seed)
    B = rng.uniform(0.0, 1.0, (3, scene.H, scene.W)).astype(np.float32)
    wA = rng.standard_normal((scene.H, scene.W)).astype(np.float32)
    return B, np.asarray(scene.dL_dout, np.float32), wA


def decompose(img0, img_e, grads, B, w, wA, dtype=np.float64):
    """img0, img_e: the images with bg = 0 and bg = e0; grads(bg, dL) -> {name: gradient of sum(dL * image)} of the render with that
    background (bg: 0 or 1 for e0).  B: (3, H, W) or a uniform (3,) colour.  Returns image, alpha, T, the summed gradients, dL/dB per
    pixel and its sum per channel."""
    img0, img_e = np.asarray(img0, dtype), np.asarray(img_e, dtype)
    B = np.asarray(B, dtype)
    Bp = B if B.ndim == 3 else np.broadcast_to(B[:, None, None], img0.shape)
    w, wA = np.asarray(w, dtype), np.asarray(wA, dtype)
    T = img_e[0] - img0[0]
    s = np.zeros_like(img0)
    s[0] = (Bp * w).sum(0) - wA
    g0, ge = grads(0, (w - s).astype(dtype)), grads(1, s)
    out = {n: (None if g0[n] is None else np.asarray(g0[n], dtype) + np.asarray(ge[n], dtype)) for n in g0}
    dB = T[None] * w
    return dict(image=img0 + T[None] * Bp, alpha=1.0 - T, T=T, grads=out, dB=dB, dbg=dB.reshape(3, -1).sum(1))


def reference(scene, B, w, wA, **kw):
    """The yardstick in float64; kw: render_core's (order, depth_key, proper_ewa_scaling, ...)."""
    renders = [torch_ref.render_core(with_bg(scene, bg), **kw)[:2] for bg in (np.zeros(3, np.float32), E0)]

    def grads(which, dL):
        img, leaves = renders[which]
        names = list(leaves)
        g = torch.autograd.grad((img * torch.tensor(dL, dtype=torch.float64)).sum(), [leaves[n] for n in names], allow_unused=True, retain_graph=True)
        return {n: (None if x is None else x.detach().numpy()) for n, x in zip(names, g)}

    return decompose(renders[0][0].detach().numpy(), renders[1][0].detach().numpy(), grads, B, w, wA)
