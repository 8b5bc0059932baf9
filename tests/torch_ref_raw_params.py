"""Float64 yardstick of the raw parameter inputs (GaussianRasterizer(..., raw=); include/stp_raster.h: stp_set_forward_raw_params /
stp_set_backward_raw_params): the three activations, their VJPs, and both composed in front of tests/torch_ref_per_gaussian.py.

    opacity   o = 1 / (1 + exp(-x))                     dL/dx = g o (1 - o)
    scale     s = exp(x)                                dL/dx = g s
    rotation  qh = q / max(|q|, 1e-12)                  dL/dq = (g - qh (qh . g)) / |q|;  g / 1e-12 where |q| < 1e-12 (the clamp was active)

-- torch.sigmoid, torch.exp and torch.nn.functional.normalize with its eps (tests/test_raw_params_cpu.py holds the three VJPs to
torch.autograd on those functions).  g is the gradient of the plain call with respect to the activated value, that call's conventions
included: reference() hands a copy of the scene whose scales / rotations / opacities are the float64 activations of the raw arrays to
pg.vjp(..., kernel=True) and applies the chain rule above in float64.

The raw inputs of a family (raw_inputs) are the inverse activations of pg.family(name)'s own inputs, rounded to float32: log s, logit o, and
q times a per-row factor drawn from [0.5, 3].  Means, SH coefficients and camera are the family's, so its margins (1e-4 from the
1.3 tan_fov band and from the colour clamp) are what they were; measure_float32 asserts them and the visible count, as pg.conditions does.

The measure is pg's: ratio = max over the row |got - float64| / S, with S of pg.scale carried through the activation --
    S_scales max_j s_j        S_opacity o (1 - o)        S_rotations / |q|
(the chain rule of a row scaled entrywise is bounded by the row's largest factor; the projection I - qh qh^T has norm 1).

The bound T[family][tensor] is measured, not chosen, by pg's own rule: 4 x the worst ratio of THIS module evaluated in float32 on the CPU
(the activations, pg.vjp and the chain rule all in float32; never the kernel) over pg's record kinds, rounded up to two digits, floor
16 * 2^-24, cap 2e-3.  tests/test_raw_params_cpu.py re-measures it; tests/test_gpu_raw_params.py holds the kernel to it for the gradient
of every raw input, and to pg.T for every other tensor.
"""
from __future__ import annotations

import copy

import numpy as np
import torch

import torch_ref
import torch_ref_per_gaussian as pg
from diff_gaussian_rasterization import scenes

EPS = 1e-12
BITS = {"opacities": 1, "scales": 2, "rotations": 4}                      # the mask of include/stp_raster.h
TENSOR_BIT = {"dL_dopacity": 1, "dL_dscales": 2, "dL_drotations": 4}     # the gradient a bit redefines
FAMILIES = ("plain", "clamped", "rawquat", "needles10", "plain_ewa")     # "<family>_ewa": under proper_ewa_scaling
MIN_VISIBLE = 200   # of 293, tests/test_per_gaussian_cpu.py


# ---- the activations and their VJPs, in the dtype of their inputs (torch tensors) ---------------------------------------------------------------
def act_opacity(x):
    return 1.0 / (1.0 + torch.exp(-x))


def act_scale(x):
    return torch.exp(x)


def act_rotation(q):
    """(q / max(|q|, eps), |q| before the clamp (P, 1))"""
    n = torch.sqrt((q * q).sum(-1, keepdim=True))
    return q / torch.clamp(n, min=EPS), n


def vjp_opacity(g, x):
    o = act_opacity(x)
    return g * (o * (1.0 - o))


def vjp_scale(g, x):
    return g * act_scale(x)


def vjp_rotation(g, q):
    qh, n = act_rotation(q)
    inside = (g - qh * (qh * g).sum(-1, keepdim=True)) / torch.clamp(n, min=EPS)
    return torch.where(n < EPS, g / EPS, inside)


# ---- the raw inputs of a family ------------------------------------------------------------------------------------------------------------------
def raw_inputs(sc, seed=31):
    """{"scales": log s (P,3), "rotations": q * factor (P,4), "opacities": logit o (P,1)}, float32: the inverse activations of the scene's own
    inputs (rotations: of their direction), rounded once."""
    s, o, q = (np.asarray(a, np.float64) for a in (sc.scales, sc.opacities, sc.rotations))
    factor = 0.5 + 2.5 * scenes.uniform(seed, 600, len(q))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {"scales": f32(np.log(s)), "rotations": f32(q * factor[:, None]), "opacities": f32(np.log(o / (1.0 - o)))}


def _activate_np(name, raw, dtype):
    x = torch.tensor(np.asarray(raw), dtype=dtype)
    y = act_opacity(x) if name == "opacities" else act_scale(x) if name == "scales" else act_rotation(x)[0]
    return y.numpy()


def activated_scene(sc, raw, mask=7, dtype=torch.float64):
    """A copy of the scene whose inputs of `mask` are the activations, evaluated in `dtype`, of the raw arrays; the others stay the scene's own."""
    out = copy.copy(sc)
    for name, bit in BITS.items():
        if mask & bit:
            setattr(out, name, _activate_np(name, raw[name], dtype))
    return out


def split_family(name):
    """"plain_ewa" -> ("plain", True)"""
    return (name[:-4], True) if name.endswith("_ewa") else (name, False)


# ---- the composed map: float64 reference, scale, and the float32 evaluation ----------------------------------------------------------------------
def chain(g, raw, mask, dtype=torch.float64):
    """The gradients g of the plain call on the activated scene (numpy, by output name) carried to the raw inputs of `mask`, in `dtype`."""
    out = dict(g)
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    if mask & 1:
        out["dL_dopacity"] = vjp_opacity(t(g["dL_dopacity"]).reshape(-1, 1), t(raw["opacities"]).reshape(-1, 1)).numpy().reshape(np.shape(g["dL_dopacity"]))
    if (mask & 2) and "dL_dscales" in g:
        out["dL_dscales"] = vjp_scale(t(g["dL_dscales"]), t(raw["scales"])).numpy()
    if (mask & 4) and "dL_drotations" in g:
        out["dL_drotations"] = vjp_rotation(t(g["dL_drotations"]), t(raw["rotations"])).numpy()
    return out


def carry_scale(S, raw, mask):
    """pg.scale's S (P,) per tensor carried through the activations of `mask` (float64)"""
    out = dict(S)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    if mask & 1:
        o = act_opacity(t(raw["opacities"]).reshape(-1)).numpy()
        out["dL_dopacity"] = S["dL_dopacity"] * o * (1.0 - o)
    if (mask & 2) and "dL_dscales" in S:
        out["dL_dscales"] = S["dL_dscales"] * act_scale(t(raw["scales"])).numpy().max(1)
    if (mask & 4) and "dL_drotations" in S:
        n = act_rotation(t(raw["rotations"]))[1].numpy().reshape(-1)
        out["dL_drotations"] = S["dL_drotations"] / np.maximum(n, EPS)
    return out


def reference(sc, raw, mask, rec, visible, key=None, **kw):
    """({name: float64 gradient with respect to the inputs as handed over -- raw where `mask` says so}, {name: S}) of the composed map; the
    plain call's part is pg.reference on the activated scene, kept under `key`."""
    act = activated_scene(sc, raw, mask)
    g, S = pg.reference(act, rec, visible, key=None if key is None else ("raw", mask) + tuple(key), **kw)
    return chain(g, raw, mask), carry_scale(S, raw, mask)


def evaluate_float32(sc, raw, mask, rec, visible, **kw):
    """The composed map with every step in float32 on the CPU: the activations, pg.vjp(kernel=True) and the chain rule."""
    act = activated_scene(sc, raw, mask, dtype=torch.float32)
    g = pg.vjp(act, rec, visible, kernel=True, dtype=torch.float32, **kw)
    return chain(g, raw, mask, dtype=torch.float32)


def visible_and_conditions(sc, raw, ewa):
    """The float64 visibility of the fully activated scene, with pg's assertions on it (band, clamp) and the visible count."""
    act = activated_scene(sc, raw, 7)
    vis = pg.yardstick_visible(act, ewa)
    cond = pg.conditions(act, vis)
    assert int(vis.sum()) >= MIN_VISIBLE, int(vis.sum())
    return vis, cond


def measure_float32(name, mask=7, kinds=pg.KINDS):
    """{tensor of a raw input: worst ratio over `kinds`} of evaluate_float32 against reference on family `name` (FAMILIES)."""
    fam, ewa = split_family(name)
    sc = pg.family(fam)
    raw = raw_inputs(sc)
    vis, _ = visible_and_conditions(sc, raw, ewa)
    kw = dict(proper_ewa_scaling=True) if ewa else {}
    worst = {}
    for kind in kinds:
        rec = pg.records(kind, sc.P)
        ref, S = reference(sc, raw, mask, rec, vis, key=(name, kind), **kw)
        got = evaluate_float32(sc, raw, mask, rec, vis, **kw)
        for n, bit in TENSOR_BIT.items():
            if mask & bit:
                worst[n] = max(worst.get(n, 0.0), pg.ratio(got[n], ref[n], S[n]))
    return worst, int(vis.sum())


# T[family][tensor of a raw input], measured as the module docstring says (tests/test_raw_params_cpu.py repeats the measurement)
T = {
    "plain": {"dL_dopacity": 9.6e-07, "dL_dscales": 3.6e-06, "dL_drotations": 4.3e-06},
    "clamped": {"dL_dopacity": 9.6e-07, "dL_dscales": 5.9e-06, "dL_drotations": 6.1e-06},
    "rawquat": {"dL_dopacity": 9.6e-07, "dL_dscales": 3.1e-05, "dL_drotations": 5.2e-06},
    "needles10": {"dL_dopacity": 9.6e-07, "dL_dscales": 1.2e-05, "dL_drotations": 2.2e-04},
    "plain_ewa": {"dL_dopacity": 9.6e-07, "dL_dscales": 3.6e-06, "dL_drotations": 4.3e-06},
}
