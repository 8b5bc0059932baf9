"""Yardstick of the densification kernels (include/stp_raster.h: stp_densify_stats, stp_densify_plan, stp_densify_scan, stp_densify_apply), in
plain numpy and torch, with the inputs the CPU measurement and the GPU tests share.

stats():   the per-step statistics in float32 -- sqrt(gx * gx + gy * gy) with every operation rounded to float32, as the kernel writes it out.
plan():    the rule in float32 (numpy's exp; the inputs of model_inputs() keep every compared value at least MARGIN away from its threshold,
           relative, so that an exp that differs in its last bits decides alike -- plan_margins() measures that).
apply():   torch.cat([t[K], t[C], t[S], t[S]]) per tensor, moments of the K rows copied and all others zero, the children's xyz and scaling in
           float64 from the float32 inputs:  xyz' = xyz + R(q / |q|) (s * noise),  scaling' = log(s / split_shrink)  (s = exp(scaling) where raw).
children_kernel_order(): what csrc/stp_densify.hip computes for the children, operation by operation, in float32 (a fused multiply-add is
           formed as the float64 product and sum rounded once -- exact product, one extra rounding at most in rare ties).
upstream_densify_and_prune(): a restatement of the 3DGS trainer's own sequence -- densify_and_clone, densification_postfix, densify_and_split
           with padded gradients, densification_postfix, prune_points(split mask), prune_points(opacity / world size) -- on a dict of tensors
           and their Adam moments, in the dtype of its inputs."""
import numpy as np
import torch

# The worst errors of children_kernel_order() against apply()'s float64 children on the inputs below (every size of SIZES, raw and not), as
# tests/test_densify_cpu.py measures them (rounded up to two digits), and the GPU tests' bounds: 4 times that.
#   xyz:     max(0, |xyz' - ref|_2 - ulp(|ref|_inf)) / (max(s) |noise|_2)
#   scaling: |scaling' - ref| / max(1, |ref|)
CHILD_XYZ_MEASURED, CHILD_XYZ_BOUND = 1.6e-7, 6.4e-7
CHILD_SCALING_MEASURED, CHILD_SCALING_BOUND = 1.6e-7, 6.4e-7

SIZES = (1, 63, 64, 65, 257, 4097)
MARGIN = 1e-4            # least relative distance of a compared value from its threshold in model_inputs()
SPLIT_SHRINK = 0.8 * 2
RULE = dict(grad_threshold=0.0002, percent_dense=0.01, extent=5.0, min_opacity=0.005, max_screen_size=20.5)
ROLES = {"xyz": 1, "scaling": 2, "rotation": 3}


def f32(x):
    return float(np.float32(x))


def rule_numbers(grad_threshold, percent_dense, extent, min_opacity, max_screen_size):
    """The six thresholds as the package rounds them (each to float32 once) and prune_big."""
    big = max_screen_size is not None
    return dict(grad_threshold=f32(grad_threshold), split_size=f32(float(percent_dense) * float(extent)), min_opacity=f32(min_opacity),
                max_screen_size=f32(max_screen_size if big else 0.0), max_world_size=f32(0.1 * float(extent)), split_shrink=f32(SPLIT_SHRINK), prune_big=big)


# ---- statistics ----------------------------------------------------------------------------------------------------------------------------

def stats(accum, denom, max_radii2D, grad2d, radii):
    """-> (accum, denom, max_radii2D or None) after one step, float32 copies; radii: int32 radii (> 0 = visible) or a bool / uint8 mask."""
    accum, denom = np.array(accum, np.float32).reshape(-1), np.array(denom, np.float32).reshape(-1)
    radii = np.asarray(radii).reshape(-1)
    vis = radii > 0 if radii.dtype == np.int32 else radii != 0
    g = np.asarray(grad2d, np.float32)
    with np.errstate(all="ignore"):
        norm = np.sqrt((g[:, 0] * g[:, 0]).astype(np.float32) + (g[:, 1] * g[:, 1]).astype(np.float32), dtype=np.float32)
        accum[vis] = (accum[vis] + norm[vis]).astype(np.float32)
    denom[vis] = denom[vis] + np.float32(1)
    if max_radii2D is not None:
        max_radii2D = np.array(max_radii2D, np.float32).reshape(-1)
        max_radii2D[vis] = np.maximum(max_radii2D[vis], radii[vis].astype(np.float32))
    return accum, denom, max_radii2D


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------

def _activated(scaling, opacity, raw, dtype):
    s, o = np.asarray(scaling, np.float32).astype(dtype), np.asarray(opacity, np.float32).astype(dtype).reshape(-1)
    if raw:
        one = dtype(1)
        with np.errstate(all="ignore"):
            s, o = np.exp(s), one / (one + np.exp(-o))
    return s, o


def _compared(accum, denom, scaling, opacity, raw, shrink, dtype):
    accum, denom = np.asarray(accum, np.float32).reshape(-1), np.asarray(denom, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        g = np.where(denom > 0, (accum / denom).astype(np.float32), np.float32(0)).astype(dtype)
    s, o = _activated(scaling, opacity, raw, dtype)
    smax = s.max(axis=1)
    return g, smax, (smax / dtype(shrink)).astype(dtype), o


def plan(accum, denom, scaling, opacity, max_radii2D=None, *, grad_threshold, percent_dense=0.01, extent, min_opacity=0.005, max_screen_size=None, raw=True):
    """-> uint8 (P,): K | C << 1 | S << 2, the rule of include/stp_raster.h in float32."""
    r = rule_numbers(grad_threshold, percent_dense, extent, min_opacity, max_screen_size)
    g, smax, smax_child, o = _compared(accum, denom, scaling, opacity, raw, r["split_shrink"], np.float32)
    hot = g >= np.float32(r["grad_threshold"])
    clone, split = hot & (smax <= np.float32(r["split_size"])), hot & (smax > np.float32(r["split_size"]))
    low = o < np.float32(r["min_opacity"])
    big = r["prune_big"]
    ws, ws_child = big & (smax > np.float32(r["max_world_size"])), big & (smax_child > np.float32(r["max_world_size"]))
    vs = np.zeros_like(low) if (max_radii2D is None or not big) else np.asarray(max_radii2D, np.float32).reshape(-1) > np.float32(r["max_screen_size"])
    K, C, S = ~split & ~(low | ws | vs), clone & ~(low | ws), split & ~(low | ws_child)
    return (K.astype(np.uint8) | (C.astype(np.uint8) << 1) | (S.astype(np.uint8) << 2)).astype(np.uint8)


def plan_margins(accum, denom, scaling, opacity, max_radii2D, *, grad_threshold, percent_dense=0.01, extent, min_opacity=0.005, max_screen_size=None, raw=True):
    """The least relative distance |value - threshold| / threshold of every comparison the rule makes, in float64."""
    r = rule_numbers(grad_threshold, percent_dense, extent, min_opacity, max_screen_size)
    g, smax, smax_child, o = _compared(accum, denom, scaling, opacity, raw, r["split_shrink"], np.float64)
    d = [np.abs(g - r["grad_threshold"]) / r["grad_threshold"], np.abs(smax - r["split_size"]) / r["split_size"], np.abs(o - r["min_opacity"]) / r["min_opacity"]]
    if r["prune_big"]:
        d += [np.abs(smax - r["max_world_size"]) / r["max_world_size"], np.abs(smax_child - r["max_world_size"]) / r["max_world_size"]]
        if max_radii2D is not None:
            d.append(np.abs(np.asarray(max_radii2D, np.float64).reshape(-1) - r["max_screen_size"]) / r["max_screen_size"])
    return float(min(x.min() for x in d))


# ---- the apply -----------------------------------------------------------------------------------------------------------------------------

def _rotation(q):
    q = q / np.sqrt((q * q).sum(axis=1))[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3), q.dtype)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def children(xyz, scaling, rotation, noise, split_shrink=SPLIT_SHRINK, raw=True):
    """The 2 n children of n split Gaussians, float64 from the float32 inputs: noise (2n, 3), child j of Gaussian r uses noise[j * n + r].
    -> (xyz' (2n, 3), scaling' (2n, 3), s (2n, 3) activated scales)"""
    xyz, sc, q, nz = (np.asarray(a, np.float32).astype(np.float64) for a in (xyz, scaling, rotation, noise))
    s = np.exp(sc) if raw else sc
    shrunk = s / f32(split_shrink)
    new_scaling = np.log(shrunk) if raw else shrunk
    R = _rotation(q)
    s2, R2, xyz2 = np.concatenate([s, s]), np.concatenate([R, R]), np.concatenate([xyz, xyz])
    return xyz2 + (R2 @ (s2 * nz)[:, :, None])[:, :, 0], np.concatenate([new_scaling, new_scaling]), s2


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def children_kernel_order(xyz, scaling, rotation, noise, split_shrink=SPLIT_SHRINK, raw=True):
    """The kernel's evaluation order in float32 -> (xyz' (2n, 3), scaling' (2n, 3))."""
    one, two = np.float32(1), np.float32(2)
    xyz, sc, q, nz = (np.asarray(a, np.float32) for a in (xyz, scaling, rotation, noise))
    s = np.exp(sc) if raw else sc
    shrunk = s / np.float32(split_shrink)
    new_scaling = np.log(shrunk) if raw else shrunk
    norm = np.sqrt(_fma(q[:, 3], q[:, 3], _fma(q[:, 2], q[:, 2], _fma(q[:, 1], q[:, 1], q[:, 0] * q[:, 0]))))
    r, a, b, c = (q[:, j] / norm for j in range(4))
    R = np.empty((q.shape[0], 3, 3), np.float32)
    R[:, 0, 0] = one - two * _fma(b, b, c * c); R[:, 0, 1] = two * _fma(a, b, -(r * c)); R[:, 0, 2] = two * _fma(a, c, r * b)
    R[:, 1, 0] = two * _fma(a, b, r * c); R[:, 1, 1] = one - two * _fma(a, a, c * c); R[:, 1, 2] = two * _fma(b, c, -(r * a))
    R[:, 2, 0] = two * _fma(a, c, -(r * b)); R[:, 2, 1] = two * _fma(b, c, r * a); R[:, 2, 2] = one - two * _fma(a, a, b * b)
    s2, R2, xyz2 = np.concatenate([s, s]), np.concatenate([R, R]), np.concatenate([xyz, xyz])
    t = s2 * nz
    out = np.stack([xyz2[:, j] + _fma(R2[:, j, 2], t[:, 2], _fma(R2[:, j, 1], t[:, 1], R2[:, j, 0] * t[:, 0])) for j in range(3)], axis=1)
    assert out.dtype == np.float32 and new_scaling.dtype == np.float32
    return out, np.concatenate([new_scaling, new_scaling])


def child_errors(got_xyz, got_scaling, xyz, scaling, rotation, noise, split_shrink=SPLIT_SHRINK, raw=True):
    """-> (worst xyz ratio, worst scaling ratio) of children against the float64 yardstick, in the measures stated at the top."""
    ref_xyz, ref_scaling, s = children(xyz, scaling, rotation, noise, split_shrink, raw)
    if ref_xyz.shape[0] == 0:
        return 0.0, 0.0
    err = np.linalg.norm(np.asarray(got_xyz, np.float64) - ref_xyz, axis=1)
    ulp = np.spacing(np.abs(ref_xyz).max(axis=1).astype(np.float32)).astype(np.float64)
    scale = s.max(axis=1) * np.linalg.norm(np.asarray(noise, np.float64), axis=1)
    assert np.all(scale > 0)
    ex = float(np.max(np.maximum(err - ulp, 0.0) / scale))
    es = float(np.max(np.abs(np.asarray(got_scaling, np.float64) - ref_scaling) / np.maximum(1.0, np.abs(ref_scaling))))
    return ex, es


def plan_rows(plan_bytes):
    """-> (K, C, S) index arrays of a plan"""
    p = np.asarray(plan_bytes).astype(np.uint8)
    return np.nonzero(p & 1)[0], np.nonzero(p & 2)[0], np.nonzero(p & 4)[0]


def apply(plan_bytes, tensors, roles, exp_avgs, exp_avg_sqs, noise, split_shrink=SPLIT_SHRINK, raw=True):
    """-> (new tensors, new exp_avgs, new exp_avg_sqs) as float64 arrays (copies are exact in float64): torch.cat([t[K], t[C], t[S], t[S]])
    with the children's xyz and scaling replaced; moments None where none was given."""
    K, C, S = plan_rows(plan_bytes)
    rows = np.concatenate([K, C, S, S])
    first_child = K.size + C.size
    role_t = {r: np.asarray(t, np.float32) for t, r in zip(tensors, roles) if r}
    kids = children(role_t[1][S], role_t[2][S], role_t[3][S], noise, split_shrink, raw) if S.size else None
    out_t, out_m, out_v = [], [], []
    for t, role, m, v in zip(tensors, roles, exp_avgs, exp_avg_sqs):
        new = np.asarray(t, np.float32).astype(np.float64)[rows]
        if S.size and role in (1, 2):
            new[first_child:] = kids[role - 1]
        out_t.append(new)
        for src, dst in ((m, out_m), (v, out_v)):
            if src is None:
                dst.append(None)
                continue
            z = np.zeros_like(new)
            z[:K.size] = np.asarray(src, np.float32).astype(np.float64)[K]
            dst.append(z)
    return out_t, out_m, out_v


# ---- upstream's own sequence -----------------------------------------------------------------------------------------------------------------

def _build_rotation(r):
    q = r / torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])[:, None]
    R = torch.zeros((q.size(0), 3, 3), dtype=r.dtype)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def upstream_densify_and_prune(tensors, exp_avgs, exp_avg_sqs, accum, denom, noise_pool, *, grad_threshold, percent_dense=0.01, extent, min_opacity=0.005,
                               max_screen_size=None):
    """The trainer's densify_and_prune on dicts {name: torch tensor} with the names xyz, scaling, rotation, opacity (raw parameters) and any
    others; exp_avgs / exp_avg_sqs: dicts of the moments (a missing name: no state).  noise_pool: (2, P, 3) standard normal draws, [j, i] for
    child j of Gaussian i -- what upstream takes from torch.normal(0, stds) as stds * noise.  Upstream splits EVERY hot, large Gaussian and
    prunes the children of some again (low opacity, too large), so its draws are indexed by the Gaussian here; the package's noise for the
    surviving split rows S is split_noise(noise_pool, S).  The thresholds are the package's float32-rounded ones.  -> (tensors, exp_avgs,
    exp_avg_sqs) after it, new dicts."""
    r = rule_numbers(grad_threshold, percent_dense, extent, min_opacity, max_screen_size)
    t = {k: v.clone() for k, v in tensors.items()}
    m = {k: v.clone() for k, v in exp_avgs.items()}
    v2 = {k: v.clone() for k, v in exp_avg_sqs.items()}
    dt = t["xyz"].dtype

    def cat(ext):     # cat_tensors_to_optimizer
        for k in t:
            t[k] = torch.cat([t[k], ext[k]], dim=0)
            if k in m:
                m[k] = torch.cat([m[k], torch.zeros_like(ext[k])], dim=0)
                v2[k] = torch.cat([v2[k], torch.zeros_like(ext[k])], dim=0)

    def prune(mask):  # prune_points
        keep = ~mask
        for k in t:
            t[k] = t[k][keep]
            if k in m:
                m[k], v2[k] = m[k][keep], v2[k][keep]

    grads = (torch.as_tensor(np.asarray(accum, np.float32).reshape(-1, 1)) / torch.as_tensor(np.asarray(denom, np.float32).reshape(-1, 1))).to(dt)
    grads[grads.isnan()] = 0.0
    get_scaling = lambda: torch.exp(t["scaling"])
    # densify_and_clone
    mask = (torch.norm(grads, dim=-1) >= r["grad_threshold"]) & (get_scaling().max(dim=1).values <= r["split_size"])
    cat({k: x[mask] for k, x in t.items()})
    # densify_and_split
    n_init = t["xyz"].size(0)
    padded = torch.zeros(n_init, dtype=dt)
    padded[:grads.size(0)] = grads.squeeze()
    mask = (padded >= r["grad_threshold"]) & (get_scaling().max(dim=1).values > r["split_size"])
    stds = get_scaling()[mask].repeat(2, 1)
    pool = torch.as_tensor(np.asarray(noise_pool, np.float32)).to(dt).reshape(2, -1, 3)
    samples = stds * pool[:, mask[:pool.size(1)]].reshape(-1, 3)
    rots = _build_rotation(t["rotation"][mask]).repeat(2, 1, 1)
    ext = {k: x[mask].repeat(2, *([1] * (x.dim() - 1))) for k, x in t.items()}
    ext["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + t["xyz"][mask].repeat(2, 1)
    ext["scaling"] = torch.log(get_scaling()[mask].repeat(2, 1) / r["split_shrink"])
    cat(ext)
    prune(torch.cat([mask, torch.zeros(2 * int(mask.sum()), dtype=torch.bool)]))
    # the prune of densify_and_prune (max_radii2D was zeroed by densification_postfix: the screen-size test never fires)
    mask = (torch.sigmoid(t["opacity"]) < r["min_opacity"]).reshape(-1)
    if max_screen_size is not None:
        mask = mask | (get_scaling().max(dim=1).values > r["max_world_size"])
    prune(mask)
    return t, m, v2


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------

GROUPS = (("xyz", (3,)), ("f_dc", (1, 3)), ("f_rest", (15, 3)), ("opacity", (1,)), ("scaling", (3,)), ("rotation", (4,)))   # a 3DGS model's six groups


def model_inputs(P, seed=0, rule=RULE):
    """dict of float32 arrays for P Gaussians: the six parameter tensors of GROUPS (raw scaling U[-6, 0.5], raw opacity U[-7, 4], quaternions of
    random direction and norm in [0.2, 3]), both Adam moments of each ("m_<name>", "v_<name>", non-zero), the statistics accum / denom /
    max_radii2D (denom in 0..10 with zeros, where accum is zero too; accum / denom log-uniform around the threshold) and a standard normal
    noise pool (2P, 3).  Rows whose compared values come within 10 MARGIN of a threshold are moved (raw scaling and opacity shifted, accum
    scaled) until none is left: test_densify_cpu.py asserts the margin itself."""
    rng = np.random.default_rng(1000 * seed + P)
    d = {}
    for name, shape in GROUPS:
        d[name] = rng.standard_normal((P,) + shape).astype(np.float32)
        d["m_" + name] = (0.1 * rng.standard_normal((P,) + shape)).astype(np.float32)
        d["v_" + name] = (0.01 * rng.uniform(0.1, 1.0, (P,) + shape)).astype(np.float32)
    d["xyz"] = rng.uniform(-5.0, 5.0, (P, 3)).astype(np.float32)
    d["scaling"] = rng.uniform(-6.0, 0.5, (P, 3)).astype(np.float32)
    d["opacity"] = rng.uniform(-7.0, 4.0, (P, 1)).astype(np.float32)
    q = rng.standard_normal((P, 4))
    d["rotation"] = (q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.2, 3.0, (P, 1))).astype(np.float32)
    denom = rng.integers(0, 11, P).astype(np.float32)
    g = rule["grad_threshold"] * np.exp(rng.uniform(-2.0, 2.0, P))
    d["denom"] = denom
    d["accum"] = (g * denom).astype(np.float32)
    d["max_radii2D"] = rng.integers(0, 41, P).astype(np.float32)
    d["noise"] = rng.standard_normal((2 * P, 3)).astype(np.float32)
    r = rule_numbers(**rule)
    for _ in range(50):
        g, smax, smax_child, o = _compared(d["accum"], d["denom"], d["scaling"], d["opacity"], True, r["split_shrink"], np.float64)
        near = lambda x, thr: np.abs(x - thr) / thr < 10 * MARGIN
        bad_s = near(smax, r["split_size"]) | near(smax, r["max_world_size"]) | near(smax_child, r["max_world_size"])
        bad_o, bad_g = near(o, r["min_opacity"]), near(g, r["grad_threshold"])
        if not (bad_s.any() or bad_o.any() or bad_g.any()):
            break
        d["scaling"][bad_s] += np.float32(0.01)
        d["opacity"][bad_o] += np.float32(0.05)
        d["accum"][bad_g] *= np.float32(1.01)
    else:
        raise AssertionError("model_inputs: could not place the inputs")
    return d


def split_noise(noise_pool, S):
    """The (2 nS, 3) noise of the split rows S out of a pool (2, P, 3) indexed by the Gaussian: row j * nS + r is pool[j, S[r]]."""
    pool = np.asarray(noise_pool, np.float32)
    return np.ascontiguousarray(pool.reshape(2, -1, 3)[:, S].reshape(-1, 3))


def model_plan(d, with_radii=False, rule=RULE):
    return plan(d["accum"], d["denom"], d["scaling"], d["opacity"], d["max_radii2D"] if with_radii else None, **rule)
