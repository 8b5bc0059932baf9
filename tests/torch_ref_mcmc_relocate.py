"""Yardstick of the fused 3DGS-MCMC relocation and growth (include/stp_raster.h: stp_mcmc_sample, stp_mcmc_relocate_apply, stp_mcmc_add_apply;
mcmc_relocation_plan, mcmc_relocate_tensors_, mcmc_add_plan, mcmc_add_tensors), the float32 restatement of the kernels' raw path that fixes the
tolerances on the CPU, and the inputs the CPU measurement and the GPU tests share.  No reference code is involved: the semantics are the
issue's restatement of that trainer's relocate_gs and add_new_gs.

sample():   the inverse CDF over integer weights in int64 / float64 torch: cumsum and searchsorted(right=True).
relocate()/grow(): the two applies as plain indexed torch in float64, the new opacity and scaling from torch_ref_mcmc.relocation (the double loop).
stored_kernel_order(): what fresh_kernel of csrc/stp_mcmc_relocate.hip computes for a source, operation by operation, in numpy float32 around
torch_ref_mcmc.relocation_kernel_order -- sigmoid and exp first, the clamp, then log(o' / (1 - o')) and log(s').

Measured by tests/test_mcmc_relocate_cpu.py on exactly the GPU tests' inputs (numpy on the CPU), the error being |got - ref| / max(1, |ref|) of
the STORED opacity (a logit) and scaling (a logarithm) of every source row:
    restatement against the float64 yardstick, raw path                          2.0e-6   ->   RELOCATE_RAW_BOUND = 4 x = 8.0e-6
    float32 sigmoid weights against round(sigmoid64 * 2^24), integer units        2        ->   RELOCATE_RAW_WEIGHT_BOUND = 8
The factor 4 is the project's convention (torch_ref_mcmc.RELOCATION_BOUND): it covers the few-ulp differences between the device's and numpy's
expf / logf.  The error is that of 1 - o: the float32 sigmoid is good to 6e-8 of o, which is 6e-6 of 1 - o at the generators' largest live
opacity, 0.99 (and would be 6e-5 at 0.999, the limit check_opacities enforces), and the logit passes it on undiminished."""
import numpy as np
import torch

import torch_ref_mcmc as trm

MIN_OPACITY = 0.005
ONE_MINUS_EPS = 1.0 - float(np.finfo(np.float32).eps)
EXCLUSION = 1e-6              # no opacity lies this close to min_opacity: a one-ulp difference in the sigmoid cannot flip a row
MAX_SOURCE_OPACITY = 0.999    # of the tolerance tests
WEIGHT_ONE = float(2 ** 24)

RELOCATE_RAW_MEASURED, RELOCATE_RAW_BOUND = 2.0e-6, 8.0e-6
RELOCATE_RAW_WEIGHT_MEASURED, RELOCATE_RAW_WEIGHT_BOUND = 2, 8

SIZES = (1, 2, 63, 64, 65, 257, 2047, 2048, 2049, 4097, 100003)   # 2048: the scan's tile; 100003: several workgroups of every kernel


def f32(x):
    return float(np.float32(x))


# ---- sampling ----------------------------------------------------------------------------------------------------------------------------------

def activated64(opacity, raw):
    """the opacity in float64 from the float32 input: itself, or the float64 sigmoid of the stored logit"""
    o = opacity.detach().cpu().reshape(-1).to(torch.float64)
    return torch.sigmoid(o) if raw else o


def dead_rows(opacity, raw, min_opacity=MIN_OPACITY):
    """the float64 decision o <= min_opacity (min_opacity rounded to float32 once); NaN is not dead"""
    return activated64(opacity, raw) <= f32(min_opacity)


def weights_of(o, candidate):
    """round_to_nearest_even(clamp(o, 0, 1) * 2^24) as int64 where candidate, else 0 (torch.round rounds halves to even); NaN is never one"""
    o = torch.as_tensor(o, dtype=torch.float64)
    w = torch.round(o.nan_to_num(0.0).clamp(0.0, 1.0) * WEIGHT_ONE).to(torch.int64)
    return torch.where(candidate & ~torch.isnan(o), w, torch.zeros_like(w))


def relocation_weights(opacity, raw, min_opacity=MIN_OPACITY):
    """the weights of a relocation from float64 opacities: exact where raw is False (the product is exact in float32 too)"""
    o = activated64(opacity, raw)
    return weights_of(o, o > f32(min_opacity))


def growth_weights(opacity, raw):
    o = activated64(opacity, raw)
    return weights_of(o, torch.ones_like(o, dtype=torch.bool))


def draw(weights, uniforms):
    """One source per uniform: cumsum in int64, t = min(total - 1, floor(float64(u) * float64(total))), the smallest k with S_k > t.
    -> int64 sources, all -1 where the total weight is 0.  u is clamped into [0, 1): NaN and negatives are 0."""
    w = torch.as_tensor(weights).to(torch.int64).cpu()
    u = uniforms.detach().cpu().to(torch.float32)
    cum = torch.cumsum(w, 0)
    total = int(cum[-1]) if w.numel() else 0
    if total == 0:
        return torch.full((u.numel(),), -1, dtype=torch.int64)
    assert total < 2 ** 53
    below_one = torch.tensor(np.nextafter(np.float32(1.0), np.float32(0.0)))
    u = torch.where(u >= 0, u, torch.zeros_like(u))
    u = torch.where(u < 1, u, below_one.expand_as(u))
    t = torch.floor(u.to(torch.float64) * float(total)).to(torch.int64).clamp(max=total - 1)
    src = torch.searchsorted(cum, t, right=True)
    assert bool((w[src] > 0).all())
    return src


def sample_relocation(weights, dead, uniforms):
    """-> (src int64 (P,), count int64 (P,)): a draw on every dead row, -1 elsewhere"""
    P = dead.numel()
    src = torch.full((P,), -1, dtype=torch.int64)
    if bool(dead.any()):
        src[dead] = draw(weights, uniforms.detach().cpu()[dead])
    return src, count_of(src, P)


def sample_growth(weights, uniforms):
    src = draw(weights, uniforms)
    return src, count_of(src, torch.as_tensor(weights).numel())


def count_of(src, P):
    return torch.bincount(src[src >= 0], minlength=P)


# ---- the applies, float64 ----------------------------------------------------------------------------------------------------------------------

def new_values(opacity, scaling, count, raw, min_opacity=MIN_OPACITY):
    """-> (rows k with count > 0, their stored opacity (n,), their stored scaling (n, 3)) in float64: compute_relocation's formulas for
    N = count + 1 (clamped to 50 inside), the clamp, and the inverse activations where raw"""
    k = torch.nonzero(torch.as_tensor(count) > 0)[:, 0]
    if k.numel() == 0:
        return k, torch.zeros(0, dtype=torch.float64), torch.zeros(0, 3, dtype=torch.float64)
    o = activated64(opacity, raw)[k].numpy()
    s = scaling.detach().cpu().to(torch.float64).reshape(-1, 3)[k].numpy()
    if raw:
        s = np.exp(s)
    N = (torch.as_tensor(count)[k] + 1).numpy()
    # (the yardstick takes float32 inputs: in raw mode the float64 activations go in as they are)
    x = 1.0 - np.power(1.0 - o, 1.0 / trm.clamp_N(N))
    coef = o / trm.denominator_double_loop(x, trm.clamp_N(N))
    o_new = np.clip(x, f32(min_opacity), ONE_MINUS_EPS)
    s_new = coef[:, None] * s
    if raw:
        o_new, s_new = np.log(o_new / (1.0 - o_new)), np.log(s_new)
    return k, torch.from_numpy(o_new), torch.from_numpy(s_new)


def _scatter_new(out, role, rows, from_rows, k, o_new, s_new):
    """out[rows] = the new value of source rows from_rows (a subset of k)"""
    pos = torch.full((int(max(int(k.max()) + 1 if k.numel() else 0, 1)),), -1, dtype=torch.int64)
    pos[k] = torch.arange(k.numel())
    new = o_new if role == "opacity" else s_new
    out[rows] = new[pos[from_rows]].reshape(out[rows].shape)


def relocate(tensors, roles, moments, src, count, raw, min_opacity=MIN_OPACITY, reset_dead_moments=False):
    """tensors: list of float32 (P, ...); moments: list of (exp_avg, exp_avg_sq) or None -> (float64 tensors, float64 moment pairs) after the
    in-place relocation, as plain indexed torch"""
    src, count = torch.as_tensor(src).to(torch.int64).cpu(), torch.as_tensor(count).to(torch.int64).cpu()
    k, o_new, s_new = new_values(tensors[roles.index("opacity")], tensors[roles.index("scaling")], count, raw, min_opacity)
    drawn = count > 0
    dead = (src >= 0) & ~drawn
    out_t, out_m = [], []
    for t, role, mv in zip(tensors, roles, moments):
        old = t.detach().cpu().to(torch.float64)
        new = old.clone()
        new[dead] = old[src[dead]]
        if role != "plain":
            _scatter_new(new, role, k, k, k, o_new, s_new)
            _scatter_new(new, role, torch.nonzero(dead)[:, 0], src[dead], k, o_new, s_new)
        out_t.append(new)
        if mv is None:
            out_m.append(None)
            continue
        pair = []
        for m in mv:
            m = m.detach().cpu().to(torch.float64).clone()
            m[drawn] = 0.0
            if reset_dead_moments:
                m[dead] = 0.0
            pair.append(m)
        out_m.append(tuple(pair))
    return out_t, out_m


def grow(tensors, roles, moments, src, count, raw, min_opacity=MIN_OPACITY):
    """-> (float64 tensors of P + n rows, float64 moment pairs): rows [0, P) with the drawn rows rewritten, then one row per draw"""
    src, count = torch.as_tensor(src).to(torch.int64).cpu(), torch.as_tensor(count).to(torch.int64).cpu()
    k, o_new, s_new = new_values(tensors[roles.index("opacity")], tensors[roles.index("scaling")], count, raw, min_opacity)
    drawn = count > 0
    P, n = count.numel(), src.numel()
    there = src >= 0
    out_t, out_m = [], []
    for t, role, mv in zip(tensors, roles, moments):
        old = t.detach().cpu().to(torch.float64)
        new = torch.zeros((P + n,) + tuple(old.shape[1:]), dtype=torch.float64)
        new[:P] = old
        new[P:][there] = old[src[there]]
        if role != "plain":
            _scatter_new(new, role, k, k, k, o_new, s_new)
            _scatter_new(new, role, P + torch.nonzero(there)[:, 0], src[there], k, o_new, s_new)
        out_t.append(new)
        if mv is None:
            out_m.append(None)
            continue
        pair = []
        for m in mv:
            big = torch.zeros_like(new)
            big[:P] = m.detach().cpu().to(torch.float64)
            big[:P][drawn] = 0.0
            pair.append(big)
        out_m.append(tuple(pair))
    return out_t, out_m


# ---- the kernel's own order, float32 -----------------------------------------------------------------------------------------------------------

def sigmoid32(x):
    one = np.float32(1)
    with np.errstate(all="ignore"):
        return one / (one + np.exp(-np.asarray(x, np.float32)))


def weights_kernel_order(opacity, raw, candidate):
    """the kernel's weights: the float32 sigmoid where raw, then rint(o * 2^24) (exact in float32)"""
    o = np.asarray(opacity, np.float32).reshape(-1)
    o = sigmoid32(o) if raw else o
    w = np.rint(np.clip(np.nan_to_num(o, nan=0.0), 0.0, 1.0).astype(np.float32) * np.float32(WEIGHT_ONE)).astype(np.int64)
    return np.where(candidate, w, 0)


def stored_kernel_order(opacity, scaling, count, raw, min_opacity=MIN_OPACITY):
    """-> (rows k with count > 0, stored opacity (n,) float32, stored scaling (n, 3) float32) as fresh_kernel evaluates them"""
    count = np.asarray(count).astype(np.int64)
    k = np.nonzero(count > 0)[0]
    if k.size == 0:
        return k, np.zeros(0, np.float32), np.zeros((0, 3), np.float32)
    o = np.asarray(opacity, np.float32).reshape(-1)[k]
    s = np.asarray(scaling, np.float32).reshape(-1, 3)[k]
    if raw:
        o, s = sigmoid32(o), np.exp(s)
    o_new, s_new = trm.relocation_kernel_order(o, s, count[k] + 1)
    o_new = np.minimum(np.maximum(o_new, np.float32(min_opacity)), np.float32(ONE_MINUS_EPS))
    if raw:
        o_new, s_new = np.log(o_new / (np.float32(1) - o_new)), np.log(s_new)
    assert o_new.dtype == s_new.dtype == np.float32
    return k, o_new, s_new


def stored_error(got, ref):
    """the worst |got - ref| / max(1, |ref|)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))) if ref.size else 0.0


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------

TRAILING = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
NAMES = tuple(TRAILING)
ROLES = tuple(n if n in ("opacity", "scaling") else "plain" for n in NAMES)


def check_opacities(opacity, raw, min_opacity=MIN_OPACITY, sources_below=MAX_SOURCE_OPACITY):
    """the two guarantees of the generators, asserted where the CPU run sees them"""
    o = activated64(opacity, raw)
    o = o[~torch.isnan(o)]
    assert bool(((o - f32(min_opacity)).abs() > EXCLUSION).all()), "an opacity lies within the exclusion band around min_opacity"
    if sources_below is not None:
        assert bool((o[o > f32(min_opacity)] <= sources_below).all()), "a source opacity above the tolerance tests' limit"


def model_inputs(P, raw, seed=40, dead_every=9, names=NAMES):
    """dict name -> float32 tensor (P, *TRAILING[name]) of a model in its stored form (raw: logits and log-scales), with about one row in
    dead_every dead (opacity in [0, 0.004], an exact 0 among them) and the live opacities in [0.01, 0.99]; plus "uniforms" (P,) in [0, 1) and,
    per name, the moments "m_" + name and "v_" + name (non-zero everywhere).  A smaller P is not a prefix of a larger one.  names: the tensors
    to make (a test of the sampling alone at a large P needs the opacity only)."""
    rng = np.random.default_rng(seed + 7 * P + int(raw))
    o = rng.uniform(0.01, 0.99, P)
    dead = rng.integers(0, dead_every, P) == 0
    if P >= 2:
        dead[0], dead[1] = True, False   # work whatever the draw
    o[dead] = rng.uniform(0.0, 0.004, int(dead.sum()))
    if P >= 64:
        o[np.nonzero(dead)[0][-1]] = 0.0
    o = o.astype(np.float32)
    s = np.exp(rng.uniform(-6.0, 1.0, (P, 3))).astype(np.float32)
    out = {}
    for name, shape in TRAILING.items():
        if name not in names:
            continue
        out[name] = torch.from_numpy(rng.standard_normal((P,) + shape).astype(np.float32))
    with np.errstate(all="ignore"):
        logit = (np.log(o.astype(np.float64)) - np.log1p(-o.astype(np.float64))).astype(np.float32)
    out["opacity"] = torch.from_numpy(logit if raw else o).reshape(P, 1)
    out["scaling"] = torch.from_numpy(np.log(s.astype(np.float64)).astype(np.float32) if raw else s)
    for name, shape in TRAILING.items():
        if name not in names:
            continue
        out["m_" + name] = torch.from_numpy(rng.uniform(0.5, 1.5, (P,) + shape).astype(np.float32) * np.where(rng.integers(0, 2, (P,) + shape) == 0, -1, 1).astype(np.float32))
        out["v_" + name] = torch.from_numpy(rng.uniform(0.5, 1.5, (P,) + shape).astype(np.float32))
    out["uniforms"] = torch.from_numpy(rng.uniform(0.0, 1.0, P).astype(np.float32)).clamp(max=float(np.nextafter(np.float32(1), np.float32(0))))
    check_opacities(out["opacity"], raw)
    return out


def growth_uniforms(P, n, seed=50):
    rng = np.random.default_rng(seed + 3 * P + n)
    return torch.from_numpy(rng.uniform(0.0, 1.0, n).astype(np.float32)).clamp(max=float(np.nextafter(np.float32(1), np.float32(0))))


def lists_of(inp):
    """-> (tensors, roles, moments) in NAMES' order"""
    return [inp[n] for n in NAMES], list(ROLES), [(inp["m_" + n], inp["v_" + n]) for n in NAMES]
