#!/usr/bin/env python3
"""Cost of 3DGS adaptive density control: upstream's torch composition against the fused densification calls (GPU box).
usage: tools/densify_cost.py [--counts 1000000 6000000] [--steps 3] [--stat-steps 50] [--rounds 5]

A model of P Gaussians with SH degree 3 (xyz, f_dc, f_rest (P, 15, 3), opacity, scaling, rotation: 59 floats per Gaussian) and both Adam
moments of every tensor.  About 8.5 % of the Gaussians are cloned, 0.8 % split and 10 % removed.  Cases:
  statistics: torch     stat[vis] += grad[vis, :2].norm(dim=-1, keepdim=True); denom[vis] += 1; max_radii2D[vis] = max(max_radii2D[vis], radii[vis])
              fused     densification_stats_(stat, denom, max_radii2D, grad, radii): one kernel, no synchronisation
  densify_and_prune:
              torch     upstream's sequence on the tensors and moments: densify_and_clone, densification_postfix (cat), densify_and_split with
                        padded gradients, postfix, prune_points(split mask), prune_points(opacity / world size)
              fused     densify_plan + densify_tensors (scan, apply): 5 kernels, one synchronisation
Both densify cases start from the same tensors (which they do not modify) and allocate their outputs inside the timed window.  The normal
draws are made once outside it, one pair per Gaussian; each case gets the rows of the Gaussians IT splits, gathered outside the window too
(upstream splits every hot, large Gaussian and prunes some children again; the plan splits only those whose children stay), so that both
give the same model.  Every case is timed with events around `steps` calls after two warm-up calls; the cases alternate `rounds` times;
per round and as medians.  For the fused apply also its algorithmic bytes (parameter and moments of the kept rows read, parameters of the copied and split
rows read, all output rows written) over the time of the whole fused call, as a fraction of the stp_hbm_probe copy rate of the same run."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stopthepop-rasterization_amd")); sys.path.insert(0, ROOT)
import torch
import diff_gaussian_rasterization as dgr
from diff_gaussian_rasterization import _C

ap = argparse.ArgumentParser()
ap.add_argument("--counts", type=int, nargs="*", default=[1_000_000, 6_000_000])
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--stat-steps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/densify_cost.py measures on a GPU; there is none")
dev = torch.device("cuda:0")
GROUPS = (("xyz", (3,)), ("f_dc", (1, 3)), ("f_rest", (15, 3)), ("opacity", (1,)), ("scaling", (3,)), ("rotation", (4,)))
RULE = dict(grad_threshold=0.0002, percent_dense=0.01, extent=5.0, min_opacity=0.005, max_screen_size=20.0)
FLOATS = 59


def timed(step, steps, warm=2):
    for _ in range(warm):
        step()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def copy_rate():
    """TB/s of the library's float4 copy kernel on 1 GiB (read + write bytes), best of 10 over a few grids"""
    x, y = torch.ones(1 << 28, device=dev), torch.empty(1 << 28, device=dev)
    best = float("inf")
    for blocks in (2048, 4096, 8192, 16384):
        for nt in (False, True):
            best = min(best, min(timed(lambda: _C.hbm_probe("copy", y, x, blocks=blocks, nontemporal=nt), 10) for _ in range(2)))
    return 2 * x.numel() * 4 / (best * 1e-3) / 1e12


def build_rotation(r):   # upstream utils/general_utils.py
    q = r / torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])[:, None]
    R = torch.zeros((q.size(0), 3, 3), device=r.device)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


@torch.no_grad()
def upstream(t, m, v, accum, denom, noise):
    """upstream's densify_and_prune on dicts of tensors and moments -> (tensors, exp_avgs, exp_avg_sqs)"""
    t, m, v = dict(t), dict(m), dict(v)
    split_size, world = RULE["percent_dense"] * RULE["extent"], 0.1 * RULE["extent"]

    def cat(ext):
        for k in t:
            t[k] = torch.cat([t[k], ext[k]], dim=0)
            m[k] = torch.cat([m[k], torch.zeros_like(ext[k])], dim=0)
            v[k] = torch.cat([v[k], torch.zeros_like(ext[k])], dim=0)

    def prune(mask):
        keep = ~mask
        for k in t:
            t[k], m[k], v[k] = t[k][keep], m[k][keep], v[k][keep]

    grads = accum / denom
    grads[grads.isnan()] = 0.0
    mask = (torch.norm(grads, dim=-1) >= RULE["grad_threshold"]) & (torch.exp(t["scaling"]).max(dim=1).values <= split_size)
    cat({k: x[mask] for k, x in t.items()})
    padded = torch.zeros(t["xyz"].size(0), device=dev)
    padded[:grads.size(0)] = grads.squeeze()
    mask = (padded >= RULE["grad_threshold"]) & (torch.exp(t["scaling"]).max(dim=1).values > split_size)
    stds = torch.exp(t["scaling"][mask]).repeat(2, 1)
    samples = stds * noise
    rots = build_rotation(t["rotation"][mask]).repeat(2, 1, 1)
    ext = {k: x[mask].repeat(2, *([1] * (x.dim() - 1))) for k, x in t.items()}
    ext["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + t["xyz"][mask].repeat(2, 1)
    ext["scaling"] = torch.log(torch.exp(t["scaling"][mask]).repeat(2, 1) / (0.8 * 2))
    cat(ext)
    prune(torch.cat([mask, torch.zeros(2 * int(mask.sum()), device=dev, dtype=torch.bool)]))
    mask = (torch.sigmoid(t["opacity"]) < RULE["min_opacity"]).squeeze() | (torch.exp(t["scaling"]).max(dim=1).values > world)
    prune(mask)
    return t, m, v


def report(name, ms, fused="fused", other="torch"):
    med = {n: statistics.median(x) for n, x in ms.items()}
    for n in ms:
        print(f"  {name} {n:6s} median {med[n]:.4f}  rounds " + " ".join(f"{x:.4f}" for x in ms[n]))
    faster = sum(f < t for f, t in zip(ms[fused], ms[other]))
    print(f"  {name} fused / torch = {med[fused] / med[other]:.4f} (fused faster in {faster} of {len(ms[fused])} rounds)")
    return med


def workload(P, rate):
    gen = torch.Generator(device=dev).manual_seed(1)
    rand = lambda *shape: torch.rand(*shape, device=dev, generator=gen)
    t = {n: torch.randn(P, *shape, device=dev, generator=gen) for n, shape in GROUPS}
    t["scaling"] = rand(P, 3) * 3 - 6.5                                   # max scale mostly below split_size = 0.05 ...
    big = rand(P) < 0.1
    t["scaling"][big] += 3.5                                              # ... 10 % above it
    t["opacity"] = torch.logit(rand(P, 1) * 0.98 + 0.01)
    t["opacity"][rand(P) < 0.05] = -6.0                                   # 5 % below min_opacity
    m = {n: torch.randn_like(x) * 0.1 for n, x in t.items()}
    v = {n: torch.rand_like(x) * 0.01 for n, x in t.items()}
    denom = torch.randint(1, 10, (P, 1), device=dev, generator=gen).float()
    accum = denom * RULE["grad_threshold"] * torch.where(rand(P, 1) < 0.1, 2.0, 0.5)     # 10 % hot
    max_radii = torch.zeros(P, device=dev)
    grad = torch.randn(P, 3, device=dev, generator=gen) * 1e-4
    radii = (torch.randint(1, 40, (P,), device=dev, generator=gen) * (rand(P) < 0.5)).int()
    pool = torch.randn(2, P, 3, device=dev, generator=gen)                # child j of Gaussian i draws pool[j, i]
    names = [n for n, _ in GROUPS]
    print(f"P = {P}: {args.rounds} alternating rounds, ms per call")

    # the statistics
    stat_t, den_t, mr_t = accum.clone(), denom.clone(), max_radii.clone()
    stat_f, den_f, mr_f = accum.clone(), denom.clone(), max_radii.clone()

    @torch.no_grad()
    def stats_torch():
        vis = radii > 0
        stat_t[vis] += torch.norm(grad[vis, :2], dim=-1, keepdim=True)
        den_t[vis] += 1
        mr_t[vis] = torch.max(mr_t[vis], radii[vis].float())

    def stats_fused():
        dgr.densification_stats_(stat_f, den_f, mr_f, grad, radii)

    ms = {"torch": [], "fused": []}
    for _ in range(args.rounds):
        ms["torch"].append(timed(stats_torch, args.stat_steps))
        ms["fused"].append(timed(stats_fused, args.stat_steps))
    same = bool(torch.equal(den_t, den_f) and torch.allclose(stat_t, stat_f, rtol=1e-6) and torch.equal(mr_t, mr_f))
    print(f"  statistics: both accumulate alike: {same}")
    report("statistics", ms)

    # densify_and_prune
    counts = [None]
    with torch.no_grad():
        hot_large = ((accum / denom).squeeze() >= RULE["grad_threshold"]) & (torch.exp(t["scaling"]).max(dim=1).values > RULE["percent_dense"] * RULE["extent"])
        noise_torch = pool[:, hot_large].reshape(-1, 3).contiguous()
        split = (dgr.densify_plan(accum, denom, t["scaling"], t["opacity"], None, **RULE) & 4) != 0
        noise_fused = pool[:, split].reshape(-1, 3).contiguous()

    def dens_torch():
        return upstream(t, m, v, accum, denom, noise_torch)

    def dens_fused():
        plan = dgr.densify_plan(accum, denom, t["scaling"], t["opacity"], None, **RULE)
        offsets, c = _C.densify_scan(plan)
        counts[0] = c
        return _C.densify_apply(plan, offsets, c, [t[n] for n in names], [_C.DENSIFY_ROLES.get(n, 0) for n in names], [m[n] for n in names],
                                [v[n] for n in names], noise_fused, 1.6, True)

    a, b = dens_torch(), dens_fused()
    nK, nC, nS = counts[0]
    agree = all(a[0][n].shape == b[0][k].shape and torch.allclose(a[0][n], b[0][k], rtol=1e-4, atol=1e-5) and torch.equal(a[1][n], b[1][k])
                for k, n in enumerate(names))
    print(f"  densify_and_prune: kept {nK}, cloned {nC}, split {nS} -> {nK + nC + 2 * nS} rows; both give the same model: {agree}")
    del a, b
    ms = {"torch": [], "fused": []}
    for _ in range(args.rounds):
        ms["torch"].append(timed(dens_torch, args.steps))
        ms["fused"].append(timed(dens_fused, args.steps))
    med = report("densify_and_prune", ms)
    moved = 4 * FLOATS * (3 * nK + nC + nS + 3 * (nK + nC + 2 * nS))
    achieved = moved / (med["fused"] * 1e-3) / 1e12
    print(f"  the fused apply moves {moved / 1e6:.1f} MB -> {achieved:.2f} TB/s over the whole fused call = {100.0 * achieved / rate:.1f} % of the copy rate")


print(f"stp_hbm_probe copy, 1 GiB, this box, this run: {(rate := copy_rate()):.2f} TB/s")
for P in args.counts:
    workload(P, rate)
    torch.cuda.empty_cache()
