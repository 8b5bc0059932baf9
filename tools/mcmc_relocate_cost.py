#!/usr/bin/env python3
"""Cost of 3DGS-MCMC's relocate_gs and add_new_gs on an optimizer: the torch compositions against the fused mcmc_relocate_ / mcmc_add_new (GPU box).
usage: tools/mcmc_relocate_cost.py [--sizes 1000000 6000000] [--steps 20] [--rounds 5]

The model is a trainer's: xyz (P, 3), f_dc (P, 1, 3), f_rest (P, 15, 3), opacity (P, 1), scaling (P, 3), rotation (P, 4) in their stored form, one
named optimizer group per tensor (torch.optim.Adam), exp_avg and exp_avg_sq present: 59 floats per Gaussian, three times.  Cases:
  relocate_torch   examples/train_render.py's relocate_dead(): dead = sigmoid(_opacity) <= 0.005, int(dead.sum()), two nonzero, torch.multinomial,
                   bincount, compute_relocation, one indexed copy per parameter and per moment
  relocate_fused   mcmc_relocate_(optimizer, uniforms, reset_dead_moments=True): four sampling kernels, one pass over the sources, one apply
  add_torch        upstream's add_new_gs as torch: multinomial over all rows, bincount, compute_relocation, indexed writes of the sources'
                   opacity and scaling, torch.cat of every parameter with its sampled rows and of both moments with zeros, zeroed source moments
  add_fused        mcmc_add_new's work on the same tensors: mcmc_add_plan + mcmc_add_tensors (the optimizer surgery around it is host code)
5 % of the rows are dead for the relocation; the growth adds 5 %.  Every timed call first restores _opacity and _scaling (two copies, in every
case alike), so that each call meets the same model.  The uniforms of the fused cases are drawn once outside the timed window, as
torch.multinomial's random numbers are drawn inside it: the fused figures exclude one torch.rand of P (relocation) or 0.05 P (growth) floats.
Every case is timed with events around `steps` calls after three warm-up calls; the cases alternate `rounds` times; per round and as medians.
The host synchronisations of one call of each case are counted with torch.cuda.set_sync_debug_mode and reported apart from the time."""
import argparse
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stopthepop-rasterization_amd")); sys.path.insert(0, ROOT)
import torch
import diff_gaussian_rasterization as dgr

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="*", default=[1_000_000, 6_000_000])
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/mcmc_relocate_cost.py measures on a GPU; there is none")
dev = torch.device("cuda:0")
MIN_OPACITY = 0.005
SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
ROLES = [n if n in ("opacity", "scaling") else "plain" for n in SHAPES]


def timed(step, steps):
    for _ in range(3):
        step()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def host_syncs(step):
    """the synchronising calls torch reports for one call of step (None where the debug mode is not available)"""
    try:
        torch.cuda.set_sync_debug_mode("warn")
    except Exception:
        return None
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            step()
        return sum("synchroniz" in str(w.message).lower() for w in caught)
    finally:
        torch.cuda.set_sync_debug_mode("default")


def model(P):
    gen = torch.Generator(device=dev).manual_seed(1)
    params = {n: torch.nn.Parameter(torch.randn(P, *s, device=dev, generator=gen)) for n, s in SHAPES.items()}
    o = torch.rand(P, 1, device=dev, generator=gen) * 0.98 + 0.01
    o[torch.rand(P, device=dev, generator=gen) < 0.05] = 0.002   # 5 % dead
    with torch.no_grad():
        params["opacity"].copy_(torch.logit(o))
        params["scaling"].copy_(torch.rand(P, 3, device=dev, generator=gen) * 7 - 6)
    opt = torch.optim.Adam([{"params": [p], "lr": 0.0, "name": n} for n, p in params.items()], lr=0.0, eps=1e-15)
    for p in params.values():
        opt.state[p] = {"step": torch.tensor(1.0), "exp_avg": torch.randn_like(p), "exp_avg_sq": torch.rand_like(p)}
    return params, opt


@torch.no_grad()
def relocate_torch(params, opt):
    """examples/train_render.py: relocate_dead()"""
    opacity = torch.sigmoid(params["opacity"]).reshape(-1)
    dead = opacity <= MIN_OPACITY
    n_dead = int(dead.sum())
    if n_dead == 0 or n_dead == dead.numel():
        return 0
    dead_idx, alive_idx = dead.nonzero()[:, 0], (~dead).nonzero()[:, 0]
    sampled = alive_idx[torch.multinomial(opacity[alive_idx], n_dead, replacement=True)]
    ratio = torch.bincount(sampled, minlength=dead.numel())[sampled] + 1
    new_opacity, new_scaling = dgr.compute_relocation(torch.sigmoid(params["opacity"])[sampled], torch.exp(params["scaling"])[sampled], ratio)
    new_opacity = new_opacity.clamp(MIN_OPACITY, 1.0 - torch.finfo(torch.float32).eps)
    params["opacity"][sampled] = torch.log(new_opacity / (1.0 - new_opacity))
    params["scaling"][sampled] = torch.log(new_scaling)
    touched = torch.cat([sampled, dead_idx])
    for param in params.values():
        param[dead_idx] = param[sampled]
        state = opt.state.get(param)
        if state:
            state["exp_avg"][touched] = 0
            state["exp_avg_sq"][touched] = 0
    return n_dead


@torch.no_grad()
def add_torch(params, opt, n_new):
    """upstream's add_new_gs (its _sample_alives, _update_params and the optimizer's cat) as torch -> the new tensors and moments"""
    probs = torch.sigmoid(params["opacity"]).reshape(-1)
    idx = torch.multinomial(probs, n_new, replacement=True)
    ratio = torch.bincount(idx, minlength=probs.numel())[idx] + 1
    new_opacity, new_scaling = dgr.compute_relocation(torch.sigmoid(params["opacity"])[idx], torch.exp(params["scaling"])[idx], ratio)
    new_opacity = new_opacity.clamp(MIN_OPACITY, 1.0 - torch.finfo(torch.float32).eps)
    params["opacity"][idx] = torch.log(new_opacity / (1.0 - new_opacity))
    params["scaling"][idx] = torch.log(new_scaling)
    out = []
    for param in params.values():
        state = opt.state[param]
        state["exp_avg"][idx] = 0
        state["exp_avg_sq"][idx] = 0
        zeros = torch.zeros((n_new,) + param.shape[1:], device=dev)
        out.append((torch.cat([param, param[idx]]), torch.cat([state["exp_avg"], zeros]), torch.cat([state["exp_avg_sq"], zeros])))
    return out


def add_fused(params, opt, uniforms):
    tensors = list(params.values())
    plan = dgr.mcmc_add_plan(params["opacity"], uniforms)
    return dgr.mcmc_add_tensors(plan, tensors, ROLES, [opt.state[p]["exp_avg"] for p in tensors], [opt.state[p]["exp_avg_sq"] for p in tensors])


def size(P):
    params, opt = model(P)
    opacity0, scaling0 = params["opacity"].detach().clone(), params["scaling"].detach().clone()
    n_new = int(1.05 * P) - P
    gen = torch.Generator(device=dev).manual_seed(2)
    u_reloc, u_add = torch.rand(P, device=dev, generator=gen), torch.rand(n_new, device=dev, generator=gen)

    def restore():
        with torch.no_grad():
            params["opacity"].copy_(opacity0)
            params["scaling"].copy_(scaling0)

    def with_restore(f):
        def step():
            restore()
            return f()
        return step

    cases = {"relocate_torch": with_restore(lambda: relocate_torch(params, opt)),
             "relocate_fused": with_restore(lambda: dgr.mcmc_relocate_(opt, u_reloc, reset_dead_moments=True)),
             "add_torch": with_restore(lambda: add_torch(params, opt, n_new)),
             "add_fused": with_restore(lambda: add_fused(params, opt, u_add))}
    restore()
    n_dead = relocate_torch(params, opt)
    restore()
    plan = dgr.mcmc_relocate_(opt, u_reloc, reset_dead_moments=True)
    assert int((plan[0] >= 0).sum()) == n_dead
    syncs = {n: host_syncs(step) for n, step in cases.items()}
    ms = {n: [] for n in cases}
    for _ in range(args.rounds):
        for n, step in cases.items():
            ms[n].append(timed(step, args.steps))
            torch.cuda.empty_cache()
    med = {n: statistics.median(v) for n, v in ms.items()}
    print(f"P = {P}: {n_dead} dead rows relocated, {n_new} rows added; {args.rounds} alternating rounds of {args.steps} calls, ms per call")
    for n in cases:
        print(f"  {n:15s} median {med[n]:8.3f}  host synchronisations per call {syncs[n]}  rounds " + " ".join(f"{x:.3f}" for x in ms[n]))
    for a, b in (("relocate_fused", "relocate_torch"), ("add_fused", "add_torch")):
        faster = sum(f < t for f, t in zip(ms[a], ms[b]))
        print(f"  {a} / {b} = {med[a] / med[b]:.4f} ({a} faster in {faster} of {args.rounds} rounds)")


for P in args.sizes:
    size(P)
    torch.cuda.empty_cache()
