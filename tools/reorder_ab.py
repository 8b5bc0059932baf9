#!/usr/bin/env python3
"""Does a model in Morton order render faster, and what does putting it there cost?  (GPU box.)
usage: tools/reorder_ab.py [--workloads C2 C5] [--steps 50] [--warmup 10] [--rounds 5] [--sizes 1000000 6000000] [--scale 1.0]

Part 1, the render: the forward + backward step of bench.py's C2 and C5 under the full StopThePop settings (hierarchical sort, PTD_MAX order,
every culling option, load balancing), through the public API, on four orders of the SAME Gaussians:
  a_generated    the scene as scenes.config makes it: positions from a counter hash, so the row order is random
  b_reordered    (a) through spatial_order + gather_tensors
  c_trained_like (b) with a seeded 30 % of the rows moved to the end in random order: what densification and relocation leave
  d_reordered    (c) through spatial_order + gather_tensors
Every variant keeps its own leaves resident; the variants alternate within the process, `rounds` times; every window is `warmup` untimed steps and
then `steps` steps between two device events.  Per variant: the median over the rounds, the smallest and the largest round.

Part 2, the call: reorder_gaussians_ on a torch.optim.Adam over a trainer's six tensors (59 floats per Gaussian) with exp_avg and exp_avg_sq, at
each of `sizes` rows; spatial_order and gather_tensors alone; and the same moves as one torch.index_select per stream (18 streams), the order
given.  Timed like part 1.

Part 3: for the pairs (a -> b) and (c -> d) of a workload, the steps after which one reorder_gaussians_ call of the nearest measured size has
paid for itself: cost / (step before - step after); "never" where the step did not get faster, and a remark where the gain is no larger than the
spread of the rounds it was measured in."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stopthepop-rasterization_amd")); sys.path.insert(0, ROOT)
import numpy as np
import torch
import diff_gaussian_rasterization as dgr
from diff_gaussian_rasterization import scenes

ap = argparse.ArgumentParser()
ap.add_argument("--workloads", nargs="*", default=["C2", "C5"])
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--sizes", type=int, nargs="*", default=[1_000_000, 6_000_000])
ap.add_argument("--scale", type=float, default=1.0, help="shrink the workloads (a dry run of the script; the figures then say nothing about C2 and C5)")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/reorder_ab.py measures on a GPU; there is none")
if args.steps < 50 and args.scale == 1.0:
    raise SystemExit("a window is at least 50 steps")
dev = torch.device("cuda:0")
NAMES = ("means3D", "opacities", "scales", "rotations", "shs")


def full_settings():
    es = dgr.ExtendedSettings()
    es.sort_settings.sort_mode = dgr.SortMode.HIER
    es.sort_settings.sort_order = dgr.GlobalSortOrder.PTD_MAX
    es.culling_settings.rect_bounding = es.culling_settings.tight_opacity_bounding = True
    es.culling_settings.tile_based_culling = es.culling_settings.hierarchical_4x4_culling = True
    es.load_balancing = True
    return es


def window(step, warmup, steps):
    for _ in range(warmup):
        step()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def alternate(cases, warmup, steps, rounds):
    ms = {n: [] for n in cases}
    for _ in range(rounds):
        for n, step in cases.items():
            ms[n].append(window(step, warmup, steps))
    return ms


def report(ms, unit="ms per step"):
    med = {n: statistics.median(v) for n, v in ms.items()}
    for n, v in ms.items():
        print(f"  {n:16s} median {med[n]:9.4f}  min {min(v):9.4f}  max {max(v):9.4f}  spread {(max(v) - min(v)) / med[n] * 100:5.2f} %  rounds " + " ".join(f"{x:.4f}" for x in v))
    return med


class Variant:
    def __init__(self, tensors, rs, w_img):
        self.leaves = [t.clone().requires_grad_(True) for t in tensors]
        self.means2D = torch.zeros_like(self.leaves[0], requires_grad=True)
        self.raster, self.w_img = dgr.GaussianRasterizer(rs), w_img

    def step(self):
        for x in self.leaves + [self.means2D]:
            x.grad = None
        m, o, s, r, sh = self.leaves
        color, radii = self.raster(m, self.means2D, o, shs=sh, scales=s, rotations=r)
        color.backward(self.w_img)
        self.visible = radii


def render_part(name):
    sc = scenes.config(name, scale=args.scale)
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    rs = dgr.GaussianRasterizationSettings(
        image_height=sc.H, image_width=sc.W, tanfovx=sc.tanfovx, tanfovy=sc.tanfovy, bg=t(sc.bg), scale_modifier=1.0, viewmatrix=t(sc.viewmatrix),
        projmatrix=t(sc.projmatrix), inv_viewprojmatrix=t(sc.inv_viewprojmatrix), sh_degree=sc.sh_degree, campos=t(sc.campos), prefiltered=False,
        settings=full_settings(), render_depth=False, debug=False)
    w_img = t(sc.dL_dout)
    a = [t(getattr(sc, n)) for n in NAMES]
    P = a[0].shape[0]
    b, _, _ = dgr.gather_tensors(dgr.spatial_order(a[0]), a)
    gen = torch.Generator().manual_seed(30)
    moved = torch.rand(P, generator=gen) < 0.3
    stay, go = (~moved).nonzero()[:, 0], moved.nonzero()[:, 0]
    index = torch.cat([stay, go[torch.randperm(go.numel(), generator=gen)]]).to(torch.int32).to(dev)
    c, _, _ = dgr.gather_tensors(index, b)
    d, _, _ = dgr.gather_tensors(dgr.spatial_order(c[0]), c)
    variants = {"a_generated": Variant(a, rs, w_img), "b_reordered": Variant(b, rs, w_img), "c_trained_like": Variant(c, rs, w_img), "d_reordered": Variant(d, rs, w_img)}
    del a, b, c, d
    for v in variants.values():
        v.step()
    visible = {n: int((v.visible > 0).sum()) for n, v in variants.items()}
    assert len(set(visible.values())) == 1, visible
    print(f"{name}-full{'' if args.scale == 1.0 else f' at scale {args.scale}'}: {P} Gaussians ({visible['a_generated']} visible), {sc.W}x{sc.H}, forward + backward; "
          f"{args.rounds} alternating rounds, windows of {args.warmup} + {args.steps} steps, ms per step; {int(moved.sum())} rows moved to the end for (c)")
    ms = alternate({n: v.step for n, v in variants.items()}, args.warmup, args.steps, args.rounds)
    med = report(ms)
    for before, after in (("a_generated", "b_reordered"), ("c_trained_like", "d_reordered")):
        faster = sum(y < x for x, y in zip(ms[before], ms[after]))
        print(f"  {after} / {before} = {med[after] / med[before]:.4f}   (gain {med[before] - med[after]:+.4f} ms per step; faster in {faster} of {args.rounds} rounds; "
              f"the larger spread of the two {max(max(ms[n]) - min(ms[n]) for n in (before, after)):.4f} ms)")
    return P, med, ms


SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}


def cost_part(P):
    gen = torch.Generator(device=dev).manual_seed(1)
    params = {n: torch.nn.Parameter(torch.randn(P, *s, device=dev, generator=gen)) for n, s in SHAPES.items()}
    opt = torch.optim.Adam([{"params": [p], "lr": 0.0, "name": n} for n, p in params.items()], lr=0.0, eps=1e-15)
    for p in params.values():
        opt.state[p] = {"step": torch.tensor(1.0), "exp_avg": torch.randn_like(p), "exp_avg_sq": torch.rand_like(p)}
    xyz = params["xyz"].detach().clone()           # (a random order at every call: the optimizer's own xyz is sorted after the first)
    order = dgr.spatial_order(xyz)
    order64 = order.long()

    def streams():
        ps = [g["params"][0] for g in opt.param_groups]
        return [p.detach() for p in ps], [opt.state[p]["exp_avg"] for p in ps], [opt.state[p]["exp_avg_sq"] for p in ps]

    def by_index_select():
        t, m, v = streams()
        return [torch.index_select(x, 0, order64) for x in t + m + v]

    cases = {"reorder_gaussians_": lambda: dgr.reorder_gaussians_(opt, order),
             "order + reorder": lambda: dgr.reorder_gaussians_(opt, dgr.spatial_order(xyz)),
             "spatial_order": lambda: dgr.spatial_order(xyz),
             "gather_tensors": lambda: dgr.gather_tensors(order, *streams()),
             "index_select x18": by_index_select}
    print(f"P = {P}: six tensors of 59 floats per Gaussian with exp_avg and exp_avg_sq ({P * 59 * 3 * 4 / 2 ** 20:.0f} MiB read and as much written); "
          f"{args.rounds} alternating rounds, windows of 3 + 20 calls, ms per call")
    med = report(alternate(cases, 3, 20, args.rounds), "ms per call")
    print(f"  gather_tensors / index_select x18 = {med['gather_tensors'] / med['index_select x18']:.4f};  gather_tensors moves "
          f"{2 * P * 59 * 3 * 4 / med['gather_tensors'] / 1e6:.0f} GB/s (read + written)")
    return med["order + reorder"]


steps_ms = {}
for name in args.workloads:
    steps_ms[name] = render_part(name)
    torch.cuda.empty_cache()
costs = {}
for P in args.sizes:
    costs[P] = cost_part(P)
    torch.cuda.empty_cache()
print("steps after which one call (spatial_order + reorder_gaussians_ with Adam state, the nearest measured size) has paid for itself:")
for name, (P, med, ms) in steps_ms.items():
    if not costs:
        break
    near = min(costs, key=lambda n: abs(n - P))
    for before, after in (("a_generated", "b_reordered"), ("c_trained_like", "d_reordered")):
        gain = med[before] - med[after]
        spread = max(max(ms[n]) - min(ms[n]) for n in (before, after))
        pays = "never (the step did not get faster)" if gain <= 0 else f"{costs[near] / gain:.0f} steps" + ("" if gain > spread else " -- but the gain is within the rounds' spread")
        print(f"  {name} {before} -> {after}: call {costs[near]:.3f} ms at {near} rows, gain {gain:+.4f} ms per step: {pays}")
