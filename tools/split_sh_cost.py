#!/usr/bin/env python3
"""Step time and peak memory of split SH inputs (dc=) against torch.cat in front of the concatenated path (GPU box).
usage: tools/split_sh_cost.py [workload ...] [--steps 30] [--rounds 5] [--variant full]      (default workloads: C2 C5)

The model keeps its SH coefficients as a trainer does, in two leaf parameters: f_dc (P, 1, 3) and f_rest (P, 15, 3).  One forward + backward
per step with dL_dout = the scene's, all gradients cleared behind it.  Cases:
  cat     shs = torch.cat((f_dc, f_rest), dim=1): the (P, 16, 3) copy going in, a full-size dL_dsh and CatBackward's two slice copies
          coming out -- what a trainer does without the input
  split   dc = f_dc, shs = f_rest: no copy in either direction, the two .grad tensors are the library's outputs
Each case is timed with events around `steps` steps after five warm-up steps; the cases alternate `rounds` times; ms per step per round and
as medians.  Peak memory: torch.cuda.max_memory_allocated over `steps` steps of each case on its own, after a reset, with the gradients
of the other case gone.  Last, the per-stage split of both (the library's stage timer: Preprocess .. BwdPreprocess, mean ms; the colour
kernel runs on a side stream beside the Sort stage) and the byte estimate the difference is held against: 768 B per Gaussian per step."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stopthepop-rasterization_amd")); sys.path.insert(0, ROOT)
import torch
import bench
import diff_gaussian_rasterization as dgr
from diff_gaussian_rasterization import _C, scenes

ap = argparse.ArgumentParser()
ap.add_argument("workloads", nargs="*", default=["C2", "C5"])
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--variant", default="full")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/split_sh_cost.py measures on a GPU; there is none")
dev = torch.device("cuda:0")
NAMES = ("cat", "split")


def timed(step, steps):
    for _ in range(5):
        step()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def workload(name):
    sc = scenes.config(name)
    t = lambda a, rg=False: torch.tensor(a, device=dev).requires_grad_(rg)
    shs = t(sc.shs)
    leaves = dict(means3D=t(sc.means3D, True), opacities=t(sc.opacities, True), scales=t(sc.scales, True), rotations=t(sc.rotations, True),
                  f_dc=shs[:, :1].contiguous().requires_grad_(True), f_rest=shs[:, 1:].contiguous().requires_grad_(True))
    del shs
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    w = t(sc.dL_dout)
    rs = dgr.GaussianRasterizationSettings(
        image_height=sc.H, image_width=sc.W, tanfovx=sc.tanfovx, tanfovy=sc.tanfovy, bg=t(sc.bg), scale_modifier=1.0, sh_degree=sc.sh_degree,
        prefiltered=False, settings=bench.settings_for(args.variant, name), render_depth=False, debug=False, viewmatrix=t(sc.viewmatrix),
        projmatrix=t(sc.projmatrix), inv_viewprojmatrix=t(sc.inv_viewprojmatrix), campos=t(sc.campos))
    rast = dgr.GaussianRasterizer(rs)
    P = len(sc.means3D)

    def case(which):
        def step(keep=False):
            kw = dict(scales=leaves["scales"], rotations=leaves["rotations"])
            if which == "cat":
                image = rast(leaves["means3D"], means2D, leaves["opacities"], shs=torch.cat((leaves["f_dc"], leaves["f_rest"]), dim=1), **kw)[0]
            else:
                image = rast(leaves["means3D"], means2D, leaves["opacities"], shs=leaves["f_rest"], dc=leaves["f_dc"], **kw)[0]
            (image * w).sum().backward()
            grads = {n: x.grad for n, x in leaves.items()} if keep else None
            for x in list(leaves.values()) + [means2D]:
                x.grad = None
            return grads
        return step

    cases = {n: case(n) for n in NAMES}
    a, b = cases["cat"](keep=True), cases["split"](keep=True)
    worst = max(float((a[n] - b[n]).abs().max()) / max(float(a[n].abs().max()), 1e-30) for n in a)
    print(f"{name}-{args.variant}: P = {P}, {sc.W}x{sc.H}, {args.steps} steps x {args.rounds} alternating rounds, ms per step")
    print(f"  both give the same gradients: largest difference {worst:.2e} of a tensor's largest entry (float atomics in the render half)")
    del a, b
    ms = {n: [] for n in NAMES}
    for _ in range(args.rounds):
        for n in NAMES:
            ms[n].append(timed(cases[n], args.steps))
    med = {n: statistics.median(ms[n]) for n in NAMES}
    for n in NAMES:
        print(f"  {n:6s} median {med[n]:.4f}  rounds " + " ".join(f"{x:.4f}" for x in ms[n]))
    faster = sum(s < c for s, c in zip(ms["split"], ms["cat"]))
    diff = med["cat"] - med["split"]
    print(f"  split / cat = {med['split'] / med['cat']:.4f}, {diff * 1e3:+.1f} us per step saved (split faster in {faster} of {args.rounds} rounds)")
    est = 768 * P
    print(f"  byte estimate: {est / 1e9:.3f} GB per step -> {est / 5e12 * 1e3:.3f} .. {est / 4e12 * 1e3:.3f} ms at 5 .. 4 TB/s"
          + (f"; the measured difference corresponds to {est / (diff * 1e-3) / 1e12:.2f} TB/s" if diff > 0 else ""))
    peak = {}
    for n in NAMES:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        for _ in range(args.steps):
            cases[n]()
        torch.cuda.synchronize()
        peak[n] = (torch.cuda.max_memory_allocated(), base)
        print(f"  {n:6s} peak memory {peak[n][0] / 2**20:.1f} MiB ({(peak[n][0] - base) / 2**20:.1f} MiB above the model and the frame)")
    print(f"  split - cat = {(peak['split'][0] - peak['cat'][0]) / 2**20:+.1f} MiB peak (estimate: -{(192 + 192) * P / 2**20:.0f} MiB, the concatenated tensor and the full-size dL_dsh)")
    L = _C._load()
    stages = ("Preprocess", "Duplicate", "Sort", "Render", "BwdRender", "BwdPreprocess")
    for n in NAMES:
        L.stp_timing_enable(1)
        for _ in range(args.steps):
            cases[n]()
        torch.cuda.synchronize()
        buf = (ctypes.c_float * 6)()
        L.stp_timing_read(buf)
        L.stp_timing_enable(0)
        print(f"  {n:6s} stages " + "  ".join(f"{s} {v:.4f}" for s, v in zip(stages, buf)))


for name in args.workloads:
    workload(name)
    torch.cuda.empty_cache()
