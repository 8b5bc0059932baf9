#!/usr/bin/env python3
"""Step time of the alpha / background requests through the public API, beside the plain step of the same run (GPU box).
usage: tools/background_cost.py [workload] [variant] [steps] [rounds]      (default: C2 full 30 3)

One forward + backward per step with dL_dout = the scene's, timed with events around `steps` steps after five warm-up steps; the five
cases alternate `rounds` times and the median per case is printed with its spread.  Cases:
  plain        bg = three floats
  alpha        settings._alpha = True, a loss term on alpha (its gradient joins the pixel prologue of the backward)
  bg_image     a (3, H, W) background
  bg_grad      three floats that require grad (the streaming kernel + the two-stage sum)
  bg_image_grad  a (3, H, W) background that requires grad (the streaming kernel writes 3 x H x W)"""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stopthepop-rasterization_amd")); sys.path.insert(0, ROOT)
import torch
import bench
import diff_gaussian_rasterization as dgr
from diff_gaussian_rasterization import scenes

workload = sys.argv[1] if len(sys.argv) > 1 else "C2"
variant = sys.argv[2] if len(sys.argv) > 2 else "full"
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 30
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
dev = torch.device("cuda:0")
sc = scenes.config(workload)
t = lambda a, rg=False: torch.tensor(a, device=dev).requires_grad_(rg)
gauss = dict(means3D=t(sc.means3D, True), opacities=t(sc.opacities, True), shs=t(sc.shs, True), scales=t(sc.scales, True), rotations=t(sc.rotations, True))
means2D = torch.zeros_like(gauss["means3D"], requires_grad=True)
w = t(sc.dL_dout)
wA = torch.rand(1, sc.H, sc.W, device=dev) - 0.5
B = torch.rand(3, sc.H, sc.W, device=dev)
cam = dict(viewmatrix=t(sc.viewmatrix), projmatrix=t(sc.projmatrix), inv_viewprojmatrix=t(sc.inv_viewprojmatrix), campos=t(sc.campos))


def case(name):
    es = bench.settings_for(variant, workload)
    es._alpha = name == "alpha"
    bg = B.clone() if name.startswith("bg_image") else t(sc.bg)
    bg.requires_grad_(name.endswith("grad"))
    rs = dgr.GaussianRasterizationSettings(image_height=sc.H, image_width=sc.W, tanfovx=sc.tanfovx, tanfovy=sc.tanfovy, bg=bg, scale_modifier=1.0,
                                           sh_degree=sc.sh_degree, prefiltered=False, settings=es, render_depth=False, debug=False, **cam)
    rast = dgr.GaussianRasterizer(rs)

    def step():
        out = rast(gauss["means3D"], means2D, gauss["opacities"], shs=gauss["shs"], scales=gauss["scales"], rotations=gauss["rotations"])
        torch.autograd.backward([out[0], out[2]] if es._alpha else [out[0]], [w, wA] if es._alpha else [w])
        for x in list(gauss.values()) + [means2D, bg]:
            x.grad = None
    return step


def timed(step):
    for _ in range(5):
        step()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


names = ("plain", "alpha", "bg_image", "bg_grad", "bg_image_grad")
cases = {n: case(n) for n in names}
ms = {n: [] for n in names}
for _ in range(rounds):
    for n in names:
        ms[n].append(timed(cases[n]))
base = statistics.median(ms["plain"])
print(f"{workload}-{variant}, {sc.W}x{sc.H}, {steps} steps x {rounds} rounds, ms per step (median [min .. max], against plain)")
for n in names:
    m = statistics.median(ms[n])
    print(f"  {n:14s} {m:.4f} [{min(ms[n]):.4f} .. {max(ms[n]):.4f}]  {m - base:+.4f} ms  {100.0 * (m / base - 1.0):+.2f} %")
