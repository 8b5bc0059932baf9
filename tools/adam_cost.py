#!/usr/bin/env python3
"""Step time of the optimizer beside the rasterizer's: torch.optim.Adam against SparseGaussianAdam on a trainer's six tensors (GPU box).
usage: tools/adam_cost.py [workload ...] [--steps 100] [--rounds 5] [--variant full]      (default workloads: C2 C5)

The six tensors have the trainer's shapes for the workload's P Gaussians -- xyz (P,3), f_dc (P,1,3), f_rest (P,15,3), opacity (P,1),
scaling (P,3), rotation (P,4): 59 floats per Gaussian -- and random gradients.  Every case is timed with events around `steps` steps after
five warm-up steps; the cases alternate `rounds` times and the median per case is printed with its spread.  Cases:
  adam_foreach     torch.optim.Adam as examples/train_render.py uses it (foreach on a GPU)
  adam_fused       torch.optim.Adam(fused=True)
  sparse_all       SparseGaussianAdam, everything visible (a bool mask)
  sparse_frame     SparseGaussianAdam with the visibility of the workload's own frame: the int32 radii of one forward, read as they are
  raster_step      the plain forward + backward of the same workload, for proportion
For the two sparse cases also the bytes the step has to move (28 bytes per element of a visible Gaussian: p, g, m, v read, p, m, v written;
plus the visibility entries, once per tensor) and the rate that makes, beside the copy rate of stp_hbm_probe in the same run."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stopthepop-rasterization_amd")); sys.path.insert(0, ROOT)
import torch
import bench
import diff_gaussian_rasterization as dgr
from diff_gaussian_rasterization import _C, scenes

SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 2.5e-2, "scaling": 5e-3, "rotation": 1e-3}   # the 3DGS trainer's
FLOATS = sum(int(torch.Size(s).numel()) for s in SHAPES.values())   # 59

ap = argparse.ArgumentParser()
ap.add_argument("workloads", nargs="*", default=["C2", "C5"])
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--variant", default="full")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/adam_cost.py measures on a GPU; there is none")
dev = torch.device("cuda:0")


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


def copy_rate():
    """TB/s of the library's float4 copy kernel on 1 GiB (read + write bytes), best of 10 over a few grids"""
    x, y = torch.ones(1 << 28, device=dev), torch.empty(1 << 28, device=dev)
    best = float("inf")
    for blocks in (2048, 4096, 8192, 16384):
        for nt in (False, True):
            best = min(best, min(timed(lambda: _C.hbm_probe("copy", y, x, blocks=blocks, nontemporal=nt), 10) for _ in range(2)))
    return 2 * x.numel() * 4 / (best * 1e-3) / 1e12


def workload(name):
    sc = scenes.config(name)
    P = int(sc.means3D.shape[0])
    t = lambda a, rg=False: torch.tensor(a, device=dev).requires_grad_(rg)
    gauss = dict(means3D=t(sc.means3D, True), opacities=t(sc.opacities, True), shs=t(sc.shs, True), scales=t(sc.scales, True), rotations=t(sc.rotations, True))
    means2D = torch.zeros_like(gauss["means3D"], requires_grad=True)
    w = t(sc.dL_dout)
    rs = dgr.GaussianRasterizationSettings(image_height=sc.H, image_width=sc.W, tanfovx=sc.tanfovx, tanfovy=sc.tanfovy, bg=t(sc.bg), scale_modifier=1.0,
                                           sh_degree=sc.sh_degree, prefiltered=False, settings=bench.settings_for(args.variant, name), render_depth=False,
                                           debug=False, viewmatrix=t(sc.viewmatrix), projmatrix=t(sc.projmatrix),
                                           inv_viewprojmatrix=t(sc.inv_viewprojmatrix), campos=t(sc.campos))
    rast = dgr.GaussianRasterizer(rs)

    def raster_step():
        out = rast(gauss["means3D"], means2D, gauss["opacities"], shs=gauss["shs"], scales=gauss["scales"], rotations=gauss["rotations"])
        out[0].backward(w)
        for x in list(gauss.values()) + [means2D]:
            x.grad = None
        return out[1]

    radii = raster_step().clone()
    n_visible = int((radii > 0).sum())
    everything = torch.ones(P, dtype=torch.bool, device=dev)

    gen = torch.Generator(device=dev).manual_seed(1)
    params = {n: torch.nn.Parameter(torch.randn((P,) + s, device=dev, generator=gen)) for n, s in SHAPES.items()}
    for p in params.values():   # (one set of parameters and gradients for all optimizers: each has its own moments)
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
    groups = lambda: [{"params": [params[n]], "lr": LRS[n], "name": n} for n in SHAPES]
    foreach = torch.optim.Adam(groups(), lr=0.0, eps=1e-15)
    fused = torch.optim.Adam(groups(), lr=0.0, eps=1e-15, fused=True)
    sparse_all, sparse_frame = dgr.SparseGaussianAdam(groups(), lr=0.0, eps=1e-15), dgr.SparseGaussianAdam(groups(), lr=0.0, eps=1e-15)
    cases = {"adam_foreach": (foreach.step, args.steps), "adam_fused": (fused.step, args.steps),
             "sparse_all": (lambda: sparse_all.step(everything, P), args.steps), "sparse_frame": (lambda: sparse_frame.step(radii, P), args.steps),
             "raster_step": (raster_step, max(10, args.steps // 4))}
    ms = {n: [] for n in cases}
    for _ in range(args.rounds):
        for n, (step, steps) in cases.items():
            ms[n].append(timed(step, steps))
    assert sparse_all.last_launches == 1 and sparse_frame.last_launches == 1
    moved = {"sparse_all": 28 * FLOATS * P + len(SHAPES) * P, "sparse_frame": 28 * FLOATS * n_visible + len(SHAPES) * 4 * P}
    med = {n: statistics.median(v) for n, v in ms.items()}
    print(f"{name}-{args.variant}: P = {P}, {sc.W}x{sc.H}, {n_visible} visible ({100.0 * n_visible / P:.1f} %), {args.rounds} alternating rounds, "
          f"ms per step (median [min .. max])")
    for n in cases:
        line = f"  {n:13s} {med[n]:.4f} [{min(ms[n]):.4f} .. {max(ms[n]):.4f}]  {cases[n][1]} steps per round  {100.0 * med[n] / med['raster_step']:.1f} % of raster_step"
        if n in moved:
            line += f"  {moved[n] / 1e9:.3f} GB -> {moved[n] / (med[n] * 1e-3) / 1e12:.2f} TB/s"
        print(line)
    print(f"  sparse_frame / adam_fused = {med['sparse_frame'] / med['adam_fused']:.3f} (visible share {n_visible / P:.3f}); "
          f"sparse_all / adam_fused = {med['sparse_all'] / med['adam_fused']:.3f}")
    return moved["sparse_all"] / (med["sparse_all"] * 1e-3) / 1e12


print(f"stp_hbm_probe copy, 1 GiB, this box, this run: {(rate := copy_rate()):.2f} TB/s")
for name in args.workloads:
    achieved = workload(name)
    print(f"  sparse_all reaches {100.0 * achieved / rate:.1f} % of the copy rate")
    torch.cuda.empty_cache()
