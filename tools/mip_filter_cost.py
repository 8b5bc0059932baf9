#!/usr/bin/env python3
"""Cost of Mip-Splatting's 3D filter: the torch compositions against the fused calls (GPU box).
usage: tools/mip_filter_cost.py [--counts 1000000 6000000] [--cameras 200] [--steps 2] [--fused-steps 50] [--act-steps 200] [--rounds 5]

P Gaussians uniform in [-6, 6]^3, C cameras of 1600 x 1064 pixels (focal lengths near 1300) on a ring of radius 9 that look at the origin.  Cases:
  filter:      torch   that trainer's compute_3D_filter: a Python loop over the cameras, per camera xyz @ R + T, the depth and screen tests, and
                       distance[valid] = min(distance[valid], z[valid]) through boolean-mask indexing; then the fix-up and the scaling
               fused   compute_3d_filter(xyz, world_view_transforms, intrinsics): two kernels behind a 4-byte fill, no synchronisation
  activations: torch   get_scaling_with_3D_filter and get_opacity_with_3D_filter (the determinant form) forward, torch.autograd.grad backward
               fused   filtered_activations forward, torch.autograd.grad backward: one kernel each way
Every case is timed with events around its calls (`steps` of the torch filter, `fused-steps` of the fused one, `act-steps` of either
activation pair) after its warm-up calls; the cases alternate `rounds` times; per round and as medians.  For
the fused filter also its Gaussian-camera pairs per second; for the fused activations the algorithmic bytes (forward: 5 floats read and 4
written per row; backward: 9 read and 4 written) beside the stp_hbm_probe copy rate of the same run -- a rate above it is no share of HBM: every step
reads the same tensors again, and the 256 MiB Infinity Cache still holds part of them."""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stopthepop-rasterization_amd")); sys.path.insert(0, ROOT)
import numpy as np
import torch
import diff_gaussian_rasterization as dgr
from diff_gaussian_rasterization import _C, scenes

ap = argparse.ArgumentParser()
ap.add_argument("--counts", type=int, nargs="*", default=[1_000_000, 6_000_000])
ap.add_argument("--cameras", type=int, default=200)
ap.add_argument("--steps", type=int, default=2)
ap.add_argument("--fused-steps", type=int, default=50)
ap.add_argument("--act-steps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/mip_filter_cost.py measures on a GPU; there is none")
dev = torch.device("cuda:0")


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


def ring_cameras(C):
    views, intrinsics = [], []
    for c in range(C):
        a = 2.0 * math.pi * c / C
        views.append(scenes.look_at_view((9.0 * math.cos(a), 2.0 * math.sin(3.0 * a), 9.0 * math.sin(a)), (0.0, 0.0, 0.0)))
        intrinsics.append((1300.0 + 10.0 * (c % 7), 1290.0 + 10.0 * (c % 5), 1600.0, 1064.0))
    return torch.tensor(np.asarray(views, np.float32), device=dev), torch.tensor(np.asarray(intrinsics, np.float32), device=dev)


@torch.no_grad()
def filter_torch(xyz, cameras):
    """that trainer's compute_3D_filter; cameras: a list of (R (3, 3), T (3,), focal_x, focal_y, width, height) with Python numbers, as its Camera objects hold them"""
    distance = torch.ones(xyz.shape[0], device=xyz.device) * 100000.0
    valid_points = torch.zeros(xyz.shape[0], device=xyz.device, dtype=torch.bool)
    focal_length = 0.0
    for R, T, fx, fy, W, H in cameras:
        xyz_cam = xyz @ R + T[None, :]
        valid_depth = xyz_cam[:, 2] > 0.2
        x, y, z = xyz_cam[:, 0], xyz_cam[:, 1], xyz_cam[:, 2]
        z = torch.clamp(z, min=0.001)
        x = x / z * fx + W / 2.0
        y = y / z * fy + H / 2.0
        in_screen = torch.logical_and(torch.logical_and(x >= -0.15 * W, x <= W * 1.15), torch.logical_and(y >= -0.15 * H, y <= 1.15 * H))
        valid = torch.logical_and(valid_depth, in_screen)
        distance[valid] = torch.min(distance[valid], z[valid])
        valid_points = torch.logical_or(valid_points, valid)
        if focal_length < fx:
            focal_length = fx
    distance[~valid_points] = distance[valid_points].max()
    return (distance / focal_length * (0.2 ** 0.5))[..., None]


def activations_torch(scaling, opacity, filter_3d):
    scales = torch.exp(scaling)
    scales_square = torch.square(scales)
    det1 = scales_square.prod(dim=1)
    scales_after_square = scales_square + torch.square(filter_3d)
    det2 = scales_after_square.prod(dim=1)
    coef = torch.sqrt(det1 / det2)
    return torch.sqrt(scales_after_square), torch.sigmoid(opacity) * coef[..., None]


def report(name, ms):
    med = {n: statistics.median(x) for n, x in ms.items()}
    for n in ms:
        print(f"  {name} {n:6s} median {med[n]:.4f}  rounds " + " ".join(f"{x:.4f}" for x in ms[n]))
    faster = sum(f < t for f, t in zip(ms["fused"], ms["torch"]))
    print(f"  {name} fused / torch = {med['fused'] / med['torch']:.4f} (fused faster in {faster} of {len(ms['fused'])} rounds)")
    return med


def workload(P, rate):
    gen = torch.Generator(device=dev).manual_seed(1)
    rand = lambda *shape: torch.rand(*shape, device=dev, generator=gen)
    C = args.cameras
    print(f"P = {P}, C = {C}: {args.rounds} alternating rounds, ms per call (filter: {args.steps} torch and {args.fused_steps} fused calls a round; activations: {args.act_steps})")
    xyz = rand(P, 3) * 12.0 - 6.0
    views, intrinsics = ring_cameras(C)
    host = intrinsics.cpu().tolist()
    cameras = [(views[c, :3, :3].contiguous(), views[c, 3, :3].contiguous(), *host[c]) for c in range(C)]
    a, b = filter_torch(xyz, cameras), dgr.compute_3d_filter(xyz, views, intrinsics)
    differ = int((~torch.isclose(a, b, rtol=1e-4, atol=0)).sum())
    print(f"  filter: rows that differ by more than 1e-4 relative: {differ} of {P} (a decision at a threshold may fall either way in float32); "
          f"filter_3d in [{float(b.min()):.6f}, {float(b.max()):.6f}]")
    ms = {"torch": [], "fused": []}
    for _ in range(args.rounds):
        ms["torch"].append(timed(lambda: filter_torch(xyz, cameras), args.steps, warm=1))
        ms["fused"].append(timed(lambda: dgr.compute_3d_filter(xyz, views, intrinsics), args.fused_steps))
    med = report("filter", ms)
    print(f"  the fused filter decides {P * C / (med['fused'] * 1e-3) / 1e9:.1f} G Gaussian-camera pairs per second")

    scaling = (rand(P, 3) * 10.0 - 9.0).requires_grad_(True)
    opacity = (torch.randn(P, 1, device=dev, generator=gen) * 3.0).requires_grad_(True)
    filter_3d = b
    g_scales, g_opacities = torch.randn(P, 3, device=dev, generator=gen), torch.randn(P, 1, device=dev, generator=gen)

    def step(fn):
        outs = fn(scaling, opacity, filter_3d)
        return outs, torch.autograd.grad(outs, (scaling, opacity), (g_scales, g_opacities))

    (ta, tg), (fa, fg) = step(activations_torch), step(dgr.filtered_activations)
    rel = lambda x, y: float(((x - y).detach().abs().max() / y.detach().abs().max()))
    print(f"  activations: largest difference relative to the largest entry: scales {rel(fa[0], ta[0]):.1e} opacities {rel(fa[1], ta[1]):.1e} "
          f"grad_scaling {rel(fg[0], tg[0]):.1e} grad_opacity {rel(fg[1], tg[1]):.1e}; non-finite entries torch {sum(int((~torch.isfinite(t)).sum()) for t in tg)} "
          f"fused {sum(int((~torch.isfinite(t)).sum()) for t in fg)}")
    del ta, tg, fa, fg
    ms = {"torch": [], "fused": []}
    for _ in range(args.rounds):
        ms["torch"].append(timed(lambda: step(activations_torch), args.act_steps))
        ms["fused"].append(timed(lambda: step(dgr.filtered_activations), args.act_steps))
    med = report("activations forward + backward", ms)
    moved = 4 * 22 * P
    achieved = moved / (med["fused"] * 1e-3) / 1e12
    note = "" if achieved <= rate else " (above it: the steps re-read the same tensors, part of which the 256 MiB Infinity Cache still holds -- no share of HBM)"
    print(f"  the fused pair moves {moved / 1e6:.1f} MB -> {achieved:.2f} TB/s over forward + backward = {100.0 * achieved / rate:.1f} % of the copy rate{note}")


print(f"stp_hbm_probe copy, 1 GiB, this box, this run: {(rate := copy_rate()):.2f} TB/s")
for P in args.counts:
    workload(P, rate)
    torch.cuda.empty_cache()
