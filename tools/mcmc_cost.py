#!/usr/bin/env python3
"""Cost of 3DGS-MCMC's per-iteration position noise: upstream's torch composition against the fused mcmc_add_noise_ (GPU box).
usage: tools/mcmc_cost.py [workload ...] [--steps 100] [--rounds 5]      (default workloads: C2 C5 -- their Gaussian counts are what is used)

Both cases start from the model's RAW parameters, as the trainer has them after an optimizer step, and add the noise to xyz in place; the
normal noise tensor is drawn once outside the timed window (it is torch's in both).  Cases:
  torch_composition   upstream: opacity = sigmoid(_opacity), L = build_scaling_rotation(exp(_scaling), _rotation), Sigma = L @ L^T,
                      noise = randn * op_sigmoid(1 - opacity) * noise_lr * xyz_lr, xyz.add_(bmm(Sigma, noise[..., None]))
  fused               mcmc_add_noise_(xyz, _scaling, _rotation, _opacity, randn, noise_lr * xyz_lr, raw=True): one kernel
Every case is timed with events around `steps` calls after five warm-up calls; the cases alternate `rounds` times; per round and as medians.
For the fused case also its algorithmic bytes (68 per Gaussian: xyz read and written, scales, quaternion, opacity, noise) over its time, as
a fraction of the stp_hbm_probe copy rate of the same run.  (68 MB at C2's count fit the 256 MiB last-level cache: that rate is not an HBM
rate; C5's 408 MB do not fit.)  Last, one compute_relocation call at n = 50 000 with N uniform in 1..50."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stopthepop-rasterization_amd")); sys.path.insert(0, ROOT)
import torch
import diff_gaussian_rasterization as dgr
from diff_gaussian_rasterization import _C, scenes

ap = argparse.ArgumentParser()
ap.add_argument("workloads", nargs="*", default=["C2", "C5"])
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/mcmc_cost.py measures on a GPU; there is none")
dev = torch.device("cuda:0")
NOISE_SCALE = 5e5 * 1.6e-4   # upstream's noise_lr * position_lr_init


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


def build_rotation(r):   # upstream utils/general_utils.py
    q = r / torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])[:, None]
    R = torch.zeros((q.size(0), 3, 3), device=r.device)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def build_scaling_rotation(s, r):
    L = torch.zeros((s.shape[0], 3, 3), dtype=torch.float, device=s.device)
    R = build_rotation(r)
    L[:, 0, 0] = s[:, 0]; L[:, 1, 1] = s[:, 1]; L[:, 2, 2] = s[:, 2]
    return R @ L


def workload(name, rate):
    P = scenes._CONFIGS[name]["P"]
    gen = torch.Generator(device=dev).manual_seed(1)
    rand = lambda *shape: torch.rand(*shape, device=dev, generator=gen)
    xyz = rand(P, 3) * 10 - 5
    scaling = rand(P, 3) * 7 - 6                      # raw: scales exp(U[-6, 1])
    rotation = torch.randn(P, 4, device=dev, generator=gen)
    opacity = torch.logit(rand(P, 1) * 0.98 + 0.01)   # raw
    noise = torch.randn(P, 3, device=dev, generator=gen)
    xyz_torch, xyz_fused = xyz.clone(), xyz.clone()

    @torch.no_grad()
    def torch_composition():
        L = build_scaling_rotation(torch.exp(scaling), rotation)
        sigma = L @ L.transpose(1, 2)
        gate = 1 / (1 + torch.exp(-100.0 * ((1 - torch.sigmoid(opacity)) - 0.995)))
        w = noise * gate * NOISE_SCALE
        xyz_torch.add_(torch.bmm(sigma, w.unsqueeze(-1)).squeeze(-1))

    def fused():
        dgr.mcmc_add_noise_(xyz_fused, scaling, rotation, opacity, noise, NOISE_SCALE, raw=True)

    # both add the same displacement: one call each from equal positions
    torch_composition(); fused()
    diff = float((xyz_torch - xyz_fused).abs().max())
    cases = {"torch_composition": torch_composition, "fused": fused}
    ms = {n: [] for n in cases}
    for _ in range(args.rounds):
        for n, step in cases.items():
            ms[n].append(timed(step, args.steps))
    med = {n: statistics.median(v) for n, v in ms.items()}
    print(f"{name}: P = {P}, {args.rounds} alternating rounds of {args.steps} calls, ms per call; largest difference of one call's positions {diff:.3g}")
    for n in cases:
        print(f"  {n:18s} median {med[n]:.4f}  rounds " + " ".join(f"{x:.4f}" for x in ms[n]))
    faster = sum(f < t for f, t in zip(ms["fused"], ms["torch_composition"]))
    moved = 68 * P
    achieved = moved / (med["fused"] * 1e-3) / 1e12
    print(f"  fused / torch_composition = {med['fused'] / med['torch_composition']:.4f} (fused faster in {faster} of {args.rounds} rounds); "
          f"fused moves {moved / 1e6:.1f} MB -> {achieved:.2f} TB/s = {100.0 * achieved / rate:.1f} % of the copy rate")


def relocation():
    n = 50_000
    gen = torch.Generator(device=dev).manual_seed(2)
    o = torch.rand(n, device=dev, generator=gen) * 0.994 + 0.005
    s = torch.exp(torch.rand(n, 3, device=dev, generator=gen) * 7 - 6)
    N = torch.randint(1, 51, (n,), device=dev, generator=gen)
    ms = [timed(lambda: dgr.compute_relocation(o, s, N), args.steps) for _ in range(args.rounds)]
    print(f"compute_relocation, n = {n}, N uniform in 1..50: median {statistics.median(ms) * 1e3:.1f} us per call (outputs allocated by the call)  rounds "
          + " ".join(f"{x * 1e3:.1f}" for x in ms))


print(f"stp_hbm_probe copy, 1 GiB, this box, this run: {(rate := copy_rate()):.2f} TB/s")
for name in args.workloads:
    workload(name, rate)
    torch.cuda.empty_cache()
relocation()
