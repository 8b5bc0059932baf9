#!/usr/bin/env python3
"""Step time of the dense optimizer a 3DGS-MCMC trainer runs every iteration: GaussianAdam (one fused launch, the two regularisers folded in)
against torch.optim.Adam plus the autograd regulariser chain it replaces, on a trainer's six tensors (GPU box).
usage: tools/dense_adam_cost.py [workload ...] [--steps 50] [--rounds 5]      (default workloads: C2 C5 -- 1M and 6M Gaussians)

The six tensors have the trainer's shapes for the workload's P Gaussians -- xyz (P,3), f_dc (P,1,3), f_rest (P,15,3), opacity (P,1),
scaling (P,3), rotation (P,4): 59 floats per Gaussian -- and random gradients.  Every case is timed with events around `steps` steps after
five warm-up steps; the cases alternate `rounds` times IN ONE PROCESS and the median per case is printed with its spread.  Cases:
  gaussian_adam        GaussianAdam.step() with reg = ("sigmoid", 0.01) on opacity and ("exp", 0.01) on scaling
  gaussian_adam_plain  GaussianAdam.step() without regularisers
  adam_foreach         torch.optim.Adam as the trainers construct it (foreach on a GPU), no regularisers
  adam_foreach+reg     ... after (0.01 * sigmoid(opacity).abs().mean() + 0.01 * exp(scaling).abs().mean()).backward(): the chain the fused step replaces
  adam_fused           torch.optim.Adam(fused=True), if it constructs here
  adam_fused+reg       ... after the same chain
For the two GaussianAdam cases also the bytes the step has to move (28 bytes per element: p, g, m, v read, p, m, v written) and the rate that
makes, beside the copy rate of stp_hbm_probe in the same run; and the kernel's register / LDS / scratch line from the library's code object."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stopthepop-rasterization_amd")); sys.path.insert(0, ROOT)
import torch
import diff_gaussian_rasterization as dgr
from diff_gaussian_rasterization import _C, scenes

SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 2.5e-2, "scaling": 5e-3, "rotation": 1e-3}   # the 3DGS trainer's
FLOATS = sum(int(torch.Size(s).numel()) for s in SHAPES.values())   # 59
OPACITY_REG = SCALE_REG = 0.01                                       # 3DGS-MCMC's defaults

ap = argparse.ArgumentParser()
ap.add_argument("workloads", nargs="*", default=["C2", "C5"])
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/dense_adam_cost.py measures on a GPU; there is none")
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
    P = int(scenes.config(name).means3D.shape[0])
    gen = torch.Generator(device=dev).manual_seed(1)

    def tensors():   # every optimizer steps parameters of its own: the regulariser chain reads them
        params = {n: torch.nn.Parameter(torch.randn((P,) + s, device=dev, generator=gen)) for n, s in SHAPES.items()}
        for p in params.values():
            p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
        return params, [{"params": [params[n]], "lr": LRS[n], "name": n} for n in SHAPES]

    def with_chain(opt, params):
        def step():   # (the gradients accumulate from step to step: the time does not depend on their values)
            (OPACITY_REG * torch.sigmoid(params["opacity"]).abs().mean() + SCALE_REG * torch.exp(params["scaling"]).abs().mean()).backward()
            opt.step()
        return step

    cases = {}
    params, groups = tensors()
    ours = dgr.GaussianAdam(groups, lr=0.0, eps=1e-15)
    ours.set_regularizer("opacity", "sigmoid", OPACITY_REG)
    ours.set_regularizer("scaling", "exp", SCALE_REG)
    cases["gaussian_adam"] = ours.step
    params, groups = tensors()
    plain = dgr.GaussianAdam(groups, lr=0.0, eps=1e-15)
    cases["gaussian_adam_plain"] = plain.step
    params, groups = tensors()
    cases["adam_foreach"] = torch.optim.Adam(groups, lr=0.0, eps=1e-15).step
    params, groups = tensors()
    cases["adam_foreach+reg"] = with_chain(torch.optim.Adam(groups, lr=0.0, eps=1e-15), params)
    try:
        params, groups = tensors()
        cases["adam_fused"] = torch.optim.Adam(groups, lr=0.0, eps=1e-15, fused=True).step
        params, groups = tensors()
        cases["adam_fused+reg"] = with_chain(torch.optim.Adam(groups, lr=0.0, eps=1e-15, fused=True), params)
    except (RuntimeError, ValueError) as ex:
        print(f"  torch.optim.Adam(fused=True) does not construct here: {ex}")
    ms = {n: [] for n in cases}
    for _ in range(args.rounds):
        for n, step in cases.items():
            ms[n].append(timed(step, args.steps))
    assert ours.last_launches == 1 and plain.last_launches == 1
    moved = 28 * FLOATS * P
    med = {n: statistics.median(v) for n, v in ms.items()}
    print(f"{name}: P = {P}, {FLOATS} floats per Gaussian, {args.rounds} alternating rounds of {args.steps} steps, ms per step (median [min .. max])")
    for n in cases:
        line = f"  {n:20s} {med[n]:.4f} [{min(ms[n]):.4f} .. {max(ms[n]):.4f}]  {med[n] / med['gaussian_adam']:.2f} x gaussian_adam"
        if n.startswith("gaussian_adam"):
            line += f"  {moved / 1e9:.3f} GB -> {moved / (med[n] * 1e-3) / 1e12:.2f} TB/s"
        print(line)
    return moved / (med["gaussian_adam"] * 1e-3) / 1e12


res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "dense_adam_kernel", _C.library_path()], capture_output=True, text=True)
print(res.stdout.strip() or f"(no resource line: {res.stderr.strip()[:200]})")
print(f"stp_hbm_probe copy, 1 GiB, this box, this run: {(rate := copy_rate()):.2f} TB/s")
for name in args.workloads:
    achieved = workload(name)
    print(f"  gaussian_adam reaches {100.0 * achieved / rate:.1f} % of the copy rate")
    torch.cuda.empty_cache()
