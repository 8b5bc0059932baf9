#!/usr/bin/env python3
"""Step time and peak memory of raw parameter inputs (raw=True) against torch.exp / sigmoid / F.normalize in front of the plain call (GPU box).
usage: tools/raw_params_cost.py [workload ...] [--steps 30] [--rounds 5] [--variant full]      (default workloads: C2 C5)

The model keeps a Gaussian as a trainer does, in three raw leaf parameters: _scaling (P, 3) = log of the scale, _rotation (P, 4) an
unnormalised quaternion, _opacity (P, 1) a logit.  One forward + backward per step with dL_dout = the scene's, all gradients cleared behind
it.  Cases:
  torch   scales = torch.exp(_scaling), rotations = F.normalize(_rotation), opacities = torch.sigmoid(_opacity) in front of the plain call:
          three activated copies going in, three full-size intermediate gradients and the activations' backward nodes coming out -- what a
          trainer does without the input
  raw     the same three leaves passed straight in, to GaussianRasterizer(rs, raw=True): the kernels activate at their loads and apply the chain rule at their stores
Each case is timed with events around `steps` steps after five warm-up steps; the cases alternate `rounds` times; ms per step per round and
as medians.  Peak memory: torch.cuda.max_memory_allocated over `steps` steps of each case on its own, after a reset, with the gradients
of the other case gone.  Last, the per-stage split of both (the library's stage timer: Preprocess .. BwdPreprocess, mean ms) and the byte and
launch count the difference is held against: per Gaussian and step the eager activations read 32 B and write 32 B going in, and read and
write about 3 x 32 B more coming back (each backward node reads the incoming gradient and a saved tensor and writes a gradient; normalize is
norm, clamp, expand and div with as many backward nodes): 200 .. 300 B, in roughly a dozen launches."""
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
    raise SystemExit("tools/raw_params_cost.py measures on a GPU; there is none")
dev = torch.device("cuda:0")
NAMES = ("torch", "raw")


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
    op = t(sc.opacities).clamp(1e-4, 1 - 1e-4)
    leaves = dict(means3D=t(sc.means3D, True), shs=t(sc.shs, True), _scaling=torch.log(t(sc.scales)).requires_grad_(True),
                  _rotation=(t(sc.rotations) * 1.7).requires_grad_(True), _opacity=torch.log(op / (1 - op)).requires_grad_(True))
    del op
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    w = t(sc.dL_dout)
    rs = dgr.GaussianRasterizationSettings(
        image_height=sc.H, image_width=sc.W, tanfovx=sc.tanfovx, tanfovy=sc.tanfovy, bg=t(sc.bg), scale_modifier=1.0, sh_degree=sc.sh_degree,
        prefiltered=False, settings=bench.settings_for(args.variant, name), render_depth=False, debug=False, viewmatrix=t(sc.viewmatrix),
        projmatrix=t(sc.projmatrix), inv_viewprojmatrix=t(sc.inv_viewprojmatrix), campos=t(sc.campos))
    rast, rast_raw = dgr.GaussianRasterizer(rs), dgr.GaussianRasterizer(rs, raw=True)
    P = len(sc.means3D)

    def case(which):
        def step(keep=False):
            if which == "torch":
                image = rast(leaves["means3D"], means2D, torch.sigmoid(leaves["_opacity"]), shs=leaves["shs"], scales=torch.exp(leaves["_scaling"]),
                             rotations=torch.nn.functional.normalize(leaves["_rotation"]))[0]
            else:
                image = rast_raw(leaves["means3D"], means2D, leaves["_opacity"], shs=leaves["shs"], scales=leaves["_scaling"],
                                 rotations=leaves["_rotation"])[0]
            (image * w).sum().backward()
            grads = {n: x.grad for n, x in leaves.items()} if keep else None
            for x in list(leaves.values()) + [means2D]:
                x.grad = None
            return grads
        return step

    def copies_step():
        """the plain call on activate_params' copies -- the raw path's own values -- with the chain rule applied by hand: the raw path's equal"""
        s, q, o = (x.requires_grad_(True) for x in dgr.activate_params(leaves["_scaling"], leaves["_rotation"], leaves["_opacity"]))
        image = rast(leaves["means3D"], means2D, o, shs=leaves["shs"], scales=s, rotations=q)[0]
        (image * w).sum().backward()
        n = leaves["_rotation"].detach().norm(dim=1, keepdim=True).clamp(min=1e-12)
        qd = q.detach()
        grads = {"means3D": leaves["means3D"].grad, "shs": leaves["shs"].grad, "_scaling": s.grad * s.detach(),
                 "_rotation": (q.grad - qd * (qd * q.grad).sum(1, keepdim=True)) / n, "_opacity": o.grad * o.detach() * (1 - o.detach())}
        for x in list(leaves.values()) + [means2D]:
            x.grad = None
        return grads

    cases = {n: case(n) for n in NAMES}
    a, b, c = cases["torch"](keep=True), cases["raw"](keep=True), copies_step()
    rel = lambda x, y: float((x - y).abs().max()) / max(float(x.abs().max()), 1e-30)
    print(f"{name}-{args.variant}: P = {P}, {sc.W}x{sc.H}, {args.steps} steps x {args.rounds} alternating rounds, ms per step")
    print("  raw against the plain call on activate_params' copies (the same values: float atomics in the render half only), largest difference of a "
          "tensor's largest entry: " + "  ".join(f"{n} {rel(c[n], b[n]):.1e}" for n in c))
    print("  raw against torch's activations (inputs an ulp apart: a Gaussian at a culling threshold can change tiles), the same: "
          + "  ".join(f"{n} {rel(a[n], b[n]):.1e}" for n in a))
    del a, b, c
    ms = {n: [] for n in NAMES}
    for _ in range(args.rounds):
        for n in NAMES:
            ms[n].append(timed(cases[n], args.steps))
    med = {n: statistics.median(ms[n]) for n in NAMES}
    for n in NAMES:
        print(f"  {n:6s} median {med[n]:.4f}  rounds " + " ".join(f"{x:.4f}" for x in ms[n]))
    faster = sum(r < c for r, c in zip(ms["raw"], ms["torch"]))
    diff = med["torch"] - med["raw"]
    print(f"  raw / torch = {med['raw'] / med['torch']:.4f}, {diff * 1e3:+.1f} us per step saved (raw faster in {faster} of {args.rounds} rounds)")
    lo, hi = 200 * P, 300 * P
    print(f"  byte estimate: {lo / 1e9:.3f} .. {hi / 1e9:.3f} GB per step (200 .. 300 B per Gaussian) -> {lo / 5e12 * 1e3:.3f} .. {hi / 4e12 * 1e3:.3f} ms at 5 .. 4 TB/s"
          + (f"; the measured difference corresponds to {hi / (diff * 1e-3) / 1e12:.2f} TB/s at 300 B" if diff > 0 else "")
          + "; launch estimate: about a dozen eager launches per step against none")
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
    print(f"  raw - torch = {(peak['raw'][0] - peak['torch'][0]) / 2**20:+.1f} MiB peak (estimate: up to -{(32 + 32) * P / 2**20:.0f} MiB, the three activated copies "
          f"and the three intermediate gradients, where they are alive at the peak)")
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
