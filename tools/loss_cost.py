#!/usr/bin/env python3
"""Step time of the trainer's loss beside the rasterizer's: upstream's torch composition against photometric_loss (GPU box).
usage: tools/loss_cost.py [workload ...] [--steps 50] [--rounds 5] [--variant full] [--no-raster]      (default workloads: C2 C5)

The loss is (1 - 0.2) * L1 + 0.2 * (1 - SSIM) on the workload's frame (C2: 3 x 1080 x 1920, C5: 3 x 1063 x 1600): the image is the
workload's own render (with --no-raster: a smooth image plus 2 % noise), the target the same disturbed by 5 % noise.  Every case is
forward + backward down to dL/dimage, timed with events around `steps` steps after five warm-up steps; the cases alternate `rounds`
times and the median per case is printed with its spread.  Cases:
  torch_loss       upstream's composition written out: l1_loss + ssim() with five depthwise 11 x 11 conv2d calls and the elementwise chain
  fused_loss       photometric_loss: two fused kernels + the sum forward, one backward
  fused_eval       photometric_loss under no_grad (no derivative maps stored): the forward alone
  raster_step      the plain forward + backward of the same workload, for proportion
and whether fused_loss was faster than torch_loss in EVERY round, beside the copy rate of stp_hbm_probe in the same run and the bytes
the fused pair has to move at least (forward: x, y read, three maps written; backward: x, y and the maps read, dL/dx written: 44 bytes
per element).
With --training two more cases, the full loss of upstream's step (per-image exposure, clamp, alpha mask, depth term; forward + backward down
to dL/dimage, dL/dexposure and dL/dinvdepth), alternating like the others:
  around_fused     today's way: the torch lines (permute / matmul, clamp, mask, the depth L1) around photometric_loss
  training_loss    training_loss: the same in the fused kernels
With --ab-lib PATH two more pairs: photometric_loss alone, and training_loss with the extras above, each on the default library and on the
library at PATH, alternating (has either pair of kernels moved?)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stopthepop-rasterization_amd")); sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
import bench
import diff_gaussian_rasterization as dgr
from diff_gaussian_rasterization import _C, scenes

FRAMES = {"C2": (1080, 1920), "C5": (1063, 1600)}

ap = argparse.ArgumentParser()
ap.add_argument("workloads", nargs="*", default=["C2", "C5"])
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--variant", default="full")
ap.add_argument("--training", action="store_true", help="also time the extended loss: torch lines around photometric_loss against training_loss")
ap.add_argument("--ab-lib", default=None, help="also time photometric_loss and training_loss on the default library and on this one, alternating")
ap.add_argument("--no-raster", action="store_true", help="do not build the workload's scene: synthetic images, no raster_step")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/loss_cost.py measures on a GPU; there is none")
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


_k = torch.arange(11, dtype=torch.float64)
_w = torch.exp(-(_k - 5.0) ** 2 / 4.5)
_w = (_w / _w.sum()).float()
WINDOW = (_w[:, None] * _w[None, :]).expand(3, 1, 11, 11).contiguous().to(dev)


def torch_loss(image, target, lambda_dssim=0.2):
    """upstream's l1_loss(image, target) and ssim(image, target) (window_size = 11, size_average = True), written out"""
    l1 = torch.abs(image - target).mean()
    blur = lambda v: F.conv2d(v, WINDOW, padding=5, groups=3)
    mu1, mu2 = blur(image), blur(target)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq, sigma2_sq, sigma12 = blur(image * image) - mu1_sq, blur(target * target) - mu2_sq, blur(image * target) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - ssim_map.mean())


def workload(name):
    H, W = FRAMES[name]
    gen = torch.Generator(device=dev).manual_seed(1)
    raster_step = None
    if args.no_raster:
        yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
        base = torch.stack([0.5 + 0.4 * torch.sin(0.011 * xx + 0.007 * yy + c) * torch.cos(0.005 * yy - 0.3 * c) for c in range(3)])
        image = (base + 0.02 * torch.randn(base.shape, device=dev, generator=gen)).clamp(0.0, 1.0)
    else:
        sc = scenes.config(name)
        assert (sc.H, sc.W) == (H, W)
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
            return out[0]

        image = raster_step().detach().clamp(0.0, 1.0).clone()
    target = (image + 0.05 * torch.randn(image.shape, device=dev, generator=gen)).clamp(0.0, 1.0)
    image.requires_grad_(True)

    def step_of(loss_fn):
        def step():
            loss_fn(image[None], target[None]).backward()   # (upstream's ssim() takes a batch; the fused loss takes either)
            image.grad = None
        return step

    def fused_eval():
        with torch.no_grad():
            dgr.photometric_loss(image, target)

    # the two agree before they are timed
    a, b = torch_loss(image[None], target[None]), dgr.photometric_loss(image, target)
    ga, gb = torch.autograd.grad(a, image)[0], torch.autograd.grad(b, image)[0]
    agree = f"loss {float(a.detach()):.7f} / {float(b.detach()):.7f}, largest gradient difference {float((ga - gb).abs().max()):.3g} of {float(ga.abs().max()):.3g}"
    cases = {"torch_loss": (step_of(torch_loss), args.steps), "fused_loss": (step_of(dgr.photometric_loss), args.steps), "fused_eval": (fused_eval, args.steps)}
    if raster_step is not None:
        cases["raster_step"] = (raster_step, max(10, args.steps // 4))
    ms = {n: [] for n in cases}
    for _ in range(args.rounds):
        for n, (step, steps) in cases.items():
            ms[n].append(timed(step, steps))
    med = {n: statistics.median(v) for n, v in ms.items()}
    n_el = image.numel()
    moved = 44 * n_el
    print(f"{name}: 3 x {H} x {W}, {args.rounds} alternating rounds, ms per step (median [min .. max]); torch / fused: {agree}")
    for n in cases:
        line = f"  {n:13s} {med[n]:.4f} [{min(ms[n]):.4f} .. {max(ms[n]):.4f}]  {cases[n][1]} steps per round"
        if "raster_step" in med:
            line += f"  {100.0 * med[n] / med['raster_step']:.1f} % of raster_step"
        if n == "fused_loss":
            line += f"  {moved / 1e9:.3f} GB at least -> {moved / (med[n] * 1e-3) / 1e12:.2f} TB/s"
        print(line)
    faster = all(f < t for f, t in zip(ms["fused_loss"], ms["torch_loss"]))
    print(f"  torch_loss / fused_loss = {med['torch_loss'] / med['fused_loss']:.2f} (per round: {', '.join('%.2f' % (t / f) for f, t in zip(ms['fused_loss'], ms['torch_loss']))}); "
          f"fused_loss faster in every round: {faster}")
    extras = training_extras(image, gen) if args.training or args.ab_lib else None
    if args.training:
        training_cases(name, image, target, extras)
    if args.ab_lib:
        library_cases(name, image, target, extras)
    return moved / (med["fused_loss"] * 1e-3) / 1e12


def report(name, cases, a, b):
    ms = {n: [] for n in cases}
    for _ in range(args.rounds):
        for n, step in cases.items():
            ms[n].append(timed(step, args.steps))
    for n in cases:
        print(f"  {n:13s} {statistics.median(ms[n]):.4f} [{min(ms[n]):.4f} .. {max(ms[n]):.4f}]  {args.steps} steps per round")
    print(f"  {a} / {b} = {statistics.median(ms[a]) / statistics.median(ms[b]):.2f} (per round: {', '.join('%.2f' % (t / f) for f, t in zip(ms[b], ms[a]))}); "
          f"{b} faster in every round: {all(f < t for f, t in zip(ms[b], ms[a]))}")


def training_extras(image, gen):
    """the extras of upstream's full step on image's frame: (exposure, alpha_mask, invdepth, mono_invdepth, depth_mask); exposure and invdepth are leaves"""
    H, W = image.shape[-2:]
    exposure = (torch.eye(3, 4, device=dev) + 0.05 * torch.randn(3, 4, device=dev, generator=gen)).requires_grad_(True)
    alpha_mask = (torch.rand(1, H, W, device=dev, generator=gen) > 0.1).float()
    invdepth = torch.rand(1, H, W, device=dev, generator=gen).requires_grad_(True)
    mono = torch.rand(1, H, W, device=dev, generator=gen)
    depth_mask = (torch.rand(1, H, W, device=dev, generator=gen) > 0.2).float()
    return exposure, alpha_mask, invdepth, mono, depth_mask


def fused_training_loss(image, target, extras):
    exposure, alpha_mask, invdepth, mono, depth_mask = extras
    return dgr.training_loss(image, target, 0.2, 0.5, exposure=exposure, clamp=True, alpha_mask=alpha_mask, invdepth=invdepth, mono_invdepth=mono, depth_mask=depth_mask)


def training_cases(name, image, target, extras):
    """the full loss of upstream's step: (a) torch ops around photometric_loss, (b) training_loss"""
    exposure, alpha_mask, invdepth, mono, depth_mask = extras

    def around():
        x = torch.matmul(image.permute(1, 2, 0), exposure[:3, :3]).permute(2, 0, 1) + exposure[:3, 3, None, None]
        x = x.clamp(0, 1) * alpha_mask
        return dgr.photometric_loss(x, target) + 0.5 * ((invdepth - mono) * depth_mask).abs().mean()

    def fused():
        return fused_training_loss(image, target, extras)

    def step_of(loss_fn):
        def step():
            loss_fn().backward()
            image.grad = exposure.grad = invdepth.grad = None
        return step

    leaves = (image, exposure, invdepth)
    a, b = around(), fused()
    ga, gb = torch.autograd.grad(a, leaves), torch.autograd.grad(b, leaves)
    diffs = ", ".join("%.3g of %.3g" % (float((x - y).abs().max()), float(x.abs().max())) for x, y in zip(ga, gb))
    print(f"{name} extended loss (exposure, clamp, alpha mask, depth term): loss {float(a.detach()):.7f} / {float(b.detach()):.7f}, "
          f"largest gradient differences (image, exposure, invdepth) {diffs}")
    report(name, {"around_fused": step_of(around), "training_loss": step_of(fused)}, "around_fused", "training_loss")


def library_cases(name, image, target, extras):
    """photometric_loss alone and training_loss with every extra, the default library against args.ab_lib, alternating"""
    exposure, _, invdepth, _, _ = extras

    def plain():
        dgr.photometric_loss(image, target).backward()
        image.grad = None

    def training():
        fused_training_loss(image, target, extras).backward()
        image.grad = exposure.grad = invdepth.grad = None

    steps = {"photometric_loss": plain, "training_loss": training}
    ms = {(fn, lib): [] for fn in steps for lib in ("default_lib", "other_lib")}
    for _ in range(args.rounds):
        for lib, path in (("default_lib", None), ("other_lib", args.ab_lib)):
            _C.use_library(path)   # (the next call loads it)
            for fn, step in steps.items():
                ms[fn, lib].append(timed(step, args.steps))
    _C.use_library(None)
    for fn in steps:
        print(f"{name} {fn} alone, the default library against {args.ab_lib}:")
        for lib in ("default_lib", "other_lib"):
            v = ms[fn, lib]
            print(f"  {lib:13s} {statistics.median(v):.4f} [{min(v):.4f} .. {max(v):.4f}]  {args.steps} steps per round")
        other = ms[fn, "other_lib"]
        print(f"  default_lib's median within or below other_lib's range: {statistics.median(ms[fn, 'default_lib']) <= max(other)}")


print(f"stp_hbm_probe copy, 1 GiB, this box, this run: {(rate := copy_rate()):.2f} TB/s")
for name in args.workloads:
    achieved = workload(name)
    print(f"  fused_loss moves its least bytes at {100.0 * achieved / rate:.1f} % of the copy rate")
    torch.cuda.empty_cache()
