#!/usr/bin/env python3
"""Step time of the inverse-depth output through the public API, beside the plain step and the two-pass workaround of the same run (GPU box).
usage: tools/invdepth_cost.py [workload] [variant] [steps] [rounds]      (default: C2 full 30 3)

One forward + backward per step, timed with events around `steps` steps after five warm-up steps; the three cases alternate `rounds`
times and the median per case is printed with its spread.  Cases:
  plain      the image with dL_dout = the scene's
  invdepth   settings._invdepth = True and an L1 term on the inverse depth beside the image's gradient: one forward, one backward
  two_pass   what a trainer does without the output: the plain step + a second render with colors_precomp = (1/z, 0, 0), bg = 0, its own
             backward with the L1 term's gradient in channel 0, and 1/z chained to means3D in torch
After the timing the per-stage split of `plain` and `invdepth` (the library's stage timer: Preprocess .. BwdPreprocess, mean ms)."""
import ctypes, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stopthepop-rasterization_amd")); sys.path.insert(0, ROOT)
import torch
import bench
import diff_gaussian_rasterization as dgr
from diff_gaussian_rasterization import _C, scenes

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
cam = dict(viewmatrix=t(sc.viewmatrix), projmatrix=t(sc.projmatrix), inv_viewprojmatrix=t(sc.inv_viewprojmatrix), campos=t(sc.campos))
V = cam["viewmatrix"].reshape(4, 4)
zero_bg = torch.zeros(3, device=dev)
empty = torch.Tensor([])


def rasterizer(invdepth, bg):
    es = bench.settings_for(variant, workload)
    es._invdepth = invdepth
    rs = dgr.GaussianRasterizationSettings(image_height=sc.H, image_width=sc.W, tanfovx=sc.tanfovx, tanfovy=sc.tanfovy, bg=bg, scale_modifier=1.0,
                                           sh_degree=sc.sh_degree, prefiltered=False, settings=es, render_depth=False, debug=False, **cam)
    return dgr.GaussianRasterizer(rs)


with torch.no_grad():   # the prior the L1 term is taken against: the scene's own inverse depth, scaled (the sign of the difference is what counts)
    prior = 0.9 * rasterizer(True, t(sc.bg))(gauss["means3D"], means2D, gauss["opacities"], shs=gauss["shs"], scales=gauss["scales"],
                                             rotations=gauss["rotations"])[2]


def case(name):
    plain, with_depth, channel = rasterizer(False, t(sc.bg)), rasterizer(True, t(sc.bg)), rasterizer(False, zero_bg)
    call = lambda r, **kw: r(gauss["means3D"], means2D, gauss["opacities"], scales=gauss["scales"], rotations=gauss["rotations"], **kw)

    def step():
        if name == "invdepth":
            image, _, inv = call(with_depth, shs=gauss["shs"])
            ((image * w).sum() + 0.1 * (inv - prior).abs().mean()).backward()
        else:
            (call(plain, shs=gauss["shs"])[0] * w).sum().backward()
            if name == "two_pass":
                c = 1.0 / (gauss["means3D"] @ V[:3, 2] + V[3, 2])
                colors = torch.stack([c, torch.zeros_like(c), torch.zeros_like(c)], 1)
                inv = call(channel, colors_precomp=colors)[0][0:1]
                (0.1 * (inv - prior).abs().mean()).backward()
        for x in list(gauss.values()) + [means2D]:
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


names = ("plain", "invdepth", "two_pass")
cases = {n: case(n) for n in names}
ms = {n: [] for n in names}
for _ in range(rounds):
    for n in names:
        ms[n].append(timed(cases[n]))
base = statistics.median(ms["plain"])
print(f"{workload}-{variant}, {sc.W}x{sc.H}, {steps} steps x {rounds} rounds, ms per step (median [min .. max], against plain)")
for n in names:
    m = statistics.median(ms[n])
    print(f"  {n:10s} {m:.4f} [{min(ms[n]):.4f} .. {max(ms[n]):.4f}]  {m - base:+.4f} ms  {100.0 * (m / base - 1.0):+.2f} %")

L = _C._load()
stages = ("Preprocess", "Duplicate", "Sort", "Render", "BwdRender", "BwdPreprocess")
print("per-stage mean ms over", steps, "steps:")
for n in ("plain", "invdepth"):
    L.stp_timing_enable(1)
    for _ in range(steps):
        cases[n]()
    torch.cuda.synchronize()
    buf = (ctypes.c_float * 6)()
    L.stp_timing_read(buf)
    L.stp_timing_enable(0)
    print(f"  {n:10s} " + "  ".join(f"{s} {v:.4f}" for s, v in zip(stages, buf)))
