#!/usr/bin/env python3
"""Cost of distCUDA2 (knn_mean_dist2; include/stp_raster.h: stp_knn_mean_dist2) on uniform and clustered clouds (GPU box).
usage: tools/knn_cost.py [--sizes 100000 1000000 6000000] [--rounds 5] [--brute-at 100000]

Per cloud and size: the median over `rounds` timed calls (device events around one call, scratch and output allocation included, after two
warm-up calls of the same shape) and the rounds themselves.  At --brute-at points also the brute force a user has without this call --
torch.cdist of 4096 queries at a time against the whole cloud, the own point masked, topk(3, largest=False), squared and averaged -- timed
the same way, alternating with distCUDA2, and the largest relative difference of the two results (cdist is not bit-exact: printed only).

Boxes a workgroup scans.  The kernel has no counter; what is printed is a bracket computed here from the RESULT, over the kernel's own
boxes (rebuilt with torch: Morton order over 1024 equal-count cells per axis, 256 points per box): for every query box, the number of other boxes whose box-to-box lower bound
does not exceed T, for T = the largest mean of the box's queries (every b2 is >= its mean: a walk in ANY order scans at least these) and for
T = three times that (every b2 is <= three times its mean: a walk that knew the final b2 from the start would scan at most these).  The walk
starts with a larger b2 than the final one, so it can scan more than the upper figure; on Morton-sorted clouds the near boxes come first and
it stays close."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stopthepop-rasterization_amd")); sys.path.insert(0, ROOT)
import torch
from diff_gaussian_rasterization import _C
from simple_knn._C import distCUDA2

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="*", default=[100_000, 1_000_000, 6_000_000])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--brute-at", type=int, default=100_000)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/knn_cost.py measures on a GPU; there is none")
dev = torch.device("cuda:0")
BOX = _C.KNN_BOX


def uniform(P, gen):
    return torch.rand(P, 3, device=dev, generator=gen) * 10.0 - 5.0


def clustered(P, gen):
    """12 Gaussian clusters with sigmas 10^U(-3, 1) near (100, -50, 30) and 5 outliers at 1e4 (the tests' cloud, drawn with torch)"""
    centres = torch.tensor([100.0, -50.0, 30.0], device=dev) + 5.0 * torch.randn(12, 3, device=dev, generator=gen)
    sigmas = 10.0 ** (torch.rand(12, device=dev, generator=gen) * 4.0 - 3.0)
    which = torch.randint(0, 12, (P,), device=dev, generator=gen)
    p = centres[which] + torch.randn(P, 3, device=dev, generator=gen) * sigmas[which, None]
    p[:5] = 1.0e4 * torch.tensor([[1, 1, 1], [-1, 1, 1], [1, -1, 0.5], [0.25, 1, -1], [-1, -1, -1]], device=dev)
    return p[torch.randperm(P, device=dev, generator=gen)].contiguous()


def timed(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def brute(x):
    P = x.shape[0]
    out = torch.empty(P, device=dev)
    for s in range(0, P, 4096):
        e = min(P, s + 4096)
        d = torch.cdist(x[s:e], x)
        rows = torch.arange(e - s, device=dev)
        d[rows, rows + s] = float("inf")
        b = torch.topk(d, 3, dim=1, largest=False).values
        out[s:e] = (b * b).mean(dim=1)
    return out


def spread10(v):
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    return (v | (v << 2)) & 0x09249249


def scanned_bracket(x, mean):
    """(at least, at most with the final b2 known) scanned boxes per workgroup, averaged over the workgroups, as shares of the other boxes"""
    P = x.shape[0]
    cells = []
    for a in range(3):   # the kernel's cells: 1024 runs of equal length of the sorted coordinates per axis
        col = x[:, a].contiguous()
        cuts = torch.sort(col).values[(torch.arange(1, 1024, device=dev, dtype=torch.int64) * P) // 1024]
        cells.append(torch.searchsorted(cuts, col, right=True))
    order = torch.argsort(spread10(cells[0]) | (spread10(cells[1]) << 1) | (spread10(cells[2]) << 2), stable=True)
    boxes = (P + BOX - 1) // BOX
    pad = boxes * BOX - P
    xs = torch.cat([x[order], x[order][-1:].expand(pad, 3)])
    ms = torch.cat([mean[order], mean[order][-1:].expand(pad)])
    blo, bhi = xs.view(boxes, BOX, 3).min(dim=1).values, xs.view(boxes, BOX, 3).max(dim=1).values
    t = ms.view(boxes, BOX).max(dim=1).values
    least = most = 0
    for s in range(0, boxes, 2048):
        e = min(boxes, s + 2048)
        gap = torch.maximum(torch.maximum(blo[None, :, :] - bhi[s:e, None, :], blo[s:e, None, :] - bhi[None, :, :]), torch.zeros((), device=dev))
        bound = (gap * gap).sum(dim=2)
        bound[torch.arange(e - s, device=dev), torch.arange(s, e, device=dev)] = float("inf")   # the own box is the seed, not a scan
        least += int((bound <= t[s:e, None]).sum())
        most += int((bound <= 3.0 * t[s:e, None]).sum())
    others = max(1, boxes * (boxes - 1))
    return boxes, least / others, most / others


print(f"distCUDA2 cost, {torch.cuda.get_device_name(0)}; box = {BOX} points; ms per call, median of {args.rounds} rounds after 2 warm-up calls")
for P in args.sizes:
    for name, make in (("uniform", uniform), ("clustered", clustered)):
        x = make(P, torch.Generator(device=dev).manual_seed(1))
        with_brute = P == args.brute_at
        for _ in range(2):
            out = distCUDA2(x)
            if with_brute:
                ref = brute(x)
        torch.cuda.synchronize()
        ms, ms_brute = [], []
        for _ in range(args.rounds):
            ms.append(timed(lambda: distCUDA2(x))[0])
            if with_brute:
                ms_brute.append(timed(lambda: brute(x))[0])
        boxes, least, most = scanned_bracket(x, out)
        print(f"{name:9s} P = {P:8d} ({boxes} boxes, scratch {_C.knn_scratch_bytes(P) / 2 ** 20:.0f} MiB): distCUDA2 median {statistics.median(ms):.3f}  rounds "
              + " ".join(f"{t:.3f}" for t in ms) + f";  boxes scanned per workgroup, of the others: at least {100 * least:.2f} %, "
              f"{100 * most:.2f} % with the final b2 known")
        if with_brute:
            pos = ref > 0
            diff = float(((out[pos] - ref[pos]).abs() / ref[pos]).max())
            faster = sum(a < b for a, b in zip(ms, ms_brute))
            print(f"          chunked torch.cdist + topk: median {statistics.median(ms_brute):.3f}  rounds " + " ".join(f"{t:.3f}" for t in ms_brute)
                  + f";  distCUDA2 / brute force = {statistics.median(ms) / statistics.median(ms_brute):.4f} (faster in {faster} of {args.rounds} rounds); "
                  f"largest relative difference of the results {diff:.3g}")
        del x, out
        torch.cuda.empty_cache()
