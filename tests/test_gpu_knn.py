"""GPU tests of the nearest-neighbour call (knn_mean_dist2, simple_knn._C.distCUDA2; include/stp_raster.h: stp_knn_mean_dist2).

THE CRITERION IS np.array_equal WITH brute32 (tests/torch_ref_knn.py: numpy float32, all pairs, the header's evaluation order).  There is no
tolerance: the three smallest values of a multiset do not depend on ties or on the order of a search, so an exact search in that arithmetic
has those bits.  The float64 comparison is only printed.

The search owns one box of B = STP_KNN_BOX = 256 sorted points per workgroup, one query per lane, and walks the other boxes 256 at a step:
the sizes are the edges of a wave and of a box (4, 5, 63, 64, 65, B - 1, B, B + 1), several boxes with a partial last one (3 B + 7), a
cloud whose walk takes more than one step in both directions (20 011: 79 boxes; 70 001: 274 boxes, more than one step of 256), and a count
above 2^16.  The clouds are those in which a box test can go wrong: axes without extent, massive ties, exact duplicates, an outlier that
puts everything else into one Morton cell, clusters of very different densities."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import torch_ref_knn as trk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def distCUDA2(points):
    from simple_knn._C import distCUDA2 as f   # the trainers' import line
    return f(points)


def run(p):
    """distCUDA2 of a numpy cloud, as create_from_pcd calls it -> numpy float32 (P,)"""
    x = torch.from_numpy(np.array(p)).float().cuda()   # (a copy: the shared clouds are read-only)
    out = distCUDA2(x)
    assert out.shape == (x.shape[0],) and out.dtype == torch.float32 and out.is_cuda and not out.requires_grad
    return out.cpu().numpy()


def report(name, got, p, ref32):
    if p.shape[0] <= trk.SMALL:   # (printed only; the float64 evaluation of the large clouds is tests/test_knn_cpu.py's)
        ref64 = trk.brute64(p)
        pos = ref64 > 0
        err = float(np.max(np.abs(got[pos].astype(np.float64) - ref64[pos]) / ref64[pos])) if pos.any() else 0.0
        print(f"\n{name} P={p.shape[0]}: worst relative error against float64 {err:.3g} (brute32's own: at most {trk.KNN_MEASURED:.3g})")
    wrong = np.flatnonzero(got.view(np.uint32) != ref32.view(np.uint32))
    if wrong.size:
        i = int(wrong[0])
        print(f"\n{name} P={p.shape[0]}: {wrong.size} results differ from brute32; first at {i}: got {got[i]!r} expected {ref32[i]!r}")


@pytest.mark.parametrize("name,P", trk.CASES, ids=[f"{n}-{P}" for n, P in trk.CASES])
def test_bit_equal_to_the_float32_brute_force(name, P):
    p, ref32 = trk.case(name, P)
    got = run(p)
    report(name, got, p, ref32)
    assert np.array_equal(got, ref32)
    if name == "dups":   # a point that occurs at least four times has three neighbours at distance 0
        _, inverse, counts = np.unique(p, axis=0, return_inverse=True, return_counts=True)
        assert np.all(got[counts[inverse.reshape(-1)] >= 4] == 0)


def test_results_are_in_input_order():
    p, ref32 = trk.case("clustered", trk.SMALL)
    base = run(p)
    assert np.array_equal(base, ref32)
    perm = np.random.default_rng(11).permutation(p.shape[0])
    assert np.array_equal(run(p[perm]), base[perm])
    by_x = np.argsort(p[:, 0], kind="stable")     # a cloud that arrives sorted along an axis
    assert np.array_equal(run(p[by_x]), base[by_x])
    assert np.array_equal(run(p[::-1].copy()), base[::-1])


def test_crossing_65536_points_against_eager_torch():
    """P = 70 001, clustered.  The yardstick is built on the GPU by eager torch in float32, 1024 queries at a time: sub, mul and add one step at a
    time (eager element-wise torch operations are single IEEE operations), self masked to inf, topk(3, largest=False); the final
    (b0 + b1) + b2 and / 3 are numpy's on the CPU, so that nothing rests on the device's division."""
    P = trk.CROSSING
    p = trk.clustered(P)
    x = torch.from_numpy(p).cuda()
    cols = [x[:, a].contiguous() for a in range(3)]
    best = torch.empty((P, 3), dtype=torch.float32, device="cuda")
    for s in range(0, P, 1024):
        e = min(P, s + 1024)
        d = None
        for c in cols:
            diff = torch.sub(c[None, :], c[s:e, None])
            sq = torch.mul(diff, diff)
            d = sq if d is None else torch.add(d, sq)
        rows = torch.arange(e - s, device="cuda")
        d[rows, rows + s] = math.inf
        best[s:e] = torch.topk(d, 3, dim=1, largest=False, sorted=True).values
    b = best.cpu().numpy()
    assert np.all(b[:, 0] <= b[:, 1]) and np.all(b[:, 1] <= b[:, 2]) and np.all(np.isfinite(b))
    ref = trk.mean3(b)
    assert ref.dtype == np.float32
    got = run(p)
    report("clustered", got, p, ref)
    assert np.array_equal(got, ref)


def test_views_repeats_and_streams():
    p, ref32 = trk.case("uniform", trk.SMALL)
    x = torch.from_numpy(np.array(p)).cuda()
    first = distCUDA2(x)
    assert np.array_equal(first.cpu().numpy(), ref32)
    assert torch.equal(distCUDA2(x).view(torch.int32), first.view(torch.int32))              # a second call: equal bits
    wide = torch.zeros((p.shape[0], 5), device="cuda")
    wide[:, 1:4] = x
    view = wide[:, 1:4]
    assert not view.is_contiguous()
    assert torch.equal(distCUDA2(view).view(torch.int32), first.view(torch.int32))           # a non-contiguous view is made contiguous
    assert torch.equal(distCUDA2(x.t().contiguous().t()).view(torch.int32), first.view(torch.int32))   # (P, 3) with column-major strides
    leaf = x.clone().requires_grad_(True)
    out = distCUDA2(leaf)
    assert not out.requires_grad and out.grad_fn is None and torch.equal(out.view(torch.int32), first.view(torch.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = distCUDA2(x)
    side.synchronize()
    assert torch.equal(on_side.view(torch.int32), first.view(torch.int32))
    empty = distCUDA2(torch.zeros((0, 3), device="cuda"))
    assert empty.shape == (0,) and empty.dtype == torch.float32 and empty.is_cuda
    for n in (1, 2, 3):
        with pytest.raises(RuntimeError, match="needs at least 4 points"):
            distCUDA2(x[:n])
    import diff_gaussian_rasterization as dgr
    assert torch.equal(dgr.knn_mean_dist2(x).view(torch.int32), first.view(torch.int32))


def test_the_trainer_example_initialises_its_scales_with_it():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_render.py"), "--init-scales", "knn", "--iters", "3", "--points", "2000"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert re.search(r"initial scales from distCUDA2 over 2000 points", r.stdout)
    m = re.search(r"(\S+) -> (\S+); depth visualisation", r.stdout)
    assert m and math.isfinite(float(m.group(1))) and math.isfinite(float(m.group(2)))
