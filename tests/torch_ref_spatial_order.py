"""Yardstick and inputs of the spatial-order tests (spatial_order, gather_tensors, reorder_gaussians_; include/stp_raster.h: stp_spatial_order,
stp_gather_rows).

order_and_codes is THE reference of the GPU tests, to the bit: a numpy restatement of the definition the header fixes.  Per axis a
    key_a(i) = ordered_bits(xyz[i][a])           sorted_a = np.sort(key_a)           splitter_a[k - 1] = sorted_a[k P // 1024], k = 1 .. 1023
    cell_a(i) = np.searchsorted(splitter_a, key_a(i), side="right")                 (the number of splitters <= the key, 0 .. 1023)
then code(i) = spread10(cell_x) | spread10(cell_y) << 1 | spread10(cell_z) << 2, and order = np.argsort(code, kind="stable").  Everything is
integer arithmetic: there is no tolerance, the comparison is np.array_equal.  codes are returned in SORTED order, codes[s] = code(order[s]),
as the call returns them.

The clouds are those of tests/torch_ref_knn.py; SIZES adds the sizes below the knn call's four points and the edge of the 1024 cells."""
import functools

import numpy as np

import torch_ref_knn as trk

CELLS = 1024
# 1..4: below what knn takes; the wave and workgroup edges; 1023..1025: below 1024 points the splitters repeat; knn's 775 and 20 011
SIZES = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, trk.SMALL, trk.LARGE)
CROSSING = trk.CROSSING            # above 2^16, where rocPRIM changes its plan
# uniform at every size; every other cloud at 775 (lattice and dups have their own sizes); clustered at 20 011 and above 2^16 too
CASES = tuple(("uniform", P) for P in SIZES) + tuple((name, trk.SMALL) for name in trk.CLOUDS if name != "uniform") + (("clustered", trk.LARGE), ("clustered", CROSSING))

SIGNS = np.float32([[0, 0, 0], [-0.0, 0, 0], [np.inf, 0, 0], [-np.inf, 0, 0], [1, 0, 0]])   # -> [3, 1, 0, 4, 2]


def ordered_bits(v):
    """float32 -> uint32 of the same order: -0 below +0, the infinities at the ends"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def spread10(v):
    """bit b of 10 -> bit 3 b"""
    v = v.astype(np.uint32)
    out = np.zeros_like(v)
    for b in range(10):
        out |= ((v >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b)
    return out


def codes_of(points):
    """code(i) of every point, in INPUT order"""
    p = np.ascontiguousarray(points, dtype=np.float32)
    assert p.ndim == 2 and p.shape[1] == 3 and p.shape[0] >= 1
    P = p.shape[0]
    code = np.zeros(P, np.uint32)
    for a in range(3):
        key = ordered_bits(p[:, a])
        srt = np.sort(key)
        splitters = srt[(np.arange(1, CELLS, dtype=np.int64) * P) // CELLS]
        cell = np.searchsorted(splitters, key, side="right")
        assert cell.min() >= 0 and cell.max() <= CELLS - 1
        code |= spread10(cell) << np.uint32(a)
    return code


def order_and_codes(points):
    """(order int32 (P,), codes uint32 (P,) in sorted order)"""
    code = codes_of(points)
    order = np.argsort(code, kind="stable").astype(np.int32)
    return order, code[order]


@functools.lru_cache(maxsize=None)
def case(name, P):
    """(points, order, sorted codes) of a named case, computed once per process; all read-only"""
    p = trk.CLOUDS[name](P)
    order, codes = order_and_codes(p)
    for a in (p, order, codes):
        a.setflags(write=False)
    return p, order, codes
