"""Yardstick and inputs of the nearest-neighbour tests (knn_mean_dist2 / simple_knn._C.distCUDA2; include/stp_raster.h: stp_knn_mean_dist2).

brute32 is THE reference of the GPU tests, to the bit: numpy float32, all pairs, in the evaluation order the header fixes --
    dx = xj - xi, dy = yj - yi, dz = zj - zi      d2 = (dx * dx + dy * dy) + dz * dz      out[i] = ((b0 + b1) + b2) / 3
with b0 <= b1 <= b2 the three smallest d2 over j != i (by index).  numpy rounds every element-wise operation once and fuses nothing, and the
three smallest values of a multiset depend neither on ties nor on the order of a search: an exact search in that arithmetic has these bits.
brute64 is the same in float64; it is only ever printed beside a result, and it gives KNN_MEASURED below.

The named clouds are seeded.  They keep every squared distance either exactly 0 or above 1e-20, so that float32 denormals (which a device may
flush) never decide a result; tests/test_knn_cpu.py checks that on the three nearest of every point."""
import functools

import numpy as np

BOX = 256                          # == STP_KNN_BOX (include/stp_raster.h), checked in tests/test_knn_cpu.py
SIZES = (4, 5, 63, 64, 65, BOX - 1, BOX, BOX + 1, 3 * BOX + 7, 20011)
SMALL, LARGE, CROSSING = 3 * BOX + 7, 20011, 70001

# worst relative error of brute32 against brute64 over CASES (where brute64 > 0), as tests/test_knn_cpu.py measures it: the float32 rounding
# of three differences, three products, four sums and one division (the derivable cap: 11 roundings of 2^-24 each = 6.6e-7 < 1e-6)
KNN_MEASURED = 2.1e-7


def _nearest3(points, dtype, chunk=256):
    """(P, 3): the three smallest squared distances of every point to the others, ascending, all pairs in `dtype`."""
    p = np.ascontiguousarray(points, dtype=np.float32).astype(dtype)
    assert p.ndim == 2 and p.shape[1] == 3 and p.shape[0] >= 4
    P = p.shape[0]
    x, y, z = (np.ascontiguousarray(p[:, a]) for a in range(3))
    out = np.empty((P, 3), dtype)
    for s in range(0, P, chunk):
        e = min(P, s + chunk)
        dx, dy, dz = x[None, :] - x[s:e, None], y[None, :] - y[s:e, None], z[None, :] - z[s:e, None]
        np.multiply(dx, dx, out=dx)
        np.multiply(dy, dy, out=dy)
        np.multiply(dz, dz, out=dz)
        np.add(dx, dy, out=dx)
        np.add(dx, dz, out=dx)
        dx[np.arange(e - s), np.arange(s, e)] = np.inf   # j != i, by index
        out[s:e] = np.sort(np.partition(dx, 2, axis=1)[:, :3], axis=1)
    return out


def nearest3_32(points):
    return _nearest3(points, np.float32)


def nearest3_64(points):
    return _nearest3(points, np.float64)


def mean3(b):
    """((b0 + b1) + b2) / 3 in b's dtype"""
    return ((b[:, 0] + b[:, 1]) + b[:, 2]) / b.dtype.type(3.0)


def brute32(points):
    return mean3(nearest3_32(points))


def brute64(points):
    return mean3(nearest3_64(points))


# ---- the clouds ----------------------------------------------------------------------------------------------------------------------------

def uniform(P, seed=1):
    """a cube of side 10 about (1, -2, 3)"""
    r = np.random.default_rng(seed)
    return (r.uniform(-5.0, 5.0, (P, 3)) + [1.0, -2.0, 3.0]).astype(np.float32)


def clustered(P, seed=2):
    """12 Gaussian clusters with sigmas 10^U(-3, 1), centred near (100, -50, 30), and 5 outliers at 1e4: most points share few Morton cells"""
    r = np.random.default_rng(seed)
    centres = np.array([100.0, -50.0, 30.0]) + r.normal(0.0, 5.0, (12, 3))
    sigmas = 10.0 ** r.uniform(-3.0, 1.0, 12)
    which = r.integers(0, 12, P)
    p = centres[which] + r.normal(0.0, 1.0, (P, 3)) * sigmas[which, None]
    far = r.choice(P, 5, replace=False)
    p[far] = 1.0e4 * np.array([[1, 1, 1], [-1, 1, 1], [1, -1, 0.5], [0.25, 1, -1], [-1, -1, -1]], np.float64)
    return p.astype(np.float32)


def plane(P, seed=3):
    """z constant: the extent on one axis is 0"""
    p = uniform(P, seed)
    p[:, 2] = np.float32(0.75)
    return p


def line(P, seed=4):
    """two axes constant"""
    p = uniform(P, seed)
    p[:, 0] = np.float32(-3.5)
    p[:, 2] = np.float32(2.0)
    return p


def lattice(P=None, seed=5):
    """12^3 points, spacing 0.25, offset 7, in random order: ties are massive"""
    g = np.arange(12, dtype=np.float32) * np.float32(0.25) + np.float32(7.0)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(p.shape[0])])


def dups(P=None, seed=6):
    """300 points, each repeated 1-5 times, in random order: exact zeros; a point that occurs at least 4 times has the result 0"""
    r = np.random.default_rng(seed)
    base = uniform(300, seed + 100)
    p = np.repeat(base, r.integers(1, 6, 300), axis=0)
    return np.ascontiguousarray(p[r.permutation(p.shape[0])])


def outlier(P, seed=7):
    """a unit cube plus one point at 1e6: the whole cube falls in one Morton cell"""
    r = np.random.default_rng(seed)
    p = r.uniform(0.0, 1.0, (P, 3)).astype(np.float32)
    p[P // 3] = np.float32(1.0e6)
    return p


CLOUDS = {"uniform": uniform, "clustered": clustered, "plane": plane, "line": line, "lattice": lattice, "dups": dups, "outlier": outlier}

# the GPU tests' (cloud, P) cases: uniform at every size; every cloud at 3 BOX + 7 (lattice and dups have their own sizes, both above it);
# clustered at 20 011 too
CASES = tuple(("uniform", P) for P in SIZES) + tuple((name, SMALL) for name in CLOUDS if name != "uniform") + (("clustered", LARGE),)


@functools.lru_cache(maxsize=None)
def case(name, P):
    """(points, brute32(points)) of a named case, computed once per process; both read-only"""
    p = CLOUDS[name](P)
    ref = brute32(p)
    p.setflags(write=False)
    ref.setflags(write=False)
    return p, ref
