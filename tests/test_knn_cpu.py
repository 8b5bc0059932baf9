"""CPU tests of the nearest-neighbour call (knn_mean_dist2, distCUDA2, simple_knn._C.distCUDA2; include/stp_raster.h: stp_knn_scratch_bytes,
stp_knn_mean_dist2): the public names and the trainers' import line, the C ABI's declarations, exports and argument validation (which runs
before any launch, so without a GPU), what the functions refuse, hand-computed pins of the yardstick tests/torch_ref_knn.py, and the
MEASUREMENT of that yardstick's own float32 error on exactly the GPU tests' inputs.

The GPU tests compare bit for bit with brute32 and have no tolerance to fix here.  What is measured is how far brute32 -- and with it the
kernel -- is from the float64 evaluation: worst relative error over tests/torch_ref_knn.CASES where brute64 > 0
    measured 2.05e-7  ->  KNN_MEASURED = 2.1e-7     (the derivable cap: 11 roundings of 2^-24 = 6.6e-7 < 1e-6)"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import torch_ref_knn as trk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1


def test_names_are_public_and_the_trainers_import_line_works():
    import diff_gaussian_rasterization as dgr
    from simple_knn._C import distCUDA2   # the line of GaussianModel.create_from_pcd
    import simple_knn
    assert "knn_mean_dist2" in dgr.__all__ and "distCUDA2" in dgr.__all__ and "dist_cuda2" in dgr.__all__
    assert distCUDA2 is dgr.knn_mean_dist2 and dgr.distCUDA2 is dgr.knn_mean_dist2 and dgr.dist_cuda2 is dgr.knn_mean_dist2
    assert simple_knn.distCUDA2 is distCUDA2
    from diff_gaussian_rasterization import _C
    assert callable(_C.knn_mean_dist2) and callable(_C.knn_scratch_bytes)
    assert os.path.dirname(os.path.dirname(os.path.abspath(simple_knn.__file__))) == os.path.dirname(os.path.dirname(os.path.abspath(dgr.__file__)))
    setup_py = open(os.path.join(ROOT, "setup.py")).read()
    assert re.search(r"packages=\[[^\]]*\"simple_knn\"", setup_py)


def test_header_declares_both_calls():
    h = open(os.path.join(ROOT, "include", "stp_raster.h")).read()
    assert int(re.search(r"#define\s+STP_ABI_VERSION\s+(\d+)\b", h).group(1)) == 7
    from diff_gaussian_rasterization import _C
    assert int(re.search(r"#define\s+STP_KNN_BOX\s+(\d+)\b", h).group(1)) == _C.KNN_BOX == trk.BOX and trk.BOX % 64 == 0
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"size_t\s+stp_knn_scratch_bytes\s*\(\s*int\s+P\s*\)\s*;", h)
    assert re.search(r"int\s+stp_knn_mean_dist2\s*\(\s*int\s+P\s*,\s*const\s+float\s*\*\s*points\s*,\s*void\s*\*\s*scratch\s*,\s*size_t\s+scratch_bytes\s*,"
                     r"\s*float\s*\*\s*mean_dist2\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)


def test_library_exports_both_calls_and_the_abi_stays_7():
    from diff_gaussian_rasterization import _C
    L = _C._load()
    assert L.stp_abi_version() == 7
    for path in (_C.library_path(), os.path.join(os.path.dirname(_C.library_path()), "libstp_raster_fma.so")):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        for name in ("stp_knn_scratch_bytes", "stp_knn_mean_dist2"):
            assert re.search(r" T " + name + r"$", nm, re.M), (path, name)
    for name in ("stp_knn_scratch_bytes", "stp_knn_mean_dist2"):
        assert hasattr(L, name) and _C._require(name) is not None
    assert callable(_C._native().knn_mean_dist2)


def test_loader_message_for_a_library_without_the_symbols(monkeypatch):
    import types
    from diff_gaussian_rasterization import _C
    monkeypatch.setattr(_C, "_lib", types.SimpleNamespace())   # a loaded library that predates the exports
    for name, call in (("stp_knn_mean_dist2", lambda: _C.knn_mean_dist2(torch.zeros(8, 3))), ("stp_knn_scratch_bytes", lambda: _C.knn_scratch_bytes(8))):
        with pytest.raises(RuntimeError) as ex:
            call()
        assert str(ex.value) == f"{_C.library_path()} does not export {name} (a library built before the nearest-neighbour kernels): rebuild it"


def test_c_abi_validates_before_any_launch():
    """The refusals come before the launch, so they need no GPU (a launch here would fail with STP_ERR_HIP, not -1); the pointers are never
    followed (they are host addresses)."""
    from diff_gaussian_rasterization import _C
    L = _C._load()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a16 = (a + 15) & ~15
    err = lambda: L.stp_last_error().decode()
    big = 1 << 40   # (a size only: nothing is read or written through `scratch`)
    knn = lambda P=8, pts=a, scratch=a16, nbytes=big, out=a: L.stp_knn_mean_dist2(P, pts, scratch, nbytes, out, None)
    for P in (-1, -(2 ** 31)):
        assert knn(P=P) == -1 and "stp_knn_mean_dist2" in err() and "negative P" in err()
    for P in (1, 2, 3):
        assert knn(P=P) == -1 and "stp_knn_mean_dist2" in err() and "needs at least 4 points" in err() and f"P = {P}" in err()
    for name in ("pts", "scratch", "out"):
        assert knn(**{name: None}) == -1 and "stp_knn_mean_dist2: null pointer" in err()
    need = L.stp_knn_scratch_bytes(8)
    assert need > 0
    for nbytes in (0, need - 1):
        assert knn(nbytes=nbytes) == -1 and "stp_knn_mean_dist2: scratch of " in err() and f"stp_knn_scratch_bytes(P) = {need}" in err()
    assert knn(scratch=a16 + 4) == -1 and "stp_knn_mean_dist2: scratch is not 16-byte aligned" in err()
    assert knn(P=0) == 0 and knn(P=0, pts=None, scratch=None, nbytes=0, out=None) == 0   # empty work: no launch, 0
    assert knn(P=3, pts=None, scratch=None, nbytes=0, out=None) == -1 and "needs at least 4 points" in err()   # (too few points come first)
    assert all(x == 0.0 for x in buf)


def test_scratch_bytes_is_monotone_and_does_not_overflow():
    from diff_gaussian_rasterization import _C
    f = _C.knn_scratch_bytes
    assert f(0) == 0 and f(-1) == 0 and f(-(2 ** 31)) == 0
    at = {P: f(P) for P in (4, 2 ** 16 + 1, INT_MAX)}
    # the carve: two key and two value buffers (4 x 4 bytes), one 16-byte record per point, two 16-byte corners per box
    for P, got in at.items():
        own = 32 * P + 32 * ((P + trk.BOX - 1) // trk.BOX)
        assert own <= got <= own + own // 8 + (1 << 20), (P, got, own)
    assert at[INT_MAX] > 2 ** 36 and at[INT_MAX] < 2 ** 38   # 32 bytes per point of 2^31: 64 GiB and a little, no wrap-around
    sweep = sorted(set([1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000, 4095, 4096, 4097, 2 ** 16 - 1, 2 ** 16, 2 ** 16 + 1, 10 ** 5, 10 ** 6, 6 * 10 ** 6,
                        2 ** 24, 2 ** 24 + 1, 2 ** 30, 2 ** 30 + 1, INT_MAX - 1, INT_MAX] + [int(1.37 ** k) for k in range(4, 68)]))
    sizes = [f(P) for P in sweep]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), list(zip(sweep, sizes))
    assert all(s % 256 == 0 and s > 0 for s in sizes)
    assert f(10 ** 6) == f(10 ** 6)   # a function of P alone


def test_refusals_name_the_argument_and_come_before_the_device():
    """What is wrong with the tensor itself is refused before where it lives is looked at: every refusal can be met without a GPU."""
    import diff_gaussian_rasterization as dgr
    from simple_knn._C import distCUDA2
    p = torch.zeros(8, 3)
    for fn in (dgr.knn_mean_dist2, distCUDA2):
        for bad, what in ((p.double(), "points: expected float32"), (p.half(), "points: expected float32"), (p.int(), "points: expected float32"),
                          (torch.zeros(8, 4), r"points must be \(P, 3\)"), (torch.zeros(8), r"points must be \(P, 3\)"),
                          (torch.zeros(2, 8, 3), r"points must be \(P, 3\)"), (torch.zeros(3, 8).t()[:, :2], r"points must be \(P, 3\)"),
                          (p[:1], "needs at least 4 points"), (p[:2], "needs at least 4 points"), (p[:3], "needs at least 4 points"),
                          (p, "no CPU path"), (p[:4], "no CPU path"), (torch.zeros(3, 8).t(), "no CPU path"), (p[:0], "no CPU path"),
                          (p.clone().requires_grad_(True), "no CPU path")):
            with pytest.raises(RuntimeError, match=what):
                fn(bad)
    with pytest.raises(RuntimeError, match="points: expected float32"):   # (the dtype comes first, then the shape, then the count)
        dgr.knn_mean_dist2(torch.zeros(2, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"points must be \(P, 3\)"):
        dgr.knn_mean_dist2(torch.zeros(2, 4))


def test_yardstick_pins():
    # the corners of a unit square and its centre: a corner sees the centre at 1/2 and two corners at 1; the centre four corners at 1/2
    sq = np.float32([[0, 0, 5], [1, 0, 5], [0, 1, 5], [1, 1, 5], [0.5, 0.5, 5]])
    assert trk.brute64(sq).tolist() == [2.5 / 3] * 4 + [0.5]
    assert np.array_equal(trk.brute32(sq), np.float32([np.float32(2.5) / np.float32(3.0)] * 4 + [0.5]))
    assert trk.brute32(sq).dtype == np.float32 and trk.brute64(sq).dtype == np.float64
    assert trk.nearest3_32(sq).tolist() == [[0.5, 1.0, 1.0]] * 4 + [[0.5, 0.5, 0.5]]
    # 3-4-5: from the origin 9, 16 and 25 (the fifth point is farther), mean 50 / 3
    tri = np.float32([[0, 0, 0], [3, 0, 0], [0, 4, 0], [0, 0, 5], [0, 0, -30]])
    assert trk.nearest3_32(tri)[0].tolist() == [9.0, 16.0, 25.0] and trk.brute32(tri)[0] == np.float32(50.0) / np.float32(3.0)
    assert trk.nearest3_32(tri)[1].tolist() == [9.0, 25.0, 34.0]     # from (3, 0, 0): the origin, (0, 4, 0) at 9 + 16, (0, 0, 5) at 9 + 25
    # four coincident points: every point has three neighbours at distance 0 -- j != i is by index, not by position
    same = np.float32([[1.5, -2.25, 1e3]] * 4)
    assert np.array_equal(trk.brute32(same), np.zeros(4, np.float32)) and np.array_equal(trk.brute64(same), np.zeros(4))
    # the evaluation order is (dx^2 + dy^2) + dz^2, not dx^2 + (dy^2 + dz^2): (2^-24 + 2^-24) + 1 = 1 + 2^-23, but 2^-24 + (2^-24 + 1) = 1
    e = np.float32(2.0 ** -12)
    order = np.float32([[0, 0, 0], [e, e, 1], [9, 9, 9], [9, 9, 10], [9, 10, 9]])
    assert trk.nearest3_32(order)[0, 0] == np.float32(1.0 + 2.0 ** -23) and e * e + (e * e + np.float32(1.0)) == np.float32(1.0)


def test_inputs_cover_what_the_gpu_tests_need():
    B = trk.BOX
    assert trk.SIZES == (4, 5, 63, 64, 65, B - 1, B, B + 1, 3 * B + 7, 20011) and trk.SMALL == 3 * B + 7 and trk.CROSSING > 2 ** 16
    assert set(name for name, _ in trk.CASES) == set(trk.CLOUDS) == {"uniform", "clustered", "plane", "line", "lattice", "dups", "outlier"}
    assert ("uniform", 20011) in trk.CASES and ("clustered", 20011) in trk.CASES
    for name, P in trk.CASES:
        p = trk.CLOUDS[name](P)
        assert p.dtype == np.float32 and p.ndim == 2 and p.shape[1] == 3 and np.all(np.isfinite(p)) and np.array_equal(p, trk.CLOUDS[name](P))
        if name not in ("lattice", "dups"):
            assert p.shape[0] == P
        assert p.shape[0] >= trk.SMALL or name == "uniform"
    extent = lambda p: p.max(axis=0) - p.min(axis=0)
    assert extent(trk.plane(trk.SMALL)).tolist().count(0.0) == 1 and extent(trk.line(trk.SMALL)).tolist().count(0.0) == 2
    assert trk.lattice().shape == (12 ** 3, 3) and float(trk.lattice().min()) == 7.0 and float(trk.lattice().max()) == 7.0 + 11 * 0.25
    d = trk.dups()
    _, counts = np.unique(d, axis=0, return_counts=True)
    assert counts.size == 300 and set(counts.tolist()) == {1, 2, 3, 4, 5}
    ref = trk.case("dups", trk.SMALL)[1]
    _, inverse, counts = np.unique(d, axis=0, return_inverse=True, return_counts=True)
    assert np.all(ref[counts[inverse.reshape(-1)] >= 4] == 0) and np.all(ref[counts[inverse.reshape(-1)] == 1] > 0)
    o = trk.outlier(trk.SMALL)
    assert np.sum(np.all(o == np.float32(1e6), axis=1)) == 1 and np.sum((o >= 0).all(axis=1) & (o <= 1).all(axis=1)) == trk.SMALL - 1
    c = trk.clustered(trk.LARGE)
    assert np.sum(np.abs(c).max(axis=1) == 1e4) == 5 and np.abs(np.median(c, axis=0) - [100, -50, 30]).max() < 15


def test_measured_error_of_the_yardstick():
    worst = 0.0
    for name, P in trk.CASES:
        p, ref32 = trk.case(name, P)
        b64 = trk.nearest3_64(p)
        assert np.all((b64 == 0) | (b64 > 1e-20)), (name, P)          # float32 denormals never decide a result
        b32 = trk.nearest3_32(p) if P <= trk.SMALL else None
        if b32 is not None:
            assert np.all((b32 == 0) | (b32 > 1e-20)) and np.array_equal(trk.mean3(b32), ref32)
        ref64 = trk.mean3(b64)
        pos = ref64 > 0
        assert np.all(ref32[~pos] == 0)
        err = float(np.max(np.abs(ref32[pos].astype(np.float64) - ref64[pos]) / ref64[pos])) if pos.any() else 0.0
        print(f"\n{name} P={p.shape[0]}: worst relative error of brute32 against brute64 {err:.3g}")
        worst = max(worst, err)
    print(f"\nworst over the GPU tests' inputs {worst:.3g}; KNN_MEASURED {trk.KNN_MEASURED:.3g}")
    assert 0.5 * trk.KNN_MEASURED <= worst <= trk.KNN_MEASURED
    assert trk.KNN_MEASURED <= 1e-6
