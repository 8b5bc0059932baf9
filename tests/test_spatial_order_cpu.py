"""CPU tests of the spatial order and the gather (spatial_order, gather_tensors, reorder_gaussians_; include/stp_raster.h:
stp_spatial_order_scratch_bytes, stp_spatial_order, stp_gather_rows): the public names, the C ABI's declarations, exports and argument
validation (which runs before any launch, so without a GPU), what the Python functions refuse before they look at the device, and hand pins
of the yardstick tests/torch_ref_spatial_order.py, which the GPU tests compare with bit for bit (integers: there is no tolerance)."""
import ctypes
import itertools
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import torch_ref_knn as trk
import torch_ref_spatial_order as tso

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
EXPORTS = ("stp_spatial_order_scratch_bytes", "stp_spatial_order", "stp_gather_rows")


def test_names_are_public():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    for name in ("spatial_order", "gather_tensors", "reorder_gaussians_"):
        assert name in dgr.__all__ and callable(getattr(dgr, name))
    assert callable(_C.spatial_order) and callable(_C.gather_rows) and callable(_C.spatial_order_scratch_bytes)


def test_header_declares_the_three_calls_and_the_abi_stays_7():
    h = open(os.path.join(ROOT, "include", "stp_raster.h")).read()
    assert int(re.search(r"#define\s+STP_ABI_VERSION\s+(\d+)\b", h).group(1)) == 7
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"size_t\s+stp_spatial_order_scratch_bytes\s*\(\s*int\s+P\s*\)\s*;", h)
    assert re.search(r"int\s+stp_spatial_order\s*\(\s*int\s+P\s*,\s*const\s+float\s*\*\s*xyz\s*,\s*void\s*\*\s*scratch\s*,\s*size_t\s+scratch_bytes\s*,"
                     r"\s*int32_t\s*\*\s*order\s*,\s*uint32_t\s*\*\s*codes\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)
    assert re.search(r"int\s+stp_gather_rows\s*\(\s*int\s+P\s*,\s*int\s+M\s*,\s*const\s+int32_t\s*\*\s*index\s*,\s*int\s+n_tensors\s*,"
                     r"\s*const\s+StpGatherTensor\s*\*\s*tensors\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)
    assert re.search(r"typedef\s+StpDensifyTensor\s+StpGatherTensor\s*;", h)


def test_library_and_its_fma_twin_export_the_calls():
    from diff_gaussian_rasterization import _C
    L = _C._load()
    assert L.stp_abi_version() == 7
    for path in (_C.library_path(), os.path.join(os.path.dirname(_C.library_path()), "libstp_raster_fma.so")):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        for name in EXPORTS:
            assert re.search(r" T " + name + r"$", nm, re.M), (path, name)
    for name in EXPORTS:
        assert hasattr(L, name) and _C._require(name) is not None
    assert callable(_C._native().spatial_order) and callable(_C._native().gather_rows)


def test_export_lines_are_optional_and_the_loader_names_the_feature(monkeypatch):
    from diff_gaussian_rasterization import _C
    table = open(os.path.join(ROOT, "stopthepop-rasterization_amd", "csrc", "host", "stp_exports.h")).read()
    for name in EXPORTS:
        assert re.search(r"X\(" + name[len("stp_"):] + r", false, \"the spatial order kernels\"\)", table), name
        assert _C._SYMBOL_FEATURE[name] == "the spatial order kernels"
    monkeypatch.setattr(_C, "_lib", types.SimpleNamespace())   # a loaded library that predates the exports
    idx = torch.zeros(8, dtype=torch.int32)
    for name, call in (("stp_spatial_order", lambda: _C.spatial_order(torch.zeros(8, 3))), ("stp_spatial_order_scratch_bytes", lambda: _C.spatial_order_scratch_bytes(8)),
                       ("stp_gather_rows", lambda: _C.gather_rows(idx, [torch.zeros(8, 3)], [None], [None]))):
        with pytest.raises(RuntimeError) as ex:
            call()
        assert str(ex.value) == f"{_C.library_path()} does not export {name} (a library built before the spatial order kernels): rebuild it"


def test_spatial_order_validates_before_any_launch():
    """The refusals come before the launch, so they need no GPU (a launch here would fail with STP_ERR_HIP, not -1); the pointers are never
    followed (they are host addresses)."""
    from diff_gaussian_rasterization import _C
    L = _C._load()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a16 = (a + 15) & ~15
    err = lambda: L.stp_last_error().decode()
    big = 1 << 40   # (a size only: nothing is read or written through `scratch`)
    call = lambda P=8, xyz=a, scratch=a16, nbytes=big, order=a, codes=a: L.stp_spatial_order(P, xyz, scratch, nbytes, order, codes, None)
    for P in (-1, -(2 ** 31)):
        assert call(P=P) == -1 and "stp_spatial_order: negative P" in err()
    for name in ("xyz", "order", "scratch"):
        assert call(**{name: None}) == -1 and f"stp_spatial_order: null pointer ({name})" in err()
    for P in (1, 8):   # (P >= 1 is accepted: "at least 4 points" is the knn call's own rule)
        need = L.stp_spatial_order_scratch_bytes(P)
        assert need > 0
        for nbytes in (0, need - 1):
            assert call(P=P, nbytes=nbytes) == -1 and "stp_spatial_order: scratch of " in err() and f"stp_spatial_order_scratch_bytes(P) = {need}" in err()
        assert call(P=P, scratch=a16 + 4) == -1 and "stp_spatial_order: scratch is not 16-byte aligned" in err()
    assert call(P=0) == 0 and call(P=0, xyz=None, scratch=None, nbytes=0, order=None, codes=None) == 0   # empty work: no launch, 0
    assert all(x == 0.0 for x in buf)


def _entry(_C, param, out, row=3, m=None, v=None, mo=None, vo=None, role=0):
    return _C.StpGatherTensor(param, m, v, out, mo, vo, row, role)


def test_gather_rows_validates_before_any_launch():
    from diff_gaussian_rasterization import _C
    L = _C._load()
    assert ctypes.sizeof(_C.StpGatherTensor) == 6 * ctypes.sizeof(ctypes.c_void_p) + 8
    buf = (ctypes.c_float * 4096)()
    a = ctypes.addressof(buf)
    src, m, v, dst, mo, vo, idx = (a + k * 2048 for k in range(7))   # seven areas of 2048 bytes: 8 rows of 48 floats are 1536
    err = lambda: L.stp_last_error().decode()
    table = lambda *entries: (_C.StpGatherTensor * len(entries))(*entries)
    good = table(_entry(_C, src, dst))
    call = lambda P=8, M=8, index=idx, n=1, t=good: L.stp_gather_rows(P, M, index, n, t, None)
    assert call(P=-1) == -1 and "stp_gather_rows: negative P" in err()
    assert call(M=-1) == -1 and "stp_gather_rows: negative M" in err()
    assert call(n=-1) == -1 and "stp_gather_rows: negative n_tensors" in err()
    assert call(t=None) == -1 and "stp_gather_rows: null tensor table" in err()
    assert call(n=65, t=table(*[_entry(_C, src, dst)] * 65)) == -1 and "at most 64" in err()
    assert call(index=None) == -1 and "stp_gather_rows: null pointer (index)" in err()
    for row in (0, -3):
        assert call(t=table(_entry(_C, src, dst, row=row))) == -1 and "stp_gather_rows: tensor 0: row" in err() and "<= 0" in err()
    assert call(t=table(_entry(_C, None, dst))) == -1 and "stp_gather_rows: tensor 0: null pointer" in err()
    assert call(t=table(_entry(_C, src, None))) == -1 and "stp_gather_rows: tensor 0: null pointer" in err()
    assert call(n=2, t=table(_entry(_C, src, dst), _entry(_C, m, None))) == -1 and "stp_gather_rows: tensor 1: null pointer" in err()
    assert call(t=table(_entry(_C, src, dst, role=1))) == -1 and "stp_gather_rows: tensor 0: unknown role 1" in err()
    assert call(t=table(_entry(_C, src, dst, m=m))) == -1 and "exp_avg and exp_avg_sq must both be given or both be null" in err()
    assert call(t=table(_entry(_C, src, dst, v=v))) == -1 and "exp_avg and exp_avg_sq must both be given or both be null" in err()
    assert call(t=table(_entry(_C, src, dst, m=m, v=v, mo=mo))) == -1 and "null pointer (moment output)" in err()
    assert call(t=table(_entry(_C, src, dst, m=m, v=v, vo=vo))) == -1 and "null pointer (moment output)" in err()
    # rows * row >= 2^31, over the output rows and over the source rows
    assert call(P=8, M=2 ** 29, t=table(_entry(_C, src, dst, row=4))) == -1 and "max(P, M) * row = 2147483648 >= 2^31" in err()
    assert call(P=2 ** 29, M=8, t=table(_entry(_C, src, dst, row=4))) == -1 and "max(P, M) * row = 2147483648 >= 2^31" in err()
    assert call(P=0, M=8) == -1 and "stp_gather_rows: 8 rows from P = 0 rows" in err()
    # out of place only: an output that overlaps ANY input of the call
    assert call(t=table(_entry(_C, src, src))) == -1 and "tensor 0: param_out overlaps param of tensor 0" in err() and "out of place only" in err()
    assert call(t=table(_entry(_C, src, src + 8 * 3 * 4 - 4))) == -1 and "param_out overlaps param of tensor 0" in err()      # by the last float
    assert call(t=table(_entry(_C, src, dst, m=m, v=v, mo=v, vo=vo))) == -1 and "tensor 0: exp_avg_out overlaps exp_avg_sq of tensor 0" in err()
    assert call(n=2, t=table(_entry(_C, src, dst), _entry(_C, m, src))) == -1 and "tensor 1: param_out overlaps param of tensor 0" in err()
    assert call(t=table(_entry(_C, src, idx))) == -1 and "tensor 0: param_out overlaps the index" in err()
    # empty work: no launch, 0 -- and the table is still looked at
    assert call(M=0) == 0 and call(M=0, index=None) == 0 and call(n=0, t=None) == 0 and call(P=0, M=0) == 0
    assert call(M=0, t=table(_entry(_C, None, None))) == 0
    assert call(M=0, t=table(_entry(_C, src, dst, row=0))) == -1 and "row 0 <= 0" in err()
    assert all(x == 0.0 for x in buf)


def test_scratch_bytes_is_monotone_and_does_not_overflow():
    from diff_gaussian_rasterization import _C
    f = _C.spatial_order_scratch_bytes
    assert f(0) == 0 and f(-1) == 0 and f(-(2 ** 31)) == 0
    at = {P: f(P) for P in (1, 4, 2 ** 16 + 1, INT_MAX)}
    # the carve: two key and two value buffers (4 x 4 bytes per point), the 3 x 1024 splitters, rocPRIM's temporary storage
    for P, got in at.items():
        own = 16 * P + 3 * 1024 * 4
        assert own <= got <= own + own // 8 + (1 << 20), (P, got, own)
        assert got < _C.knn_scratch_bytes(max(P, 4))          # (without the search's records and boxes)
    assert at[INT_MAX] > 2 ** 35 and at[INT_MAX] < 2 ** 36   # 16 bytes per point of 2^31: 32 GiB and a little, no wrap-around
    sweep = sorted(set([1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000, 4095, 4096, 4097, 2 ** 16 - 1, 2 ** 16, 2 ** 16 + 1, 10 ** 5, 10 ** 6, 6 * 10 ** 6,
                        2 ** 24, 2 ** 24 + 1, 2 ** 30, 2 ** 30 + 1, INT_MAX - 1, INT_MAX] + [int(1.37 ** k) for k in range(4, 68)]))
    sizes = [f(P) for P in sweep]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), list(zip(sweep, sizes))
    assert all(s % 256 == 0 and s > 0 for s in sizes)
    assert f(10 ** 6) == f(10 ** 6)   # a function of P alone


def test_python_refusals_come_before_the_device():
    """What is wrong with a tensor itself is refused before where it lives is looked at: every refusal can be met without a GPU."""
    import diff_gaussian_rasterization as dgr
    p = torch.zeros(8, 3)
    for bad, what in ((p.double(), "xyz: expected float32"), (p.half(), "xyz: expected float32"), (p.int(), "xyz: expected float32"),
                      (torch.zeros(8, 4), r"xyz must be \(P, 3\)"), (torch.zeros(8), r"xyz must be \(P, 3\)"), (torch.zeros(2, 8, 3), r"xyz must be \(P, 3\)"),
                      (p, "no CPU path"), (p[:1], "no CPU path"), (p[:0], "no CPU path"), (torch.zeros(3, 8).t(), "no CPU path"),
                      (p.clone().requires_grad_(True), "no CPU path")):
        for codes in (False, True):
            with pytest.raises(RuntimeError, match=what):
                dgr.spatial_order(bad, codes)
    with pytest.raises(RuntimeError, match="xyz: expected float32"):   # (the dtype comes first, then the shape)
        dgr.spatial_order(torch.zeros(2, 4, dtype=torch.float64))
    idx = torch.zeros(8, dtype=torch.int32)
    g = dgr.gather_tensors
    for call, what in ((lambda: g(idx.float(), [p]), "index: expected an int32 tensor"), (lambda: g(idx.view(2, 4), [p]), r"index must be \(M,\)"),
                       (lambda: g(idx, [p.double()]), "tensor 0: expected float32 or int32"), (lambda: g(idx, [p, p.half()]), "tensor 1: expected float32 or int32"),
                       (lambda: g(idx, [p, torch.zeros(7, 3)]), "tensor 1 must have 8 rows"), (lambda: g(idx, [torch.zeros(8, 0)]), "rows without elements"),
                       (lambda: g(idx, [p], [p], [None]), "exp_avg and exp_avg_sq must both be given or both be None"),
                       (lambda: g(idx, [p], [p.int()], [p]), "tensor 0: moments: expected"), (lambda: g(idx, [p], [torch.zeros(8, 4)], [p]), "a moment has shape"),
                       (lambda: g(idx, [p], [p, p], [p, p]), "one entry per tensor"), (lambda: g(idx, [torch.zeros(0, 3)]), "8 rows from tensors without rows"),
                       (lambda: g(idx, [p] * 65), "at most 64"),
                       (lambda: g(idx, [p]), "no CPU path"), (lambda: g(idx.long(), [p.int()], None, None), "no CPU path"), (lambda: g(idx[:0], [p], [p], [p]), "no CPU path")):
        with pytest.raises(RuntimeError, match=what):
            call()
    params = {n: torch.nn.Parameter(torch.zeros(8, w)) for n, w in (("xyz", 3), ("opacity", 1))}
    opt = torch.optim.Adam([{"params": [params[n]], "name": n} for n in params], lr=1e-3)
    with pytest.raises(ValueError, match="exactly one group named 'means'"):
        dgr.reorder_gaussians_(opt, xyz="means")
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.reorder_gaussians_(opt)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.reorder_gaussians_(opt, idx, extra=[torch.zeros(8)])
    with pytest.raises(ValueError, match="every group must hold one tensor and carry a \"name\""):
        dgr.reorder_gaussians_(torch.optim.Adam(list(params.values()), lr=1e-3))
    assert all(p_ is opt.param_groups[k]["params"][0] for k, p_ in enumerate(params.values()))   # (a refused call has changed nothing)


CORNERS = np.float32([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)])   # row k = the corner with x + 2 y + 4 z = k


def test_yardstick_pins():
    # the eight corners of the unit cube: per axis four keys of 0 and four of 1, so a 0 lies in cell 511 and a 1 in cell 1023; the low nine
    # bits of every axis are set in every code, and bit 9 of x, y, z is bit 27, 28, 29: code = 2^27 - 1 + (x + 2 y + 4 z) 2^27
    want_codes = [k * 2 ** 27 - 1 for k in range(1, 9)]
    some = [list(range(8)), list(range(7, -1, -1)), [3, 6, 0, 5, 1, 7, 2, 4]] + [list(np.random.default_rng(s).permutation(8)) for s in range(20)]
    for perm in some:
        p = CORNERS[perm]
        order, codes = tso.order_and_codes(p)
        assert order.dtype == np.int32 and codes.dtype == np.uint32
        assert codes.tolist() == want_codes, perm
        assert (p[order] @ np.float32([1, 2, 4])).tolist() == list(range(8)), perm
        assert tso.codes_of(p).tolist() == [want_codes[k] for k in perm]
    # -0 sorts below +0 and the infinities sit at the ends; the two constant axes share one cell and decide nothing
    assert tso.order_and_codes(tso.SIGNS)[0].tolist() == [3, 1, 0, 4, 2]
    assert tso.ordered_bits(np.float32([-np.inf, -1, -0.0, 0.0, 1, np.inf])).tolist() == sorted(tso.ordered_bits(np.float32([-np.inf, -1, -0.0, 0.0, 1, np.inf])).tolist())
    assert tso.ordered_bits(np.float32([-0.0]))[0] == 0x7FFFFFFF and tso.ordered_bits(np.float32([0.0]))[0] == 0x80000000
    # a tie stays in index order
    assert tso.order_and_codes(np.float32([[1, 2, 3], [1, 2, 3], [0, 0, 0]]))[0].tolist() == [2, 0, 1]
    # one point: every splitter is its own key, cell 1023 on every axis
    order, codes = tso.order_and_codes(np.float32([[5, -7, 0.25]]))
    assert order.tolist() == [0] and codes.tolist() == [2 ** 30 - 1]
    assert tso.spread10(np.uint32([1023, 1, 512, 0b1000000001])).tolist() == [0x09249249, 1, 1 << 27, (1 << 27) | 1]


def test_codes_depend_on_the_multiset_only():
    for name in ("uniform", "dups", "lattice"):
        p = trk.CLOUDS[name](trk.SMALL)
        perm = np.random.default_rng(11).permutation(p.shape[0])
        assert np.array_equal(tso.codes_of(p)[perm], tso.codes_of(p[perm]))
        assert np.array_equal(tso.order_and_codes(p)[1], tso.order_and_codes(p[perm])[1])


def test_yardstick_is_idempotent_on_every_cloud():
    """order(p[order(p)]) is the identity: the codes depend on the multiset only, and the sort is stable."""
    for name, P in trk.CASES:
        p = trk.CLOUDS[name](P)
        order, codes = tso.order_and_codes(p)
        assert sorted(order.tolist()) == list(range(p.shape[0])) and np.all(codes[1:] >= codes[:-1]) and int(codes.max()) < 2 ** 30
        again, codes2 = tso.order_and_codes(p[order])
        assert np.array_equal(again, np.arange(p.shape[0], dtype=np.int32)) and np.array_equal(codes2, codes), (name, P)
    # the dups cloud exercises the stable tie: 300 distinct codes over its 925 points, the longest run of equal codes 5
    order, codes = tso.order_and_codes(trk.dups())
    runs = [len(list(g)) for _, g in itertools.groupby(codes.tolist())]
    assert trk.dups().shape[0] == 925 and len(runs) == 300 and max(runs) == 5
    for s in range(1, 925):
        assert codes[s] > codes[s - 1] or order[s] > order[s - 1]


def test_inputs_cover_what_the_gpu_tests_need():
    assert tso.SIZES == (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 775, 20011) and tso.CROSSING == 70001 > 2 ** 16
    assert set(name for name, _ in tso.CASES) == set(trk.CLOUDS) == {"uniform", "clustered", "plane", "line", "lattice", "dups", "outlier"}
    assert ("clustered", 20011) in tso.CASES and ("clustered", 70001) in tso.CASES
    # below 1024 points the splitters repeat, so cells stay empty; from 1024 on a uniform cloud fills all of them on every axis
    for P, full in ((1023, False), (1024, True), (1025, True)):
        codes = tso.codes_of(trk.uniform(P))
        cells_x = set(int(sum(((c >> (3 * b)) & 1) << b for b in range(10))) for c in codes.tolist())
        assert (len(cells_x) == 1024) == full, (P, len(cells_x))
