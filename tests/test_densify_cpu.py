"""CPU tests of the densification kernels (densification_stats_, densify_plan, densify_tensors, densify_and_prune, _C.densify_scan,
_C.densify_apply; include/stp_raster.h: stp_densify_stats / _plan / _scratch_bytes / _scan / _apply): the public names, the C ABI's
declarations, exports and argument validation (which runs before any launch, so without a GPU), what the functions refuse, the yardstick
tests/torch_ref_densify.py against a restatement of upstream's own densify_and_prune, and the MEASUREMENT that fixes the GPU tests'
tolerances: the worst error of the float32 restatement of the kernel's evaluation order against the float64 yardstick, on exactly the GPU
tests' inputs.

Measured (numpy on the CPU)                                                                   GPU bound = 4 x measured
  children's xyz,     max(0, |xyz' - ref|_2 - ulp(|ref|_inf)) / (max(s) |noise|_2)   1.6e-7  ->  CHILD_XYZ_BOUND     = 6.4e-7
  children's scaling, |scaling' - ref| / max(1, |ref|)                               1.6e-7  ->  CHILD_SCALING_BOUND = 6.4e-7
The factor 4 covers the few-ulp differences between the device's and numpy's exp / log.  The xyz error is a few float32 epsilons of the
rotation's entries and of exp; the scaling error is the rounding of exp (which log turns into an absolute error) plus the rounding of a
result of magnitude up to 6.5."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import torch_ref_densify as trd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("stp_densify_stats", "stp_densify_plan", "stp_densify_scratch_bytes", "stp_densify_scan", "stp_densify_apply")


def test_names_are_public():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import densification_stats_, densify_and_prune, densify_plan, densify_tensors   # noqa: F401
    for name in ("densification_stats_", "densify_plan", "densify_tensors", "densify_and_prune"):
        assert name in dgr.__all__
    from diff_gaussian_rasterization import _C
    assert all(callable(f) for f in (_C.densify_stats, _C.densify_plan, _C.densify_scan, _C.densify_apply))


def test_header_declares_the_five_calls():
    h = open(os.path.join(ROOT, "include", "stp_raster.h")).read()
    assert int(re.search(r"#define\s+STP_ABI_VERSION\s+(\d+)\b", h).group(1)) == 7
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"typedef\s+struct\s*\{\s*float\s+grad_threshold\s*,\s*split_size\s*,\s*min_opacity\s*,\s*max_screen_size\s*,\s*max_world_size\s*,\s*split_shrink\s*;"
                     r"\s*int32_t\s+raw\s*,\s*prune_big\s*;\s*\}\s*StpDensifyRule\s*;", h)
    assert re.search(r"typedef\s+struct\s*\{\s*const\s+float\s*\*\s*param\s*,\s*\*\s*exp_avg\s*,\s*\*\s*exp_avg_sq\s*;\s*float\s*\*\s*param_out\s*,\s*\*\s*exp_avg_out\s*,"
                     r"\s*\*\s*exp_avg_sq_out\s*;\s*int32_t\s+row\s*;\s*int32_t\s+role\s*;\s*\}\s*StpDensifyTensor\s*;", h)
    assert re.search(r"int\s+stp_densify_stats\s*\(\s*int\s+P\s*,\s*float\s*\*\s*grad_accum\s*,\s*float\s*\*\s*denom\s*,\s*float\s*\*\s*max_radii2D\s*,\s*const\s+float\s*\*\s*grad2d\s*,"
                     r"\s*int\s+grad_stride\s*,\s*const\s+void\s*\*\s*visible\s*,\s*int\s+visible_kind\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)
    assert re.search(r"int\s+stp_densify_plan\s*\(\s*int\s+P\s*,\s*const\s+float\s*\*\s*grad_accum\s*,\s*const\s+float\s*\*\s*denom\s*,\s*const\s+float\s*\*\s*scaling\s*,"
                     r"\s*const\s+float\s*\*\s*opacity\s*,\s*const\s+float\s*\*\s*max_radii2D\s*,\s*const\s+StpDensifyRule\s*\*\s*rule\s*,\s*uint8_t\s*\*\s*plan\s*,"
                     r"\s*void\s*\*\s*stream\s*\)\s*;", h)
    assert re.search(r"size_t\s+stp_densify_scratch_bytes\s*\(\s*int\s+P\s*\)\s*;", h)
    assert re.search(r"int\s+stp_densify_scan\s*\(\s*int\s+P\s*,\s*const\s+uint8_t\s*\*\s*plan\s*,\s*void\s*\*\s*scratch\s*,\s*size_t\s+scratch_bytes\s*,\s*uint32_t\s*\*\s*offsets\s*,"
                     r"\s*int64_t\s+counts\s*\[\s*3\s*\]\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)
    assert re.search(r"int\s+stp_densify_apply\s*\(\s*int\s+P\s*,\s*const\s+uint8_t\s*\*\s*plan\s*,\s*const\s+uint32_t\s*\*\s*offsets\s*,\s*const\s+int64_t\s+counts\s*\[\s*3\s*\]\s*,"
                     r"\s*int\s+n_tensors\s*,\s*const\s+StpDensifyTensor\s*\*\s*tensors\s*,\s*const\s+float\s*\*\s*noise\s*,\s*float\s+split_shrink\s*,\s*int\s+raw\s*,"
                     r"\s*void\s*\*\s*stream\s*\)\s*;", h)


def test_library_exports_the_calls_and_the_abi_stays_7():
    from diff_gaussian_rasterization import _C
    L = _C._load()
    assert L.stp_abi_version() == 7
    nm = subprocess.run(["nm", "-D", "--defined-only", _C.library_path()], capture_output=True, text=True).stdout
    for name in CALLS:
        assert hasattr(L, name) and _C._require(name) is not None
        assert re.search(r" T " + name + r"$", nm, re.M)
    host = _C._native()
    assert all(callable(getattr(host, n)) for n in ("densify_stats", "densify_plan", "densify_scan", "densify_apply"))
    assert ctypes.sizeof(_C.StpDensifyRule) == 32 and ctypes.sizeof(_C.StpDensifyTensor) == 56


def test_loader_message_for_a_library_without_the_symbols(monkeypatch):
    import types
    from diff_gaussian_rasterization import _C
    monkeypatch.setattr(_C, "_lib", types.SimpleNamespace())   # a loaded library that predates the exports
    z, plan = torch.zeros(2), torch.ones(2, dtype=torch.uint8)
    for name, call in (("stp_densify_stats", lambda: _C.densify_stats(z, z, None, torch.zeros(2, 3), torch.ones(2, dtype=torch.int32))),
                       ("stp_densify_plan", lambda: _C.densify_plan(z, z, torch.zeros(2, 3), z, None, [0.0] * 6, True, False)),
                       ("stp_densify_scan", lambda: _C.densify_scan(plan)),
                       ("stp_densify_apply", lambda: _C.densify_apply(plan, torch.zeros(6, dtype=torch.int32), (2, 0, 0), [z], [0], [None], [None], None, 1.6, True))):
        with pytest.raises(RuntimeError) as ex:
            call()
        assert str(ex.value) == f"{_C.library_path()} does not export {name} (a library built before the densification kernels): rebuild it"


def test_scratch_bytes_depend_on_P_alone():
    from diff_gaussian_rasterization import _C
    L = _C._load()
    sizes = [L.stp_densify_scratch_bytes(P) for P in (0, 1, 1365, 1366, 4097, 6_000_000, (1 << 31) // 3)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[-2] < 32768
    assert L.stp_densify_scratch_bytes(-1) == 0 and L.stp_densify_scratch_bytes((1 << 31) // 3 + 1) == 0


def test_c_abi_validates_before_any_launch():
    """The refusals come before the launch, so they need no GPU (a launch here would fail with STP_ERR_HIP, not -1); the pointers are never
    followed (they are host addresses)."""
    from diff_gaussian_rasterization import _C
    L = _C._load()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    err = lambda: L.stp_last_error().decode()
    too_many = (1 << 31) // 3 + 1

    stats = lambda P=4, ga=a, de=a, mr=None, g=a, stride=3, vis=a, kind=1: L.stp_densify_stats(P, ga, de, mr, g, stride, vis, kind, None)
    assert stats(P=-1) == -1 and "stp_densify_stats" in err() and "negative P" in err()
    assert stats(P=too_many) == -1 and ">= 2^31" in err()
    for stride in (1, 4, 0):
        assert stats(stride=stride) == -1 and f"grad_stride must be 2 or 3, got {stride}" in err()
    for kind in (2, -1):
        assert stats(kind=kind) == -1 and f"unknown visible_kind {kind}" in err()
    assert stats(mr=a, kind=0) == -1 and "max_radii2D needs the radii" in err()
    for name in ("ga", "de", "g", "vis"):
        assert stats(**{name: None}) == -1 and "stp_densify_stats: null pointer" in err()
    assert stats(P=0) == 0 and stats(P=0, ga=None, de=None, g=None, vis=None, kind=0, stride=2) == 0
    assert stats(P=0, mr=a, kind=0) == -1   # (what is wrong is refused all the same)

    rule = _C.StpDensifyRule(0.0002, 0.05, 0.005, 20.0, 0.5, 1.6, 1, 1)
    rp = ctypes.addressof(rule)
    plan = lambda P=4, ga=a, de=a, sc=a, op=a, mr=None, r=rp, out=a: L.stp_densify_plan(P, ga, de, sc, op, mr, r, out, None)
    assert plan(P=-3) == -1 and "stp_densify_plan" in err() and "negative P" in err()
    assert plan(P=too_many) == -1 and ">= 2^31" in err()
    assert plan(r=None) == -1 and "null rule" in err()
    for name in ("ga", "de", "sc", "op", "out"):
        assert plan(**{name: None}) == -1 and "stp_densify_plan: null pointer" in err()
    assert plan(P=0) == 0 and plan(P=0, ga=None, de=None, sc=None, op=None, out=None) == 0

    counts = (ctypes.c_int64 * 3)(7, 7, 7)
    cp = ctypes.addressof(counts)
    need = L.stp_densify_scratch_bytes(4)
    scan = lambda P=4, pl=a, sc=a, nb=need, off=a, c=cp: L.stp_densify_scan(P, pl, sc, nb, off, c, None)
    assert scan(P=-1) == -1 and "stp_densify_scan" in err() and "negative P" in err()
    assert scan(P=too_many) == -1 and ">= 2^31" in err()
    assert scan(nb=need - 1) == -1 and "scratch of" in err() and scan(nb=0) == -1
    assert scan(sc=a + 2) == -1 and "not 4-byte aligned" in err()
    assert scan(c=None) == -1 and "null counts" in err()
    for name in ("pl", "sc", "off"):
        assert scan(**{name: None}) == -1 and "stp_densify_scan: null pointer" in err()
    assert list(counts) == [7, 7, 7]
    assert scan(P=0, pl=None, sc=None, nb=0, off=None) == 0 and list(counts) == [0, 0, 0]   # empty work: no launch, the counts are zero

    def table(*entries):
        t = (_C.StpDensifyTensor * len(entries))()
        for k, e in enumerate(entries):
            full = dict(param=a, exp_avg=a, exp_avg_sq=a, param_out=a, exp_avg_out=a, exp_avg_sq_out=a, row=3, role=0)
            full.update(e)
            for name, value in full.items():
                setattr(t[k], name, value)
        return t

    def apply(P=4, pl=a, off=a, c=(2, 1, 0), tensors=None, n=None, noise=a, raw=1):
        tensors = table({}) if tensors is None else tensors
        cc = (ctypes.c_int64 * 3)(*(c or (0, 0, 0)))
        return L.stp_densify_apply(P, pl, off, ctypes.addressof(cc) if c is not None else None, len(tensors) if n is None else n,
                                   ctypes.addressof(tensors) if len(tensors) else None, noise, 1.6, raw, None)

    geo = ({"role": 1}, {"role": 2}, {"role": 3, "row": 4})
    assert apply(P=-1) == -1 and "stp_densify_apply" in err() and "negative P" in err()
    assert apply(P=too_many) == -1 and ">= 2^31" in err()
    assert apply(tensors=table(*[{}] * 65)) == -1 and "at most 64" in err()
    assert apply(tensors=table(*[{}] * 64), c=(0, 0, 0)) == 0   # (64 are allowed; M = 0: nothing to write, no launch)
    assert apply(n=-1) == -1 and "negative n_tensors" in err()
    for raw in (2, -1):
        assert apply(raw=raw) == -1 and f"raw must be 0 or 1, got {raw}" in err()
    assert apply(c=None) == -1 and "null counts" in err()
    for c in ((5, 0, 0), (0, -1, 0), (0, 0, 5)):
        assert apply(c=c) == -1 and "outside [0, P]" in err()
    for row in (0, -3):
        assert apply(tensors=table({"row": row})) == -1 and f"row {row} <= 0" in err()
    assert apply(P=1 << 28, tensors=table({"row": 8})) == -1 and "P * row" in err()
    for role in (4, -1):
        assert apply(tensors=table({"role": role})) == -1 and f"unknown role {role}" in err()
    for one in ("exp_avg", "exp_avg_sq"):
        assert apply(tensors=table({one: None})) == -1 and "both be given or both be null" in err()
    for name in ("param", "param_out", "exp_avg_out", "exp_avg_sq_out"):
        assert apply(tensors=table({name: None})) == -1 and "null pointer" in err()
    assert apply(tensors=table({"param": None, "param_out": None, "exp_avg_out": None, "exp_avg_sq_out": None}), c=(0, 0, 0)) == 0   # M = 0: no pointer is needed
    for name in ("pl", "off"):
        assert apply(**{name: None}) == -1 and "stp_densify_apply: null pointer" in err()
    # a split needs exactly one tensor of each of the roles 1-3 with rows 3, 3, 4, and noise
    split = (1, 0, 2)
    needs = "a split needs exactly one tensor of each of the roles"
    assert apply(c=split) == -1 and needs in err()
    for missing in range(3):
        assert apply(c=split, tensors=table(*[g for k, g in enumerate(geo) if k != missing])) == -1 and needs in err()
    for twice in range(3):
        assert apply(c=split, tensors=table(*geo, geo[twice])) == -1 and needs in err()
    for wrong in ({"role": 1, "row": 4}, {"role": 2, "row": 1}, {"role": 3, "row": 3}):
        assert apply(c=split, tensors=table(*[wrong if g["role"] == wrong["role"] else g for g in geo])) == -1 and needs in err()
    assert apply(c=split, tensors=table(*geo), noise=None) == -1 and "null noise with nS = 2" in err()
    assert apply(c=(1, 0, 0), tensors=table({"role": 1, "row": 7}), pl=None) == -1 and "null pointer" in err()   # (without a split any rows do; refused for the plan only)
    assert apply(P=0, c=(0, 0, 0), pl=None, off=None, noise=None) == 0
    assert all(x == 0.0 for x in buf)


def test_cpu_tensors_have_no_path():
    import diff_gaussian_rasterization as dgr
    d = {k: torch.from_numpy(v) for k, v in trd.model_inputs(8).items()}
    radii = torch.ones(8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.densification_stats_(d["accum"], d["denom"], d["max_radii2D"], torch.zeros(8, 3), radii)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.densify_plan(d["accum"], d["denom"], d["scaling"], d["opacity"], **trd.RULE)
    plan = torch.ones(8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.densify_tensors(plan, [d["xyz"]])
    params = [torch.nn.Parameter(d[name].clone()) for name, _ in trd.GROUPS]
    opt = torch.optim.Adam([{"params": [p], "lr": 0.01, "name": name} for p, (name, _) in zip(params, trd.GROUPS)], lr=0.0, eps=1e-15)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.densify_and_prune(opt, plan)
    assert all(g["params"][0] is p for g, p in zip(opt.param_groups, params))   # a refused call has replaced nothing
    assert torch.equal(d["denom"], torch.from_numpy(trd.model_inputs(8)["denom"]))


def test_refusals_name_the_argument():
    """What is wrong with the tensors themselves is refused before where they live is looked at: every refusal can be met without a GPU."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    z, g, radii = torch.zeros(4), torch.zeros(4, 3), torch.ones(4, dtype=torch.int32)
    for args, what in (((z.double(), z, None, g, radii), "xyz_gradient_accum: expected float32"), ((z, z, None, g.half(), radii), "grad2d: expected float32"),
                       ((z, z, None, torch.zeros(4, 4), radii), r"grad2d must be \(P, 3\) or \(P, 2\)"), ((z, z[:3], None, g, radii), "denom has 3 rows, expected 4"),
                       ((z.reshape(2, 2), z, None, g, radii), r"xyz_gradient_accum must be \(n,\) or \(n, 1\)"), ((z, z, z[:2], g, radii), "max_radii2D has 2 rows"),
                       ((z, z, None, g, radii.float()), "radii must be int32"), ((z, z, None, g, radii[:3]), "radii has 3 elements, expected 4"),
                       ((z, z, z, g, radii > 0), "max_radii2D needs the forward's int32 radii")):
        with pytest.raises((RuntimeError, ValueError), match=what):
            dgr.densification_stats_(*args)
    s = torch.zeros(4, 3)
    for args, what in (((z, z, s.double(), z), "scaling: expected float32"), ((z, z, torch.zeros(4, 2), z), r"scaling must be \(P, 3\)"),
                       ((z, z[:1], s, z), "denom has 1 rows, expected 4"), ((z, z, s, z.reshape(2, 2)), r"opacity must be \(n,\) or \(n, 1\)"),
                       ((z, z, s, z, z.double()), "max_radii2D: expected float32")):
        with pytest.raises((RuntimeError, ValueError), match=what):
            dgr.densify_plan(*args, grad_threshold=0.0002, extent=5.0)
    with pytest.raises(TypeError):
        dgr.densify_plan(z, z, s, z)   # grad_threshold and extent have no default
    with pytest.raises(RuntimeError, match="plan: expected uint8"):
        _C.densify_scan(torch.ones(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"plan must be \(P,\)"):
        _C.densify_scan(torch.ones(4, 1, dtype=torch.uint8))
    plan, off = torch.ones(4, dtype=torch.uint8), torch.zeros(12, dtype=torch.int32)
    apply = lambda tensors, roles=None, ms=None, vs=None, counts=(4, 0, 0), noise=None, offsets=off: _C.densify_apply(
        plan, offsets, counts, tensors, roles or [0] * len(tensors), ms or [None] * len(tensors), vs or [None] * len(tensors), noise, 1.6, True)
    for kwargs, what in ((dict(tensors=[s.double()]), "tensor 0: expected float32"), (dict(tensors=[s[:3]]), "tensor 0 must have 4 rows"),
                         (dict(tensors=[s], roles=[5]), "tensor 0: unknown role 5"), (dict(tensors=[s], ms=[s]), "both be given or both be None"),
                         (dict(tensors=[s], ms=[s], vs=[z]), "a moment has shape"), (dict(tensors=[s], counts=(5, 0, 0)), r"counts\[0\] = 5 outside"),
                         (dict(tensors=[s], counts=(2, 0, 1)), "nS = 1 needs noise"), (dict(tensors=[s], counts=(2, 0, 1), noise=torch.zeros(3, 3)), r"noise must be \(2, 3\)"),
                         (dict(tensors=[s], offsets=off[:5]), r"offsets: expected an int32 \(3 P,\)"), (dict(tensors=[s] * 65), "at most 64")):
        with pytest.raises((RuntimeError, ValueError), match=what):
            apply(**kwargs)
    with pytest.raises(KeyError):
        dgr.densify_tensors(plan, [s], roles=["position"])
    opt = torch.optim.Adam([{"params": [torch.nn.Parameter(s.clone())], "lr": 0.01}], lr=0.0)
    with pytest.raises(ValueError, match="carry a \"name\""):
        dgr.densify_and_prune(opt, plan)


def test_yardstick_pins():
    # statistics: a 3-4-5 triangle, an invisible NaN row, the radius maximum
    accum, denom, mr = trd.stats([1.0, 2.0, 3.0], [0.0, 1.0, 2.0], [5.0, 5.0, 5.0], np.float32([[3, 4, 99], [np.nan, 1, 0], [0, 0, 0]]), np.int32([7, 0, 2]))
    assert accum.tolist() == [6.0, 2.0, 3.0] and denom.tolist() == [1.0, 1.0, 3.0] and mr.tolist() == [7.0, 5.0, 5.0]
    assert trd.stats([0.0], [0.0], None, np.float32([[3, 4]]), np.array([True]))[0].tolist() == [5.0]
    # the plan, not raw: keep / clone / split / low opacity / too large in the world / too large on screen / denom == 0 / split children too large
    rule = dict(grad_threshold=0.25, percent_dense=0.5, extent=2.0, min_opacity=0.125, raw=False)   # split_size 1, max_world_size 0.2
    sc = np.float32([[.1, .1, .1], [.1, .1, .1], [.1, 2, .1], [.1, .1, .1], [.1, .1, .1], [.1, .1, .1], [.1, .1, .1], [.1, 2, .1]])
    accum, denom = np.float32([0, 1, 1, 1, 1, 0, 5, 1]), np.float32([1, 1, 1, 1, 1, 1, 0, 1])
    o, mr = np.float32([.5, .5, .5, .1, .5, .5, .5, .5]), np.float32([0, 0, 0, 0, 0, 30, 0, 0])
    assert trd.plan(accum, denom, sc, o, **rule).tolist() == [1, 3, 4, 0, 3, 1, 1, 4]
    sc[4] = 0.3
    assert trd.plan(accum, denom, sc, o, mr, max_screen_size=20, **rule).tolist() == [1, 3, 0, 0, 0, 0, 1, 0]
    # apply: the order K, C, first children, second children; zero moments but for K
    p = np.uint8([1, 3, 4, 0, 7])
    t = np.arange(5, dtype=np.float32)[:, None] * np.ones((1, 3), np.float32)
    q = np.float32([[2, 0, 0, 0]] * 5)
    noise = np.float32([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]])
    (xyz, sca, rot), (m, _, _), _ = trd.apply(p, [t, np.log(t + 1), q], [1, 2, 3], [t + 10, None, None], [t + 20, None, None], noise)
    assert xyz[:5, 0].tolist() == [0, 1, 4, 1, 4] and m[:, 0].tolist() == [10, 11, 14, 0, 0, 0, 0, 0, 0] and rot.shape == (9, 4)
    assert np.allclose(xyz[5:], [[2 + 3, 2, 2], [4, 4 + 5, 4], [2, 2, 2 + 3], [4 + 5, 4 + 5, 4 + 5]], rtol=1e-6)   # identity rotation: xyz + s * noise
    assert np.allclose(np.exp(sca[5:]), np.float32([[3] * 3, [5] * 3] * 2) / 1.6, rtol=1e-6)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_yardstick_is_upstreams_densify_and_prune(seed):
    """max_radii2D=None: plan() + apply() leave the rows, in the order, with the moments of upstream's own sequence."""
    d = trd.model_inputs(257, seed)
    plan = trd.model_plan(d)
    K, C, S = trd.plan_rows(plan)
    assert min(K.size, C.size, S.size, int((plan == 0).sum())) > 0 and int(((plan & 1) == 0).sum()) > S.size   # keep, clone, split and prune are all present
    noise = trd.split_noise(d["noise"], S)
    names = [n for n, _ in trd.GROUPS]
    roles = [trd.ROLES.get(n, 0) for n in names]
    out_t, out_m, out_v = trd.apply(plan, [d[n] for n in names], roles, [d["m_" + n] for n in names], [d["v_" + n] for n in names], noise)
    for dtype in (torch.float64, torch.float32):
        tt = {n: torch.from_numpy(d[n]).to(dtype) for n in names}
        mm = {n: torch.from_numpy(d["m_" + n]).to(dtype) for n in names}
        vv = {n: torch.from_numpy(d["v_" + n]).to(dtype) for n in names}
        ut, um, uv = trd.upstream_densify_and_prune(tt, mm, vv, d["accum"], d["denom"], d["noise"], **trd.RULE)
        first_child = K.size + C.size
        for n, t, m, v in zip(names, out_t, out_m, out_v):
            assert tuple(ut[n].shape) == t.shape == (K.size + C.size + 2 * S.size,) + d[n].shape[1:]
            got = ut[n].double().numpy()
            if n in ("xyz", "scaling"):
                assert np.array_equal(got[:first_child], t[:first_child])
                assert np.allclose(got[first_child:], t[first_child:], rtol=1e-12 if dtype == torch.float64 else 2e-5, atol=1e-12 if dtype == torch.float64 else 2e-5)
            else:
                assert np.array_equal(got, t)
            assert np.array_equal(um[n].double().numpy(), m) and np.array_equal(uv[n].double().numpy(), v)


def test_inputs_keep_their_distance_from_the_thresholds():
    """The condition under which the device's exp cannot flip a decision: every compared value is at least MARGIN (relative) from its threshold,
    with and without max_radii2D, for every size the GPU tests use."""
    for P in trd.SIZES:
        d = trd.model_inputs(P)
        assert trd.plan_margins(d["accum"], d["denom"], d["scaling"], d["opacity"], d["max_radii2D"], **trd.RULE) >= trd.MARGIN
        if P >= 63:
            plan = trd.model_plan(d)
            assert set(np.unique(plan).tolist()) >= {0, 1, 3, 4} and (d["denom"] == 0).any() and np.all(d["accum"][d["denom"] == 0] == 0)
            assert (trd.model_plan(d, with_radii=True) != plan).any()


def test_measured_tolerance_of_the_children():
    worst_x = worst_s = 0.0
    for raw in (True, False):
        for P in trd.SIZES:
            d = trd.model_inputs(P)
            S = trd.plan_rows(trd.model_plan(d))[2]
            scaling = d["scaling"][S] if raw else np.exp(d["scaling"][S].astype(np.float64)).astype(np.float32)
            noise = d["noise"][:2 * S.size]
            got = trd.children_kernel_order(d["xyz"][S], scaling, d["rotation"][S], noise, raw=raw)
            ex, es = trd.child_errors(*got, d["xyz"][S], scaling, d["rotation"][S], noise, raw=raw)
            worst_x, worst_s = max(worst_x, ex), max(worst_s, es)
    print(f"\nchildren restatement: worst xyz ratio {worst_x:.3g} (GPU bound {trd.CHILD_XYZ_BOUND:.3g}), worst scaling ratio {worst_s:.3g} (GPU bound {trd.CHILD_SCALING_BOUND:.3g})")
    assert 0.5 * trd.CHILD_XYZ_MEASURED <= worst_x <= trd.CHILD_XYZ_MEASURED
    assert 0.5 * trd.CHILD_SCALING_MEASURED <= worst_s <= trd.CHILD_SCALING_MEASURED
    assert trd.CHILD_XYZ_BOUND == 4 * trd.CHILD_XYZ_MEASURED and trd.CHILD_SCALING_BOUND == 4 * trd.CHILD_SCALING_MEASURED
