"""CPU tests of the fused 3DGS-MCMC relocation and growth (mcmc_relocation_plan, mcmc_relocate_tensors_, mcmc_relocate_, mcmc_add_plan,
mcmc_add_tensors, mcmc_add_new; include/stp_raster.h: stp_mcmc_relocate_scratch_bytes, stp_mcmc_sample, stp_mcmc_relocate_apply,
stp_mcmc_add_apply): the public names and defaults, the C ABI's declarations, exports and argument validation (which runs before any launch, so
without a GPU), what the functions refuse, the sanity of the yardstick tests/torch_ref_mcmc_relocate.py, and the MEASUREMENT that fixes the GPU
tests' tolerances: the worst error of the float32 restatement of the kernel's raw path against the float64 yardstick, on exactly the GPU tests'
inputs (the figures are in the yardstick's docstring)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import torch_ref_mcmc_relocate as trr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("stp_mcmc_relocate_scratch_bytes", "stp_mcmc_sample", "stp_mcmc_relocate_apply", "stp_mcmc_add_apply")
PUBLIC = ("mcmc_relocation_plan", "mcmc_relocate_tensors_", "mcmc_relocate_", "mcmc_add_plan", "mcmc_add_tensors", "mcmc_add_new")
FEATURE = "the 3DGS-MCMC relocation kernels"


def test_names_and_defaults_are_public():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    for name in PUBLIC:
        assert name in dgr.__all__ and callable(getattr(dgr, name))
    defaults = lambda f: {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults(dgr.mcmc_relocation_plan) == {"min_opacity": 0.005, "raw": True, "return_weights": False}
    assert defaults(dgr.mcmc_relocate_tensors_) == {"exp_avgs": None, "exp_avg_sqs": None, "min_opacity": 0.005, "raw": True, "reset_dead_moments": False}
    assert defaults(dgr.mcmc_relocate_) == {"uniforms": None, "min_opacity": 0.005, "raw": True, "reset_dead_moments": False, "names": ("opacity", "scaling")}
    assert defaults(dgr.mcmc_add_plan) == {"raw": True}
    assert defaults(dgr.mcmc_add_tensors) == {"exp_avgs": None, "exp_avg_sqs": None, "min_opacity": 0.005, "raw": True}
    assert defaults(dgr.mcmc_add_new) == {"uniforms": None, "min_opacity": 0.005, "raw": True, "names": ("opacity", "scaling")}
    kw_only = lambda f: [k for k, p in inspect.signature(f).parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY]
    assert kw_only(dgr.mcmc_relocation_plan) == ["min_opacity", "raw", "return_weights"] and kw_only(dgr.mcmc_add_plan) == ["raw"]
    assert all(callable(f) for f in (_C.mcmc_relocate_scratch_bytes, _C.mcmc_sample, _C.mcmc_relocate_apply, _C.mcmc_add_apply))
    assert _C.MCMC_ROLES == {"plain": 0, "opacity": 1, "scaling": 2}


def test_header_declares_the_calls():
    h = open(os.path.join(ROOT, "include", "stp_raster.h")).read()
    assert int(re.search(r"#define\s+STP_ABI_VERSION\s+(\d+)\b", h).group(1)) == 7
    assert int(re.search(r"#define\s+STP_MCMC_SAMPLE_TILE\s+(\d+)\b", h).group(1)) == 2048
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    i32, ci32 = r"int32_t\s*\*\s*", r"const\s+int32_t\s*\*\s*"
    assert re.search(r"typedef\s+struct\s*\{\s*float\s*\*\s*param\s*,\s*\*\s*exp_avg\s*,\s*\*\s*exp_avg_sq\s*;\s*float\s*\*\s*param_out\s*,\s*\*\s*exp_avg_out\s*,"
                     r"\s*\*\s*exp_avg_sq_out\s*;\s*int32_t\s+row\s*;\s*int32_t\s+role\s*;\s*\}\s*StpMcmcTensor\s*;", h)
    assert re.search(r"size_t\s+stp_mcmc_relocate_scratch_bytes\s*\(\s*int\s+P\s*\)\s*;", h)
    assert re.search(r"int\s+stp_mcmc_sample\s*\(\s*int\s+P\s*,\s*const\s+float\s*\*\s*opacity\s*,\s*int\s+rule\s*,\s*float\s+min_opacity\s*,\s*int\s+raw\s*,\s*int\s+n_draws\s*,"
                     r"\s*const\s+float\s*\*\s*uniforms\s*,\s*void\s*\*\s*scratch\s*,\s*size_t\s+scratch_bytes\s*,\s*uint32_t\s*\*\s*weights\s*,\s*" + i32 + r"src\s*,\s*" + i32 +
                     r"count\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)
    assert re.search(r"int\s+stp_mcmc_relocate_apply\s*\(\s*int\s+P\s*,\s*" + ci32 + r"src\s*,\s*" + ci32 + r"count\s*,\s*int\s+n_tensors\s*,\s*const\s+StpMcmcTensor\s*\*\s*tensors\s*,"
                     r"\s*float\s+min_opacity\s*,\s*int\s+raw\s*,\s*int\s+reset_dead_moments\s*,\s*void\s*\*\s*scratch\s*,\s*size_t\s+scratch_bytes\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)
    assert re.search(r"int\s+stp_mcmc_add_apply\s*\(\s*int\s+P\s*,\s*int\s+n_new\s*,\s*" + ci32 + r"src\s*,\s*" + ci32 + r"count\s*,\s*int\s+n_tensors\s*,"
                     r"\s*const\s+StpMcmcTensor\s*\*\s*tensors\s*,\s*float\s+min_opacity\s*,\s*int\s+raw\s*,\s*void\s*\*\s*scratch\s*,\s*size_t\s+scratch_bytes\s*,"
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
    assert all(callable(getattr(host, n)) for n in ("mcmc_sample", "mcmc_relocate_apply", "mcmc_add_apply"))
    assert ctypes.sizeof(_C.StpMcmcTensor) == 56 and _C.MCMC_SAMPLE_TILE == 2048


def test_loader_message_for_a_library_without_the_symbols(monkeypatch):
    import types
    from diff_gaussian_rasterization import _C
    monkeypatch.setattr(_C, "_lib", types.SimpleNamespace())   # a loaded library that predates the exports
    z, i = torch.zeros(2), torch.zeros(2, dtype=torch.int32)
    for name, call in (("stp_mcmc_relocate_scratch_bytes", lambda: _C.mcmc_relocate_scratch_bytes(4)),
                       ("stp_mcmc_sample", lambda: _C.mcmc_sample(z, z, 0, 0.005, True, False)),
                       ("stp_mcmc_relocate_apply", lambda: _C.mcmc_relocate_apply(i, i, [z, torch.zeros(2, 3)], [1, 2], [None] * 2, [None] * 2, 0.005, True, False)),
                       ("stp_mcmc_add_apply", lambda: _C.mcmc_add_apply(i, i, [z, torch.zeros(2, 3)], [1, 2], [None] * 2, [None] * 2, 0.005, True))):
        with pytest.raises(RuntimeError) as ex:
            call()
        assert str(ex.value) == f"{_C.library_path()} does not export {name} (a library built before {FEATURE}): rebuild it"


def test_scratch_bytes_depend_on_P_alone():
    from diff_gaussian_rasterization import _C
    L = _C._load()
    tile = _C.MCMC_SAMPLE_TILE
    Ps = (0, 1, tile - 1, tile, tile + 1, 6_000_000, 1 << 28)
    sizes = [L.stp_mcmc_relocate_scratch_bytes(P) for P in Ps]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
    for P, s in zip(Ps, sizes):   # the larger of the sample's (head, tile sums, prefix: 64-bit words) and the apply's (16 bytes per row)
        need = max(8 * (4 + (P + tile - 1) // tile + P), 16 * P)
        assert need <= s < need + 256
    assert sizes[-2] == 96_000_000 and sizes[-1] == 1 << 32
    assert L.stp_mcmc_relocate_scratch_bytes((1 << 28) + 1) == 0 and L.stp_mcmc_relocate_scratch_bytes(-1) == 0
    assert _C.mcmc_relocate_scratch_bytes(4097) == L.stp_mcmc_relocate_scratch_bytes(4097)


def _table(*entries):
    from diff_gaussian_rasterization import _C
    t = (_C.StpMcmcTensor * max(len(entries), 1))()
    for k, e in enumerate(entries):
        t[k] = _C.StpMcmcTensor(*e)
    return t


def test_c_abi_validates_before_any_launch():
    """The refusals come before the launch, so they need no GPU (a launch here would fail with STP_ERR_HIP, not -1); the pointers are never
    followed (they are host addresses)."""
    from diff_gaussian_rasterization import _C
    L = _C._load()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a += -a % 16   # (16-byte aligned, inside the buffer)
    err = lambda: L.stp_last_error().decode()
    too_many = (1 << 28) + 1
    need = L.stp_mcmc_relocate_scratch_bytes(4)

    sample = lambda P=4, o=a, rule=0, raw=1, n=4, u=a, sc=a, nb=need, w=None, src=a, cnt=a: L.stp_mcmc_sample(P, o, rule, 0.005, raw, n, u, sc, nb, w, src, cnt, None)
    assert sample(P=-1) == -1 and "stp_mcmc_sample" in err() and "negative P" in err()
    assert sample(n=-1, rule=1) == -1 and "stp_mcmc_sample" in err() and "negative n_draws" in err()
    assert sample(P=too_many, n=too_many) == -1 and "stp_mcmc_sample" in err() and "> 2^28" in err()
    for raw in (2, -1):
        assert sample(raw=raw) == -1 and f"stp_mcmc_sample: raw must be 0 or 1, got {raw}" in err()
    for rule in (2, -1):
        assert sample(rule=rule) == -1 and f"stp_mcmc_sample: unknown rule {rule}" in err()
    assert sample(n=3) == -1 and "stp_mcmc_sample: rule 0 draws once per row" in err()
    assert sample(nb=need - 1) == -1 and "stp_mcmc_sample: scratch of" in err() and sample(nb=0) == -1
    assert sample(sc=a + 4) == -1 and "stp_mcmc_sample: scratch is not 16-byte aligned" in err()
    for name in ("o", "u", "sc", "src", "cnt"):
        assert sample(**{name: None}) == -1 and "stp_mcmc_sample: null pointer" in err()
    assert sample(P=0, n=3, rule=1) == -1 and "draws from P = 0 rows" in err()
    assert sample(P=0, n=0) == 0 and sample(P=0, n=0, o=None, u=None, sc=None, nb=0, src=None, cnt=None, rule=1, raw=0) == 0   # empty work: no launch
    assert sample(P=0, n=0, raw=3) == -1   # (what is wrong is refused all the same)

    good = ((a, a, a, a, a, a, 1, 1), (a, a, a, a, a, a, 3, 2), (a, None, None, a, None, None, 45, 0))
    reloc = lambda P=4, src=a, cnt=a, n=3, t=good, raw=1, sc=a, nb=need: L.stp_mcmc_relocate_apply(P, src, cnt, n, ctypes.addressof(_table(*t)) if t is not None else None,
                                                                                                  0.005, raw, 0, sc, nb, None)
    add = lambda P=4, n_new=2, src=a, cnt=a, n=3, t=good, raw=1, sc=a, nb=need: L.stp_mcmc_add_apply(P, n_new, src, cnt, n, ctypes.addressof(_table(*t)) if t is not None else None,
                                                                                                    0.005, raw, sc, nb, None)
    for who, call in (("stp_mcmc_relocate_apply", reloc), ("stp_mcmc_add_apply", add)):
        in_place = call is reloc
        assert call(P=-1) == -1 and who in err() and "negative P" in err()
        assert call(P=too_many) == -1 and who in err() and "> 2^28" in err()
        for raw in (2, -1):
            assert call(raw=raw) == -1 and f"{who}: raw must be 0 or 1, got {raw}" in err()
        assert call(nb=need - 1) == -1 and f"{who}: scratch of" in err()
        assert call(sc=a + 8) == -1 and f"{who}: scratch is not 16-byte aligned" in err()
        assert call(sc=None) == -1 and f"{who}: null pointer" in err()
        assert call(n=-1) == -1 and f"{who}: negative n_tensors" in err()
        assert call(n=65) == -1 and f"{who}: 65 tensors, at most 64" in err()
        assert call(t=None) == -1 and f"{who}: null tensor table" in err()
        assert call(cnt=None) == -1 and f"{who}: null pointer" in err()
        assert call(src=None) == -1 and f"{who}: null pointer" in err()
        bad = lambda k, **ch: tuple(tuple(ch.get(f, v) for f, v in zip(("p", "m", "v", "po", "mo", "vo", "row", "role"), e)) if j == k else e for j, e in enumerate(good))
        assert call(t=bad(2, row=0)) == -1 and f"{who}: tensor 2: row 0 <= 0" in err()
        assert call(t=bad(2, row=1 << 30)) == -1 and f"{who}: tensor 2: rows * row" in err() and ">= 2^31" in err()
        assert call(t=bad(2, role=3)) == -1 and f"{who}: tensor 2: unknown role 3" in err()
        assert call(t=bad(0, row=2)) == -1 and f"{who}: tensor 0: role 1 needs row 1, got 2" in err()
        assert call(t=bad(1, row=4)) == -1 and f"{who}: tensor 1: role 2 needs row 3, got 4" in err()
        assert call(t=bad(1, m=None)) == -1 and f"{who}: tensor 1: exp_avg and exp_avg_sq must both be given or both be null" in err()
        assert call(t=bad(2, p=None)) == -1 and f"{who}: tensor 2: null pointer" in err()
        assert call(t=bad(0, role=0)) == -1 and f"{who}: missing role 1 (opacity, row 1)" in err()
        assert call(t=bad(1, role=0, row=3)) == -1 and f"{who}: missing role 2 (scaling, row 3)" in err()
        assert call(t=bad(2, role=1, row=1)) == -1 and f"{who}: duplicated role 1 (opacity, row 1)" in err()
        assert call(t=bad(2, role=2, row=3)) == -1 and f"{who}: duplicated role 2 (scaling, row 3)" in err()
        if not in_place:
            assert call(t=bad(2, po=None)) == -1 and f"{who}: tensor 2: null pointer" in err()
            assert call(t=bad(1, mo=None)) == -1 and f"{who}: tensor 1: null pointer (moment output)" in err()
            assert call(n_new=-1) == -1 and f"{who}: negative n_new" in err()
            assert call(P=0, n_new=2, sc=None, nb=0) == -1 and "new rows from P = 0 rows" in err()
            assert call(P=0, n_new=0, src=None, cnt=None, sc=None, nb=0) == 0
        else:
            assert call(P=0, src=None, cnt=None, sc=None, nb=0) == 0   # empty work: no launch, 0
    assert all(x == 0.0 for x in buf)


def test_cpu_tensors_have_no_path():
    import diff_gaussian_rasterization as dgr
    inp = trr.model_inputs(65, True)
    tensors, roles, moments = trr.lists_of(inp)
    ms, vs = [m for m, _ in moments], [v for _, v in moments]
    keep = [t.clone() for t in tensors]
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.mcmc_relocation_plan(inp["opacity"], inp["uniforms"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.mcmc_add_plan(inp["opacity"], inp["uniforms"][:3])
    plan = (torch.full((65,), -1, dtype=torch.int32), torch.zeros(65, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.mcmc_relocate_tensors_(plan, tensors, roles, ms, vs)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.mcmc_add_tensors((plan[0][:3], plan[1]), tensors, roles, ms, vs)
    opt = torch.optim.Adam([{"params": [torch.nn.Parameter(t.clone())], "name": n} for n, t in zip(trr.NAMES, tensors)], lr=0.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.mcmc_relocate_(opt, inp["uniforms"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.mcmc_add_new(opt, 1000)
    assert all(torch.equal(a, b) for a, b in zip(keep, tensors))
    assert dgr.mcmc_add_new(opt, 65) == {} and dgr.mcmc_add_new(opt, 10) == {}   # n_new == 0: nothing is looked at


def test_refusals_name_the_argument():
    """What is wrong with the tensors themselves is refused before where they live is looked at: every refusal can be met without a GPU."""
    import diff_gaussian_rasterization as dgr
    o, u = torch.full((4,), 0.5), torch.full((4,), 0.25)
    for f, args, what in ((dgr.mcmc_relocation_plan, (o.double(), u), "mcmc_relocation_plan: opacity: expected float32"),
                          (dgr.mcmc_relocation_plan, (o, u.half()), "mcmc_relocation_plan: uniforms: expected float32"),
                          (dgr.mcmc_relocation_plan, (o.reshape(2, 2), u), r"opacity must be \(n,\) or \(n, 1\)"),
                          (dgr.mcmc_relocation_plan, (o, u[:3]), "uniforms has 3 rows, opacity has 4"),
                          (dgr.mcmc_relocation_plan, (o, u.reshape(4, 1)), r"uniforms must be \(n,\)"),
                          (dgr.mcmc_add_plan, (o.double(), u), "mcmc_add_plan: opacity: expected float32"),
                          (dgr.mcmc_add_plan, (o, u.reshape(2, 2)), r"mcmc_add_plan: uniforms must be \(n,\)"),
                          (dgr.mcmc_add_plan, (torch.zeros(0), u), "4 draws from a model without rows")):
        with pytest.raises((RuntimeError, ValueError), match=what):
            f(*args)
    src, cnt = torch.full((4,), -1, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    op, sc, xyz, sh = torch.zeros(4, 1), torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 15, 3)
    ok = ([xyz, op, sc, sh], ["plain", "opacity", "scaling", "plain"])
    for who, f in (("mcmc_relocate_tensors_", dgr.mcmc_relocate_tensors_), ("mcmc_add_tensors", dgr.mcmc_add_tensors)):
        cases = [(((src.long(), cnt),) + ok, "plan: src: expected an int32"), (((src, cnt.float()),) + ok, "plan: count: expected an int32"),
                 (((src, cnt), [xyz.double(), op, sc], ["plain", "opacity", "scaling"]), "tensor 0: expected float32 tensor"),
                 (((src, cnt), [xyz[:3], op, sc], ["plain", "opacity", "scaling"]), "tensor 0 must have 4 rows"),
                 (((src, cnt), [xyz, op, sc], ["plain", "opacity"]), "one entry per tensor"),
                 (((src, cnt), [xyz, op, sc], [0, 1, 3]), "tensor 2: unknown role 3"),
                 (((src, cnt), [xyz, sc, sc], ["plain", "opacity", "scaling"]), "tensor 1: the opacity must have 1 float per row"),
                 (((src, cnt), [xyz, op, op], ["plain", "opacity", "scaling"]), "tensor 2: the scaling must have 3 floats per row"),
                 (((src, cnt), [xyz, op, sc], ["plain", "plain", "scaling"]), "exactly one tensor must have the role opacity"),
                 (((src, cnt), [op, op, sc], ["opacity", "opacity", "scaling"]), "exactly one tensor must have the role opacity"),
                 (((src, cnt), [xyz, op, sc], ["plain", "opacity", "scaling"], [xyz, None, None], [None] * 3), "tensor 0: exp_avg and exp_avg_sq must both be given"),
                 (((src, cnt), [xyz, op, sc], ["plain", "opacity", "scaling"], [sh, None, None], [sh, None, None]), "tensor 0: a moment has shape")]
        if who == "mcmc_relocate_tensors_":
            cases += [(((src[:3], cnt),) + ok, "plan: src has 3 rows, count has 4"),
                      (((src, cnt), [torch.zeros(3, 4).t(), op, sc], ["plain", "opacity", "scaling"]), r"tensor 0 must be contiguous \(it is updated in place\)"),
                      (((src, cnt), [xyz, op, sc], ["plain", "opacity", "scaling"], [torch.zeros(3, 4).t(), None, None], [xyz, None, None]), "the moments must be contiguous")]
        for args, what in cases:
            with pytest.raises((RuntimeError, ValueError), match=who + ".*" + what):
                f(*args)
    named = lambda names: torch.optim.Adam([{"params": [torch.nn.Parameter(torch.zeros(4, 3 if n == "scaling" else 1))], "name": n} for n in names], lr=0.0)
    for f, extra in ((dgr.mcmc_relocate_, ()), (dgr.mcmc_add_new, (100,))):
        with pytest.raises(ValueError, match="every group must hold one tensor and carry a \"name\""):
            f(torch.optim.Adam([torch.nn.Parameter(torch.zeros(4, 1))], lr=0.0), *extra)
        with pytest.raises(ValueError, match="exactly one group named 'opacity' and one named 'scaling'"):
            f(named(["opacity", "xyz"]), *extra)
    with pytest.raises(ValueError, match="uniforms has 3 rows, n_new"):
        dgr.mcmc_add_new(named(["opacity", "scaling"]), 100, torch.zeros(3))


def test_yardstick_draw_on_hand_cases():
    w = torch.tensor([0, 3, 0, 1, 0])          # S = 0 3 3 4 4, total 4: t = floor(4 u)
    below_one = float(np.nextafter(np.float32(1), np.float32(0)))
    u = torch.tensor([0.0, 0.25, 0.49, 0.5, 0.74, 0.75, below_one, 1.0, 7.0, -1.0, float("nan")])
    assert trr.draw(w, u).tolist() == [1, 1, 1, 1, 1, 3, 3, 3, 3, 1, 1]
    assert trr.draw(torch.zeros(5, dtype=torch.int64), u).tolist() == [-1] * 11
    o = torch.tensor([0.5, 0.004, 0.005, float("nan"), 1.0, 2.0 ** -25, 3 * 2.0 ** -25, 0.0050001])
    assert trr.dead_rows(o, False).tolist() == [False, True, True, False, False, True, True, False]
    assert trr.relocation_weights(o, False).tolist() == [1 << 23, 0, 0, 0, 1 << 24, 0, 0, round(float(np.float32(0.0050001)) * 2 ** 24)]
    assert trr.growth_weights(o, False).tolist()[:7] == [1 << 23, round(float(np.float32(0.004)) * 2 ** 24), round(float(np.float32(0.005)) * 2 ** 24), 0, 1 << 24, 0, 2]
    src, count = trr.sample_relocation(trr.relocation_weights(o, False), trr.dead_rows(o, False), torch.tensor([0.0, 0.99, 0.999, 0.5, 0.5, 0.0, 0.4, 0.5]))
    assert src.tolist() == [-1, 4, 7, -1, -1, 0, 4, -1] and count.tolist() == [1, 0, 0, 0, 2, 0, 0, 1]   # (the weights end at 2^23, 3 * 2^23, + 83887)


def test_yardstick_frequencies_follow_the_opacities():
    """200 000 uniforms on 50 candidates: the count of candidate k is binomial(n, p_k) with p_k = o_k / sum(o) (the quantisation moves p_k by less
    than 2^-25 / o_k relative: nothing here), so |count_k / n - p_k| <= 5 sqrt(p_k (1 - p_k) / n) fails for one k in 1.7 million per candidate."""
    rng = np.random.default_rng(7)
    n = 200_000
    o = torch.from_numpy(rng.uniform(0.01, 0.99, 50).astype(np.float32))
    u = torch.from_numpy(rng.uniform(0.0, 1.0, n).astype(np.float32)).clamp(max=float(np.nextafter(np.float32(1), np.float32(0))))
    src, count = trr.sample_growth(trr.growth_weights(o, False), u)
    assert int(count.sum()) == n and int(src.min()) >= 0
    p = o.double() / o.double().sum()
    sigma = torch.sqrt(p * (1 - p) / n)
    assert bool(((count.double() / n - p).abs() <= 5 * sigma).all())


def test_generators_keep_their_guarantees():
    for raw in (False, True):
        for P in trr.SIZES[:-1]:
            inp = trr.model_inputs(P, raw)   # (asserts the exclusion band and the sources' limit itself)
            dead = trr.dead_rows(inp["opacity"], raw)
            if P >= 2:
                assert bool(dead.any()) and not bool(dead.all())
            assert float(inp["uniforms"].max()) < 1.0 and all(bool((inp["m_" + n] != 0).all()) for n in trr.NAMES)
    with pytest.raises(AssertionError, match="exclusion band"):
        trr.check_opacities(torch.tensor([0.5, 0.0050004]), False)
    with pytest.raises(AssertionError, match="above the tolerance tests' limit"):
        trr.check_opacities(torch.tensor([0.5, 0.9995]), False)


def test_yardstick_applies_on_a_hand_case():
    """Five rows, row 0 and 3 dead, both drawn onto row 1: N = 3."""
    tensors = [torch.arange(15, dtype=torch.float32).reshape(5, 3), torch.tensor([[0.001], [0.6], [0.3], [0.002], [0.9]]), torch.full((5, 3), 2.0)]
    roles = ["plain", "opacity", "scaling"]
    moments = [(torch.ones(5, 3), torch.ones(5, 3)), None, (torch.ones(5, 3), torch.ones(5, 3))]
    src, count = torch.tensor([1, -1, -1, 1, -1]), torch.tensor([0, 2, 0, 0, 0])
    (xyz, op, sc), (mx, mo, ms) = trr.relocate(tensors, roles, moments, src, count, False)
    import torch_ref_mcmc as trm
    o_new, s_new, _ = trm.relocation(np.float32([0.6]), np.full((1, 3), 2.0, np.float32), np.array([3]))
    assert xyz.tolist() == [[3, 4, 5], [3, 4, 5], [6, 7, 8], [3, 4, 5], [12, 13, 14]]
    assert op.reshape(-1).tolist() == [o_new[0], o_new[0], float(np.float32(0.3)), o_new[0], float(np.float32(0.9))]
    assert sc[[0, 1, 3]].tolist() == [s_new[0].tolist()] * 3 and sc[[2, 4]].tolist() == [[2.0] * 3] * 2
    assert mo is None and all(m[:, 0].tolist() == [1, 0, 1, 1, 1] for m in (*mx, *ms))
    _, (mx, _, _) = trr.relocate(tensors, roles, moments, src, count, False, reset_dead_moments=True)
    assert mx[0][:, 0].tolist() == [0, 0, 1, 0, 1] and mx[1][:, 0].tolist() == [0, 0, 1, 0, 1]
    (xyz, op, sc), (mx, _, _) = trr.grow(tensors, roles, moments, torch.tensor([1, 4, 1]), torch.tensor([0, 2, 0, 0, 1]), False)
    o4, s4, _ = trm.relocation(np.float32([0.9]), np.full((1, 3), 2.0, np.float32), np.array([2]))
    assert xyz.shape == (8, 3) and xyz[5:].tolist() == [[3, 4, 5], [12, 13, 14], [3, 4, 5]] and torch.equal(xyz[:5], tensors[0].double())
    assert op.reshape(-1).tolist() == [float(np.float32(0.001)), o_new[0], float(np.float32(0.3)), float(np.float32(0.002)), o4[0], o_new[0], o4[0], o_new[0]]
    assert mx[0][:, 0].tolist() == [1, 0, 1, 1, 0, 0, 0, 0] and mx[1][:, 0].tolist() == [1, 0, 1, 1, 0, 0, 0, 0] and sc[6].tolist() == s4[0].tolist()
    # the clamp and the inverse activations: a source of sigmoid 1.0 in raw mode stores the logit of 1 - eps
    k, o_raw, s_raw = trr.new_values(torch.tensor([[40.0], [0.0]]), torch.zeros(2, 3), torch.tensor([1, 0]), True)
    assert k.tolist() == [0] and abs(float(o_raw[0]) - np.log(trr.ONE_MINUS_EPS / (1 - trr.ONE_MINUS_EPS))) < 1e-9 and np.isfinite(s_raw.numpy()).all()


def _plans_of_the_gpu_tests(raw):
    """the (inputs, count) pairs whose sources the GPU tests hold to the bound: the relocation at every size, the growth at n in {1, 3, 300}"""
    for P in trr.SIZES:
        inp = trr.model_inputs(P, raw)
        dead = trr.dead_rows(inp["opacity"], raw)
        yield inp, trr.sample_relocation(trr.relocation_weights(inp["opacity"], raw), dead, inp["uniforms"])[1]
        for n in (1, 3, 300):
            yield inp, trr.sample_growth(trr.growth_weights(inp["opacity"], raw), trr.growth_uniforms(P, n))[1]


def test_measured_tolerance_of_the_raw_path():
    worst = 0.0
    for inp, count in _plans_of_the_gpu_tests(True):
        k, o_ref, s_ref = trr.new_values(inp["opacity"], inp["scaling"], count, True)
        k2, o_got, s_got = trr.stored_kernel_order(inp["opacity"].numpy(), inp["scaling"].numpy(), count.numpy(), True)
        assert k.tolist() == k2.tolist()
        worst = max(worst, trr.stored_error(o_got, o_ref.numpy()), trr.stored_error(s_got, s_ref.numpy()))
    print(f"\nraw relocation restatement: worst |stored - ref| / max(1, |ref|) {worst:.3g}; GPU bound {trr.RELOCATE_RAW_BOUND:.3g}")
    assert 0.5 * trr.RELOCATE_RAW_MEASURED <= worst <= trr.RELOCATE_RAW_MEASURED
    assert trr.RELOCATE_RAW_BOUND == 4 * trr.RELOCATE_RAW_MEASURED


def test_non_raw_restatement_is_the_public_compute_relocation_order():
    """raw=False: the restatement differs from the float64 yardstick by the final rounding to float32 only (the GPU test asks for the bits of
    compute_relocation, not for a bound)."""
    import torch_ref_mcmc as trm
    worst = 0.0
    for inp, count in _plans_of_the_gpu_tests(False):
        k, o_ref, s_ref = trr.new_values(inp["opacity"], inp["scaling"], count, False)
        _, o_got, s_got = trr.stored_kernel_order(inp["opacity"].numpy(), inp["scaling"].numpy(), count.numpy(), False)
        if k.numel() == 0:
            continue
        worst = max(worst, float(np.max(np.abs(o_got - o_ref.numpy()) / o_ref.numpy())), float(np.max(np.abs(s_got - s_ref.numpy()) / s_ref.numpy())))
    assert worst <= trm.RELOCATION_MEASURED


def test_measured_tolerance_of_the_raw_weights():
    worst = 0
    for P in trr.SIZES:
        inp = trr.model_inputs(P, True)
        o64 = trr.activated64(inp["opacity"], True)
        for ref, cand in ((trr.relocation_weights(inp["opacity"], True), (o64 > trr.f32(trr.MIN_OPACITY)).numpy()), (trr.growth_weights(inp["opacity"], True), np.ones(P, bool))):
            got = trr.weights_kernel_order(inp["opacity"].numpy(), True, cand)
            worst = max(worst, int(np.max(np.abs(got - ref.numpy()))))
        # dead-ness by the float32 sigmoid equals the float64 decision: the exclusion band's purpose
        assert np.array_equal(trr.sigmoid32(inp["opacity"].numpy().reshape(-1)) <= np.float32(trr.MIN_OPACITY), trr.dead_rows(inp["opacity"], True).numpy())
    print(f"\nraw weights: worst |w32 - round(sigmoid64 * 2^24)| {worst}; GPU bound {trr.RELOCATE_RAW_WEIGHT_BOUND}")
    assert worst == trr.RELOCATE_RAW_WEIGHT_MEASURED and trr.RELOCATE_RAW_WEIGHT_BOUND == 4 * trr.RELOCATE_RAW_WEIGHT_MEASURED
