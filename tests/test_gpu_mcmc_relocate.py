"""GPU tests of the fused 3DGS-MCMC relocation and growth (mcmc_relocation_plan, mcmc_relocate_tensors_, mcmc_relocate_, mcmc_add_plan,
mcmc_add_tensors, mcmc_add_new; include/stp_raster.h: stp_mcmc_sample, stp_mcmc_relocate_apply, stp_mcmc_add_apply) against the yardstick
tests/torch_ref_mcmc_relocate.py:
  1. the sampling is exact: weights, src and count equal the int64 cumsum / searchsorted restatement, for both raw values;
  2. the relocation apply with raw=False gives the bits of the public compute_relocation, copies are bit-exact, everything else keeps its bits;
  3. with raw=True the stored opacity and scaling are held to RELOCATE_RAW_BOUND (measured on the CPU, tests/test_mcmc_relocate_cpu.py);
  4. contention and edges: one source for 256 dead rows, no dead rows, no live rows, a source of opacity 1, the uniforms' edges, trailing
     shapes, a misaligned view, more than eight tensors;
  5. the growth, and mcmc_add_new on both optimizers;  6. mcmc_relocate_ on both optimizers;  7. the C ABI with raw pointers;  8. the example."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import torch_ref_mcmc_relocate as trr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))


def dgr():
    import diff_gaussian_rasterization as d
    return d


def _C():
    from diff_gaussian_rasterization import _C as c
    return c


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def is_plus_zero(t):
    return bool((bits(t) == 0).all())


_inputs = {}


def inputs(P, raw):
    """the yardstick's inputs of a size, generated once and never modified (the tests work on clones on the device)"""
    if (P, raw) not in _inputs:
        _inputs[(P, raw)] = trr.model_inputs(P, raw, names=trr.NAMES if P <= max(trr.SIZES) else ("opacity", "scaling"))   # (MANY_TILES: sampling only)
    return _inputs[(P, raw)]


def on_gpu(inp):
    """-> (tensors, roles, exp_avgs, exp_avg_sqs) on the device, fresh clones in trr.NAMES' order"""
    tensors, roles, moments = trr.lists_of(inp)
    return [t.cuda() for t in tensors], roles, [m.cuda() for m, _ in moments], [v.cuda() for _, v in moments]


# ---- 1. sampling ---------------------------------------------------------------------------------------------------------------------------------

MANY_TILES = 524_289   # 257 tiles of 2048 rows: a thread of the tile prefix owns two tile sums


@pytest.mark.parametrize("P,raw", [(P, raw) for P in trr.SIZES for raw in (False, True)] + [(MANY_TILES, False)])
def test_sampling_is_exact(P, raw):
    inp = inputs(P, raw)
    o, u = inp["opacity"].cuda(), inp["uniforms"].cuda()
    src, count, w = dgr().mcmc_relocation_plan(o, u, raw=raw, return_weights=True)
    assert src.dtype == count.dtype == w.dtype == torch.int32 and src.shape == count.shape == w.shape == (P,)
    assert same_bits(o, inp["opacity"].cuda()) and same_bits(u, inp["uniforms"].cuda()), "an input was modified"
    src, count, w = src.cpu().long(), count.cpu().long(), w.cpu().long()
    ref_w = trr.relocation_weights(inp["opacity"], raw)
    if raw:   # the float32 sigmoid against the float64 one, in integer units (measured on the CPU, times 4)
        worst = int((w - ref_w).abs().max())
        print(f"\nP={P}: worst |w - round(sigmoid64 * 2^24)| {worst} (bound {trr.RELOCATE_RAW_WEIGHT_BOUND})")
        assert worst <= trr.RELOCATE_RAW_WEIGHT_BOUND
    else:
        assert torch.equal(w, ref_w)
    dead = trr.dead_rows(inp["opacity"], raw)   # the float64 decision: the generator's exclusion band makes it the kernel's
    assert torch.equal(w == 0, dead) or P == 1
    assert torch.equal(src >= 0, dead if bool((~dead).any()) else torch.zeros_like(dead))
    ref_src, ref_count = trr.sample_relocation(w, dead, inp["uniforms"])   # with the RETURNED weights: exact for both raw values
    assert torch.equal(src, ref_src) and torch.equal(count, ref_count)
    assert torch.equal(count, trr.count_of(src, P))
    assert not bool(dead[src[src >= 0]].any()), "a source is a dead row"
    # growth: every row is a candidate
    for n in (1, 3, 300):
        ug = trr.growth_uniforms(P, n)
        gsrc, gcount = dgr().mcmc_add_plan(o, ug.cuda(), raw=raw)
        assert gsrc.shape == (n,) and gcount.shape == (P,) and gsrc.dtype == gcount.dtype == torch.int32
        gw = trr.growth_weights(inp["opacity"], raw) if not raw else None
        if raw:   # the kernel's own weights of all rows: those of a relocation whose threshold nothing falls under
            gw = dgr().mcmc_relocation_plan(o, u, raw=True, min_opacity=-1.0, return_weights=True)[2].cpu().long()
            assert int((gw - trr.growth_weights(inp["opacity"], True)).abs().max()) <= trr.RELOCATE_RAW_WEIGHT_BOUND
        ref_src, ref_count = trr.sample_growth(gw, ug)
        assert torch.equal(gsrc.cpu().long(), ref_src) and torch.equal(gcount.cpu().long(), ref_count)


def test_sampling_edges_of_the_uniforms():
    P = 257
    o = torch.linspace(0.01, 0.9, P)
    o[::2] = 0.001
    w, dead = trr.relocation_weights(o, False), trr.dead_rows(o, False)
    for value in (0.0, BELOW_ONE, 1.0, float("nan"), -0.5, 3.0):
        u = torch.full((P,), value)
        src, count = dgr().mcmc_relocation_plan(o.cuda(), u.cuda(), raw=False)
        ref_src, ref_count = trr.sample_relocation(w, dead, u)
        assert torch.equal(src.cpu().long(), ref_src) and torch.equal(count.cpu().long(), ref_count), value
        first, last = 1, P - 1 if (P - 1) % 2 else P - 2
        assert set(src.cpu()[dead].tolist()) == {first if value in (0.0, -0.5) or value != value else last}
    nan_o = o.clone()
    nan_o[3], nan_o[4] = float("nan"), float("nan")   # neither dead nor a candidate
    src, count, w = dgr().mcmc_relocation_plan(nan_o.cuda(), torch.rand(P).cuda(), raw=False, return_weights=True)
    assert src[3] == -1 and src[4] == -1 and w[3] == 0 and w[4] == 0 and count[3] == 0 and count[4] == 0


# ---- 2 / 3. the relocation apply -----------------------------------------------------------------------------------------------------------------

def check_relocation(inp, raw, tensors, ms, vs, src, count, reset):
    """the device tensors after an in-place relocation by (src, count), against the inputs they started from"""
    P = count.numel()
    before_t, roles, moments = trr.lists_of(inp)
    src, count = src.cpu().long(), count.cpu().long()
    drawn = count > 0
    dead = (src >= 0) & ~drawn
    other = ~drawn & ~dead
    ref_t, _ = trr.relocate(before_t, roles, moments, src, count, raw)
    k = torch.nonzero(drawn)[:, 0]
    if not raw and k.numel():   # the bits of the public call, clamped as upstream clamps
        o_new, s_new = dgr().compute_relocation(inp["opacity"].cuda()[k], inp["scaling"].cuda()[k], (count[k] + 1).cuda())
        o_new = o_new.clamp(trr.f32(trr.MIN_OPACITY), trr.ONE_MINUS_EPS)
    worst = 0.0
    for name, role, t, m, v, old, ref, (m0, v0) in zip(trr.NAMES, roles, tensors, ms, vs, before_t, ref_t, moments):
        t, m, v = t.cpu(), m.cpu(), v.cpu()
        assert same_bits(t[other], old[other]) and same_bits(m[other], m0[other]) and same_bits(v[other], v0[other]), name
        assert is_plus_zero(m[drawn]) and is_plus_zero(v[drawn]), name
        if reset:
            assert is_plus_zero(m[dead]) and is_plus_zero(v[dead]), name
        else:
            assert same_bits(m[dead], m0[dead]) and same_bits(v[dead], v0[dead]), name
        if role == "plain":
            assert same_bits(t[drawn], old[drawn]) and same_bits(t[dead], old[src[dead]]), name
            continue
        assert same_bits(t[dead], t[src[dead]]), name   # all rows of a source agree
        if not raw:
            if k.numel():
                assert same_bits(t[k], (o_new if role == "opacity" else s_new).cpu().reshape(t[k].shape)), name
        else:
            worst = max(worst, trr.stored_error(t[k].double().numpy(), ref[k].numpy()))
    if raw:
        print(f"\nP={P}: worst |stored - ref| / max(1, |ref|) {worst:.3g} (bound {trr.RELOCATE_RAW_BOUND:.3g})")
        assert worst <= trr.RELOCATE_RAW_BOUND


@pytest.mark.parametrize("reset", [False, True])
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("P", trr.SIZES)
def test_relocation_apply(P, raw, reset):
    inp = inputs(P, raw)
    tensors, roles, ms, vs = on_gpu(inp)
    plan = dgr().mcmc_relocation_plan(inp["opacity"].cuda(), inp["uniforms"].cuda(), raw=raw)
    assert dgr().mcmc_relocate_tensors_(plan, tensors, roles, ms, vs, raw=raw, reset_dead_moments=reset) is None
    check_relocation(inp, raw, tensors, ms, vs, plan[0], plan[1], reset)


# ---- 4. contention and edges ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("raw", [False, True])
def test_one_source_for_all_dead_rows(raw):
    P = 257
    inp = {k: v.clone() for k, v in inputs(P, raw).items()}
    o = torch.full((P, 1), 0.002)
    o[100] = 0.7
    inp["opacity"] = torch.log(o / (1 - o)) if raw else o
    runs = []
    for _ in range(2):
        tensors, roles, ms, vs = on_gpu(inp)
        src, count = dgr().mcmc_relocation_plan(inp["opacity"].cuda(), inp["uniforms"].cuda(), raw=raw)
        assert int(count[100]) == 256 and int(count.sum()) == 256 and src[100] == -1 and bool((src.cpu()[torch.arange(P) != 100] == 100).all())
        dgr().mcmc_relocate_tensors_((src, count), tensors, roles, ms, vs, raw=raw)
        check_relocation(inp, raw, tensors, ms, vs, src, count, False)   # (N = 257 is clamped to 50 in the yardstick and in compute_relocation alike)
        for t in tensors:
            assert same_bits(t, t[100:101].expand_as(t).contiguous())   # every row is the source's now
        runs.append(tensors + ms + vs)
    assert all(same_bits(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("value", [0.5, 0.001], ids=["no-dead-rows", "no-live-rows"])
def test_nothing_to_relocate_changes_nothing(value, raw):
    P = 4097
    inp = {k: v.clone() for k, v in inputs(P, raw).items()}
    o = torch.full((P, 1), value)
    inp["opacity"] = torch.log(o / (1 - o)) if raw else o
    tensors, roles, ms, vs = on_gpu(inp)
    plan = dgr().mcmc_relocation_plan(inp["opacity"].cuda(), inp["uniforms"].cuda(), raw=raw)
    assert bool((plan[0] == -1).all()) and bool((plan[1] == 0).all())
    dgr().mcmc_relocate_tensors_(plan, tensors, roles, ms, vs, raw=raw, reset_dead_moments=True)
    before_t, _, moments = trr.lists_of(inp)
    for t, m, v, t0, (m0, v0) in zip(tensors, ms, vs, before_t, moments):
        assert same_bits(t.cpu(), t0) and same_bits(m.cpu(), m0) and same_bits(v.cpu(), v0)


@pytest.mark.parametrize("raw", [False, True])
def test_a_source_of_opacity_one_is_clamped(raw):
    P = 65
    inp = {k: v.clone() for k, v in inputs(P, raw).items()}
    o = torch.full((P, 1), 0.001)
    o[7] = 1.0
    inp["opacity"] = torch.where(o == 1.0, torch.tensor(40.0), torch.log(o / (1 - o))) if raw else o   # (sigmoid(40) is 1.0 in float32)
    tensors, roles, ms, vs = on_gpu(inp)
    plan = dgr().mcmc_relocation_plan(inp["opacity"].cuda(), inp["uniforms"].cuda(), raw=raw)
    assert int(plan[1][7]) == 64
    dgr().mcmc_relocate_tensors_(plan, tensors, roles, ms, vs, raw=raw)
    got = tensors[trr.NAMES.index("opacity")].cpu().reshape(-1)
    o_one, _ = dgr().compute_relocation(torch.ones(1).cuda(), torch.ones(1, 3).cuda(), torch.tensor([50]).cuda())
    want = o_one.cpu().clamp(trr.f32(trr.MIN_OPACITY), trr.ONE_MINUS_EPS)   # 1 - (1 - 1)^(1/50) = 1: the clamp decides
    assert float(want) == trr.ONE_MINUS_EPS
    if raw:
        want = torch.log(want / (1.0 - want))
        assert bool(torch.isfinite(got).all()) and bool(((got - want).abs() <= 1e-5 * want.abs()).all())
        assert bool(torch.isfinite(tensors[trr.NAMES.index("scaling")]).all())
    else:
        assert same_bits(got, want.expand(P).contiguous())


@pytest.mark.parametrize("raw", [False, True])
def test_a_misaligned_view_gives_the_same_bits(raw):
    P = 257
    inp = inputs(P, raw)
    plan = dgr().mcmc_relocation_plan(inp["opacity"].cuda(), inp["uniforms"].cuda(), raw=raw)
    aligned, roles, ms, vs = on_gpu(inp)
    dgr().mcmc_relocate_tensors_(plan, aligned, roles, ms, vs, raw=raw)

    def shifted(t):   # a contiguous view that starts 4 bytes into its storage
        base = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
        view = base[1:].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        return view
    t2, _, m2, v2 = on_gpu(inp)
    t2, m2, v2 = [shifted(t) for t in t2], [shifted(t) for t in m2], [shifted(t) for t in v2]
    dgr().mcmc_relocate_tensors_(plan, t2, roles, m2, v2, raw=raw)
    assert all(same_bits(a, b) for a, b in zip(aligned + ms + vs, t2 + m2 + v2))
    # the growth too
    gplan = dgr().mcmc_add_plan(inp["opacity"].cuda(), trr.growth_uniforms(P, 30).cuda(), raw=raw)
    a, _, am, av = on_gpu(inp)
    out_a = dgr().mcmc_add_tensors(gplan, a, roles, am, av, raw=raw)
    out_b = dgr().mcmc_add_tensors(gplan, [shifted(t) for t in a], roles, [shifted(t) for t in am], [shifted(t) for t in av], raw=raw)
    assert all(same_bits(x, y) for la, lb in zip(out_a, out_b) for x, y in zip(la, lb))


def test_more_than_eight_tensors_and_trailing_shapes():
    """eleven tensors -- two launches of the apply -- with the trailing shapes (15, 3), (1, 3), (4,), (1,) among them, some without moments"""
    P = 4097
    inp = inputs(P, True)
    tensors, roles, ms, vs = on_gpu(inp)
    assert {tuple(t.shape[1:]) for t in tensors} >= {(15, 3), (1, 3), (4,), (1,), (3,)}
    extra = [torch.randn(P, *shape, device="cuda") for shape in ((4,), (1,), (15, 3), (2, 4), (7,))]
    plan = dgr().mcmc_relocation_plan(inp["opacity"].cuda(), inp["uniforms"].cuda())
    all_t = [e.clone() for e in extra[:3]] + tensors + [e.clone() for e in extra[3:]]
    all_r = ["plain"] * 3 + roles + ["plain"] * 2
    all_m = [None, torch.ones_like(extra[1]), None] + ms + [torch.ones_like(extra[3]), None]
    all_v = [None, torch.ones_like(extra[1]), None] + vs + [torch.ones_like(extra[3]), None]
    assert len(all_t) == 11
    dgr().mcmc_relocate_tensors_(plan, all_t, all_r, all_m, all_v)
    check_relocation(inp, True, all_t[3:9], all_m[3:9], all_v[3:9], plan[0], plan[1], False)
    src, count = plan[0].cpu().long(), plan[1].cpu().long()
    dead = src >= 0
    for got, old in zip(all_t[:3] + all_t[9:], extra):
        want = old.cpu().clone()
        want[dead] = old.cpu()[src[dead]]
        assert same_bits(got.cpu(), want)
    for m in (all_m[1], all_m[9]):
        assert is_plus_zero(m.cpu()[count > 0]) and bool((m.cpu()[count == 0] == 1).all())


# ---- 5. growth -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("P", trr.SIZES)
def test_growth_against_the_yardstick(P, raw):
    inp = inputs(P, raw)
    before_t, roles, moments = trr.lists_of(inp)
    for n in (0, 1, 3, 300):
        tensors, _, ms, vs = on_gpu(inp)
        plan = dgr().mcmc_add_plan(inp["opacity"].cuda(), trr.growth_uniforms(P, n).cuda(), raw=raw)
        new_t, new_m, new_v = dgr().mcmc_add_tensors(plan, tensors, roles, ms, vs, raw=raw)
        for t, m, v, t0, (m0, v0) in zip(tensors, ms, vs, before_t, moments):
            assert same_bits(t.cpu(), t0) and same_bits(m.cpu(), m0) and same_bits(v.cpu(), v0), "an input was modified"
        src, count = plan[0].cpu().long(), plan[1].cpu().long()
        assert bool((src >= 0).all())
        drawn = count > 0
        ref_t, _ = trr.grow(before_t, roles, moments, src, count, raw)
        k = torch.nonzero(drawn)[:, 0]
        if not raw and k.numel():
            o_new, s_new = dgr().compute_relocation(inp["opacity"].cuda()[k], inp["scaling"].cuda()[k], (count[k] + 1).cuda())
            o_new = o_new.clamp(trr.f32(trr.MIN_OPACITY), trr.ONE_MINUS_EPS)
        worst = 0.0
        for name, role, t, m, v, old, ref, (m0, v0) in zip(trr.NAMES, roles, new_t, new_m, new_v, before_t, ref_t, moments):
            t, m, v = t.cpu(), m.cpu(), v.cpu()
            assert t.shape == (P + n,) + old.shape[1:] == m.shape == v.shape
            assert same_bits(t[:P][~drawn], old[~drawn]) and same_bits(m[:P][~drawn], m0[~drawn]) and same_bits(v[:P][~drawn], v0[~drawn]), name
            assert is_plus_zero(m[:P][drawn]) and is_plus_zero(v[:P][drawn]) and is_plus_zero(m[P:]) and is_plus_zero(v[P:]), name
            assert same_bits(t[P:], t[:P][src]), name   # an appended row is its (rewritten) source, in the draws' order
            if role == "plain":
                assert same_bits(t[:P], old), name
            elif not raw:
                if k.numel():
                    assert same_bits(t[k], (o_new if role == "opacity" else s_new).cpu().reshape(t[k].shape)), name
            else:
                worst = max(worst, trr.stored_error(t[k].double().numpy(), ref[k].numpy()))
        assert worst <= trr.RELOCATE_RAW_BOUND, (n, worst)


def named_optimizer(kind, inp, with_state=True, stateless=("rotation",)):
    tensors, roles, moments = trr.lists_of(inp)
    params = [torch.nn.Parameter(t.cuda()) for t in tensors]
    groups = [{"params": [p], "lr": 0.01, "name": n} for p, n in zip(params, trr.NAMES)]
    opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15) if kind == "adam" else dgr().SparseGaussianAdam(groups, lr=0.0, eps=1e-15)
    if with_state:
        for p, n, (m, v) in zip(params, trr.NAMES, moments):
            if n not in stateless:
                opt.state[p] = {"step": torch.tensor(7.0), "exp_avg": m.cuda(), "exp_avg_sq": v.cuda()}
    return opt, params


@pytest.mark.parametrize("kind", ["adam", "sparse_adam"])
def test_add_new_on_an_optimizer(kind):
    P, raw = 4097, True
    inp = inputs(P, raw)
    opt, params = named_optimizer(kind, inp)
    assert dgr().mcmc_add_new(opt, P) == {} and dgr().mcmc_add_new(opt, 100) == {}   # n_new == 0 changes nothing
    assert all(g["params"][0] is p for g, p in zip(opt.param_groups, params)) and len(opt.state) == 5
    n = min(4200, int(1.05 * P)) - P
    u = trr.growth_uniforms(P, n).cuda()
    new = dgr().mcmc_add_new(opt, 4200, u)
    assert set(new) == set(trr.NAMES) and n == 103
    tensors, roles, ms, vs = on_gpu(inp)
    plan = dgr().mcmc_add_plan(inp["opacity"].cuda(), u)
    want_t, want_m, want_v = dgr().mcmc_add_tensors(plan, tensors, roles, ms, vs)
    for g, name, old, t, m, v in zip(opt.param_groups, trr.NAMES, params, want_t, want_m, want_v):
        p = g["params"][0]
        assert p is new[name] and isinstance(p, torch.nn.Parameter) and p.requires_grad and p.shape[0] == P + n and same_bits(p, t)
        assert old not in opt.state
        if name == "rotation":
            assert p not in opt.state   # a group without state stays without
        else:
            st = opt.state[p]
            assert float(st["step"]) == 7.0 and same_bits(st["exp_avg"], m) and same_bits(st["exp_avg_sq"], v)
    with pytest.raises(ValueError, match="uniforms has 5 rows"):
        dgr().mcmc_add_new(opt, 10000, torch.rand(5).cuda())
    torch.manual_seed(11)
    again = dgr().mcmc_add_new(opt, 10000)   # uniforms=None: torch.rand
    assert again["xyz"].shape[0] == int(1.05 * (P + n))


# ---- 6. mcmc_relocate_ ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["adam", "sparse_adam"])
def test_relocate_on_an_optimizer(kind):
    P, raw = 4097, True
    inp = inputs(P, raw)
    opt, params = named_optimizer(kind, inp)
    state_before = {id(p): opt.state.get(p) for p in params}
    plan = dgr().mcmc_relocate_(opt, inp["uniforms"].cuda())
    tensors, roles, ms, vs = on_gpu(inp)
    plan2 = dgr().mcmc_relocation_plan(inp["opacity"].cuda(), inp["uniforms"].cuda())
    assert torch.equal(plan[0], plan2[0]) and torch.equal(plan[1], plan2[1]) and int((plan[0] >= 0).sum()) > 0
    dgr().mcmc_relocate_tensors_(plan2, tensors, roles, ms, vs)
    for g, name, p, t, m, v in zip(opt.param_groups, trr.NAMES, params, tensors, ms, vs):
        assert g["params"][0] is p and same_bits(p, t), name   # identity kept
        if name == "rotation":
            assert p not in opt.state
        else:
            st = opt.state[p]
            assert st is state_before[id(p)] and set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 7.0
            assert same_bits(st["exp_avg"], m) and same_bits(st["exp_avg_sq"], v), name
    runs = []
    for _ in range(2):   # uniforms=None under a fixed seed
        opt, params = named_optimizer(kind, inp)
        torch.manual_seed(5)
        plan = dgr().mcmc_relocate_(opt, reset_dead_moments=True)
        runs.append([plan[0], plan[1]] + [p.detach() for p in params] + [opt.state[p]["exp_avg"] for p in params if p in opt.state])
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and int((runs[0][0] >= 0).sum()) > 0


# ---- 7. the C ABI --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("raw", [0, 1])
def test_through_the_c_abi(raw):
    P, n_new = 65, 9
    inp = inputs(P, bool(raw))
    c = _C()
    L = c._load()
    o, u = inp["opacity"].cuda(), inp["uniforms"].cuda()
    want_plan = dgr().mcmc_relocation_plan(o, u, raw=bool(raw), return_weights=True)
    want, roles, wm, wv = on_gpu(inp)
    dgr().mcmc_relocate_tensors_(want_plan, want, roles, wm, wv, raw=bool(raw), reset_dead_moments=True)
    nbytes = L.stp_mcmc_relocate_scratch_bytes(P)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    src, count, w = (torch.full((P,), 77, dtype=torch.int32, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    assert L.stp_mcmc_sample(P, o.data_ptr(), 0, 0.005, raw, P, u.data_ptr(), scratch.data_ptr(), nbytes, w.data_ptr(), src.data_ptr(), count.data_ptr(), None) == 4
    torch.cuda.synchronize()
    assert torch.equal(src, want_plan[0]) and torch.equal(count, want_plan[1]) and torch.equal(w, want_plan[2])
    tensors, _, ms, vs = on_gpu(inp)
    table = (c.StpMcmcTensor * len(tensors))()
    for k, (t, m, v, role) in enumerate(zip(tensors, ms, vs, roles)):
        table[k] = c.StpMcmcTensor(t.data_ptr(), m.data_ptr(), v.data_ptr(), None, None, None, t.numel() // P, c.MCMC_ROLES[role])
    assert L.stp_mcmc_relocate_apply(P, src.data_ptr(), count.data_ptr(), len(tensors), ctypes.addressof(table), 0.005, raw, 1, scratch.data_ptr(), nbytes, None) == 2
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(tensors + ms + vs, want + wm + wv))
    # growth
    ug = trr.growth_uniforms(P, n_new).cuda()
    gplan = dgr().mcmc_add_plan(o, ug, raw=bool(raw))
    ins, _, im, iv = on_gpu(inp)
    want_t, want_m, want_v = dgr().mcmc_add_tensors(gplan, ins, roles, im, iv, raw=bool(raw))
    gsrc = torch.empty(n_new, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert L.stp_mcmc_sample(P, o.data_ptr(), 1, 0.0, raw, n_new, ug.data_ptr(), scratch.data_ptr(), nbytes, None, gsrc.data_ptr(), count.data_ptr(), None) == 4
    outs = [[torch.empty((P + n_new,) + t.shape[1:], device="cuda") for t in ins] for _ in range(3)]
    for k, (t, m, v, role) in enumerate(zip(ins, im, iv, roles)):
        table[k] = c.StpMcmcTensor(t.data_ptr(), m.data_ptr(), v.data_ptr(), outs[0][k].data_ptr(), outs[1][k].data_ptr(), outs[2][k].data_ptr(), t.numel() // P,
                                   c.MCMC_ROLES[role])
    assert L.stp_mcmc_add_apply(P, n_new, gsrc.data_ptr(), count.data_ptr(), len(ins), ctypes.addressof(table), 0.005, raw, scratch.data_ptr(), nbytes, None) == 2
    torch.cuda.synchronize()
    assert torch.equal(gsrc, gplan[0]) and torch.equal(count, gplan[1])
    assert all(same_bits(a, b) for a, b in zip(outs[0] + outs[1] + outs[2], want_t + want_m + want_v))


# ---- 8. the example ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra", [[], ["--raw-params", "--split-sh"]], ids=["sparse_adam", "sparse_adam-raw-split"])
def test_example_trains_with_the_fused_relocation(extra):
    """examples/train_render.py --strategy mcmc --relocate fused --optimizer sparse_adam in a child process: the run relocated Gaussians (every
    fiftieth starts dead), grew by 5 %, and the short fit still descends (the existing example tests' condition, last < 0.8 * first).
    The first case, without --split-sh, is also the one test of the example's single SH group under SparseGaussianAdam: measured on an MI355X
    0.03995 -> 0.01218 (0.01166 with --relocate torch); with --raw-params --split-sh 0.03995 -> 0.01164."""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_render.py"), "--strategy", "mcmc", "--relocate", "fused", "--optimizer", "sparse_adam",
           "--iters", "15", "--points", "3000", "--size", "96", "64"] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=170)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    r = re.search(r"^mcmc: relocated (\d+) Gaussians in (\d+) relocation steps", p.stdout, re.M)
    assert r and int(r.group(1)) > 0 and int(r.group(2)) == 1, p.stdout[-2000:]
    a = re.search(r"^mcmc: (\d+) Gaussians added towards cap_max = 3450, (\d+) at the end", p.stdout, re.M)
    assert a and int(a.group(1)) == 150 and int(a.group(2)) == 3150, p.stdout[-2000:]
    m = re.search(r"^\S.* ([0-9.eE+-]+) -> ([0-9.eE+-]+); depth visualisation", p.stdout, re.M)
    assert m, p.stdout[-2000:]
    first, last = float(m.group(1)), float(m.group(2))
    print(f"\n{extra}: first {first} last {last}")
    assert last < 0.8 * first, (first, last)
