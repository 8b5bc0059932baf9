"""GPU tests of the densification kernels (densification_stats_, densify_plan, densify_tensors, densify_and_prune, _C.densify_scan,
_C.densify_apply; include/stp_raster.h: stp_densify_stats / _plan / _scan / _apply) against the yardstick tests/torch_ref_densify.py.

Statistics and plan are held bit for bit (the plan on inputs whose compared values are at least 1e-4, relative, from every threshold --
tests/test_densify_cpu.py asserts that on the CPU -- and, not raw, on values exactly ON the thresholds).  The apply's copies are held bit
for bit, moments included; a split's children to 4 times the worst error of the CPU restatement of the kernel's evaluation order on exactly
these inputs, as tests/test_densify_cpu.py measures it (torch_ref_densify.CHILD_XYZ_BOUND = 6.4e-7 from 1.6e-7, CHILD_SCALING_BOUND =
6.4e-7 from 1.6e-7):  |xyz' - ref|_2 <= T max(s) |noise|_2 + ulp(|ref|_inf)  and  |scaling' - ref| <= T max(1, |ref|).

One lane per Gaussian in workgroups of 256 (statistics, plan), 16 flags per lane and 4096 per workgroup in the scan (3 P flags: P = 4097
is three workgroups with a ragged last one), 1024 items per workgroup in the apply: the sizes are the wave and workgroup edges and more
than one workgroup in every kernel; rows of 1, 3, 4 and 45 floats take the one-float path, rows of 4 floats with aligned pointers the 16-byte
path, and views that start 4 or 12 bytes into their storage force the one-float path on rows of 4."""
import numpy as np
import pytest
import torch

import torch_ref_densify as trd

pytestmark = pytest.mark.gpu

NAMES = [n for n, _ in trd.GROUPS]
MODEL_ROLES = [trd.ROLES.get(n, 0) for n in NAMES]


def dgr():
    import diff_gaussian_rasterization as d
    return d


def _C():
    from diff_gaussian_rasterization import _C as c
    return c


def dev(a, offset_floats=0):
    """A contiguous cuda tensor of the array's values; offset_floats = k: a view that starts 4 k bytes into its storage."""
    a = np.ascontiguousarray(a)
    if offset_floats == 0:
        return torch.from_numpy(a).cuda()
    base = torch.empty(a.size + offset_floats, dtype=torch.float32, device="cuda")
    t = base[offset_floats:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() % 16 == (4 * offset_floats) % 16
    return t


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(t, a):
    """a cuda float32 tensor against a numpy array of float32 values"""
    got = t.detach().cpu().numpy()
    return got.shape == np.shape(a) and np.array_equal(bits(got), bits(a))


class no_sync:
    """torch's synchronisation check armed on a side stream: nothing inside waits for the device or reads a value back"""

    def __enter__(self):
        torch.cuda.synchronize()
        self.side = torch.cuda.Stream()
        self.previous = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        self.ctx = torch.cuda.stream(self.side)
        self.ctx.__enter__()

    def __exit__(self, *exc):
        self.ctx.__exit__(*exc)
        torch.cuda.set_sync_debug_mode(self.previous)
        self.side.synchronize()


_MODELS = {}


def model(P):
    """the shared inputs of size P and their yardstick plan (computed once, never modified)"""
    if P not in _MODELS:
        d = trd.model_inputs(P)
        _MODELS[P] = (d, trd.model_plan(d), trd.model_plan(d, with_radii=True))
    return _MODELS[P]


# ---- statistics ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", trd.SIZES)
@pytest.mark.parametrize("width", [3, 2])
@pytest.mark.parametrize("kind", ["radii", "mask"])
def test_stats_bit_equal_without_synchronisation(P, width, kind):
    rng = np.random.default_rng(7 * P + width)
    d = model(P)[0]
    grad = (rng.standard_normal((P, width)) * np.exp(rng.uniform(-12, 2, (P, 1)))).astype(np.float32)
    radii = (rng.integers(0, 60, P) * (rng.uniform(size=P) < 0.6)).astype(np.int32)
    if P > 2:
        radii[0], radii[1] = 0, 3
    grad[radii == 0] = np.nan                        # the gradient of an invisible row is never used
    accum0, denom0, mr0 = d["accum"].copy(), d["denom"].copy(), d["max_radii2D"].copy()
    with_radii = kind == "radii"
    want = trd.stats(accum0, denom0, mr0 if with_radii else None, grad, radii if with_radii else radii > 0)
    accum, denom, mr = dev(accum0[:, None]), dev(denom0), dev(mr0[:, None])     # (P, 1) and (P,) accumulators
    g, r = dev(grad), torch.from_numpy(radii).cuda()
    vis = r if with_radii else r > 0
    with no_sync():
        assert dgr().densification_stats_(accum, denom, mr if with_radii else None, g, vis) is None
    assert same_bits(accum[:, 0], want[0]) and same_bits(denom, want[1])
    assert same_bits(mr[:, 0], want[2] if with_radii else mr0)
    hidden = radii == 0
    assert np.array_equal(bits(accum.cpu().numpy()[hidden, 0]), bits(accum0[hidden])) and not np.isnan(accum.cpu().numpy()).any()
    if not with_radii:                               # a uint8 mask reads like the bool one
        accum2, denom2 = dev(accum0), dev(denom0)
        dgr().densification_stats_(accum2, denom2, None, g, (r > 0).to(torch.uint8))
        assert same_bits(accum2, want[0]) and same_bits(denom2, want[1])


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", trd.SIZES)
@pytest.mark.parametrize("with_radii", [False, True])
def test_plan_byte_equal_without_synchronisation(P, with_radii):
    d, plan_none, plan_radii = model(P)
    args = [dev(d["accum"][:, None]), dev(d["denom"][:, None]), dev(d["scaling"]), dev(d["opacity"])]
    mr = dev(d["max_radii2D"]) if with_radii else None
    with no_sync():
        got = dgr().densify_plan(*args, mr, **trd.RULE)
    assert got.dtype == torch.uint8 and got.shape == (P,)
    assert np.array_equal(got.cpu().numpy(), plan_radii if with_radii else plan_none)
    # without max_screen_size nothing is pruned for its size, whatever max_radii2D holds
    rule = dict(trd.RULE, max_screen_size=None)
    got = dgr().densify_plan(*args, mr, **rule)
    assert np.array_equal(got.cpu().numpy(), trd.plan(d["accum"], d["denom"], d["scaling"], d["opacity"], d["max_radii2D"] if with_radii else None, **rule))


def test_plan_on_the_thresholds_and_with_denom_zero():
    """raw=False, values exactly ON each threshold: g >= threshold is hot, max(s) <= split_size clones and > splits, o < min_opacity and the
    three sizes > their thresholds prune.  denom == 0: g = 0, whatever accum holds."""
    f = np.float32
    up = lambda x: np.nextafter(f(x), f(np.inf))
    down = lambda x: np.nextafter(f(x), f(-np.inf))
    rule = dict(grad_threshold=0.25, percent_dense=0.5, extent=1.0, min_opacity=0.125, max_screen_size=16.0, raw=False)   # split_size 0.5, max_world_size f32(0.1)
    world = f(trd.f32(0.1 * 1.0))
    rows = [  # accum, denom, max scale, opacity, max_radii2D -> plan
        (0.5, 2, 0.05, 0.5, 0, 3),            # g == threshold: hot (>=); small: clone
        (down(0.5), 2, 0.05, 0.5, 0, 1),      # just below: not hot
        (0.5, 2, world, 0.5, 0, 3),           # max(s) == max_world_size: not too large (>)
        (0.5, 2, up(world), 0.5, 0, 0),       # just above: original and copy both go
        (0.0, 2, up(world), 0.5, 0, 0),
        (0.0, 2, 0.05, 0.125, 0, 1),          # o == min_opacity: stays (<)
        (0.0, 2, 0.05, down(0.125), 0, 0),
        (0.0, 2, 0.05, 0.5, 16, 1),           # max_radii2D == max_screen_size: stays (>)
        (0.0, 2, 0.05, 0.5, up(16), 0),
        (0.5, 2, 0.05, 0.5, up(16), 2),       # the screen test takes the original, not the copy
        (7.0, 0, 0.05, 0.5, 0, 1),            # denom == 0: g = 0
        (np.inf, 0, 0.05, 0.5, 0, 1),
    ]
    accum, denom, smax, o, mr, want = (np.array(c, np.float32) for c in zip(*rows))
    sc = np.stack([smax, smax * f(0.5), smax * f(0.25)], axis=1)[:, [1, 0, 2]]
    assert trd.plan(accum, denom, sc, o, mr, **rule).tolist() == want.astype(int).tolist()
    got = dgr().densify_plan(dev(accum), dev(denom), dev(sc), dev(o), dev(mr), **rule)
    assert got.cpu().tolist() == want.astype(int).tolist()
    # split_size 0.5 exactly: <= clones, > splits; a child is tested with max(s) / 1.6 against max_world_size = 1
    rule = dict(grad_threshold=0.25, percent_dense=0.05, extent=10.0, min_opacity=0.125, max_screen_size=16.0, raw=False)
    world, shrink = f(trd.f32(0.1 * 10.0)), f(trd.f32(1.6))
    on = shrink                                                                                                    # max(s) / 1.6 == max_world_size exactly
    assert world == 1.0 and f(on / shrink) == world and trd.rule_numbers(0.25, 0.05, 10.0, 0.125, 16.0)["split_size"] == 0.5
    above = [x for x in (up(on), up(up(on))) if f(x / shrink) > world][0]
    rows = [(0.5, 2, 0.5, 0.5, 0, 3),          # max(s) == split_size: clone (<=)
            (0.5, 2, up(0.5), 0.5, 0, 4),      # just above: split (>)
            (0.5, 2, on, 0.5, 0, 4),           # the original is too large in the world, the children exactly on the threshold are not (>)
            (0.5, 2, above, 0.5, 0, 0),        # the children too
            (0.0, 2, on, 0.5, 0, 0)]           # not hot: the original alone, too large
    accum, denom, smax, o, mr, want = (np.array(c, np.float32) for c in zip(*rows))
    sc = np.stack([smax * f(0.5), smax * f(0.25), smax], axis=1)
    assert trd.plan(accum, denom, sc, o, mr, **rule).tolist() == want.astype(int).tolist()
    got = dgr().densify_plan(dev(accum), dev(denom), dev(sc), dev(o), dev(mr), **rule)
    assert got.cpu().tolist() == want.astype(int).tolist()


# ---- scan and apply ------------------------------------------------------------------------------------------------------------------------

def check_apply(plan, tensors, roles, ms, vs, noise, got, raw=True):
    """got = (new_tensors, new_ms, new_vs, counts) of densify_tensors against the yardstick: copies bit for bit, children within the bounds"""
    K, C, S = trd.plan_rows(plan)
    new_t, new_m, new_v, counts = got
    assert tuple(counts) == (K.size, C.size, S.size)
    ref_t, ref_m, ref_v = trd.apply(plan, tensors, roles, ms, vs, noise, raw=raw)
    first_child = K.size + C.size
    for k, (t, role) in enumerate(zip(new_t, roles)):
        assert tuple(t.shape) == ref_t[k].shape and t.dtype == torch.float32
        if role in (1, 2) and S.size:
            assert same_bits(t[:first_child], ref_t[k][:first_child].astype(np.float32))
        else:
            assert same_bits(t, ref_t[k].astype(np.float32))
        for new, ref in ((new_m[k], ref_m[k]), (new_v[k], ref_v[k])):
            assert (new is None) == (ref is None)
            if ref is not None:
                assert same_bits(new, ref.astype(np.float32))          # K rows bit for bit, everything else exactly zero
                assert not new[K.size:].any()
    if S.size:
        by_role = {r: np.asarray(t)[S] for t, r in zip(tensors, roles) if r}
        ex, es = trd.child_errors(new_t[roles.index(1)][first_child:].cpu().numpy(), new_t[roles.index(2)][first_child:].cpu().numpy(),
                                  by_role[1], by_role[2], by_role[3], noise, raw=raw)
        print(f"children: xyz ratio {ex:.3g} (bound {trd.CHILD_XYZ_BOUND:.3g}), scaling ratio {es:.3g} (bound {trd.CHILD_SCALING_BOUND:.3g})")
        assert ex <= trd.CHILD_XYZ_BOUND and es <= trd.CHILD_SCALING_BOUND


@pytest.mark.parametrize("P", trd.SIZES)
@pytest.mark.parametrize("offset_floats", [0, 1, 3])
def test_apply_model_rows_of_1_3_4_45_floats(P, offset_floats):
    """The six tensors of a 3DGS model (rows of 3, 3, 45, 1, 3 and 4 floats) with both moments, by the rule's plan; offset_floats: every
    input is a view that starts 4 or 12 bytes into its storage."""
    d, plan, _ = model(P)
    S = trd.plan_rows(plan)[2]
    noise = d["noise"][:2 * S.size]
    tensors, ms, vs = [d[n] for n in NAMES], [d["m_" + n] for n in NAMES], [d["v_" + n] for n in NAMES]
    up = lambda arrays: [dev(a, offset_floats) for a in arrays]
    got = dgr().densify_tensors(torch.from_numpy(plan).cuda(), up(tensors), [trd.ROLES.get(n, "plain") for n in NAMES], up(ms), up(vs), dev(noise))
    check_apply(plan, tensors, MODEL_ROLES, ms, vs, noise, got)


@pytest.mark.parametrize("P", [65, 4097])
def test_apply_not_raw_and_without_moments(P):
    d, plan, _ = model(P)
    S = trd.plan_rows(plan)[2]
    noise = d["noise"][:2 * S.size]
    act = dict(d, scaling=np.exp(d["scaling"].astype(np.float64)).astype(np.float32))
    tensors = [act[n] for n in NAMES]
    ms = [d["m_" + n] if n in ("xyz", "rotation") else None for n in NAMES]     # some tensors with state, some without
    vs = [d["v_" + n] if n in ("xyz", "rotation") else None for n in NAMES]
    up = lambda arrays: [None if a is None else dev(a) for a in arrays]
    got = dgr().densify_tensors(torch.from_numpy(plan).cuda(), up(tensors), MODEL_ROLES, up(ms), up(vs), dev(noise), raw=False)
    check_apply(plan, tensors, MODEL_ROLES, ms, vs, noise, got, raw=False)


HAND_PLANS = {
    "all-keep": lambda P: np.full(P, 1),
    "all-zero": lambda P: np.zeros(P),
    "no-split": lambda P: np.arange(P) % 4,
    "all-split": lambda P: np.full(P, 4),
    "every-value": lambda P: (np.arange(P) * 5 + 3) % 8,
    "high-bits-ignored": lambda P: ((np.arange(P) * 5 + 3) % 8) | 0xA8,
}


@pytest.mark.parametrize("P", [1, 65, 257])
@pytest.mark.parametrize("which", list(HAND_PLANS))
def test_apply_hand_written_plans_and_the_output_order(P, which):
    d = model(P)[0]
    plan = HAND_PLANS[which](P).astype(np.uint8)
    K, C, S = trd.plan_rows(plan)
    if P >= 65 and which in ("every-value", "high-bits-ignored"):
        assert set((plan & 7).tolist()) == set(range(8))
    noise = d["noise"][:2 * S.size]
    index = np.arange(P, dtype=np.float32)[:, None]                               # a plain tensor that names its source row
    tensors, roles = [d["xyz"], d["scaling"], d["rotation"], index, d["f_rest"]], [1, 2, 3, 0, 0]
    ms, vs = [d["m_xyz"], None, d["m_rotation"], index + 0.5, d["m_f_rest"]], [d["v_xyz"], None, d["v_rotation"], index + 0.25, d["v_f_rest"]]
    up = lambda arrays: [None if a is None else dev(a) for a in arrays]
    got = dgr().densify_tensors(torch.from_numpy(plan).cuda(), up(tensors), roles, up(ms), up(vs), None if which == "no-split" else dev(noise))
    check_apply(plan, tensors, roles, ms, vs, noise, got)
    M = K.size + C.size + 2 * S.size
    assert got[0][3][:, 0].cpu().tolist() == np.concatenate([K, C, S, S]).tolist() and got[0][4].shape == (M, 15, 3)   # K rows in index order, C rows, first children, second children
    if which == "all-zero":
        assert M == 0 and got[3] == (0, 0, 0) and all(t.numel() == 0 for t in got[0])
    if which == "no-split":
        got2 = dgr().densify_tensors(torch.from_numpy(plan).cuda(), up(tensors), roles, up(ms), up(vs), torch.empty(0, 3, device="cuda"))   # empty noise
        assert all(torch.equal(a, b) for a, b in zip(got[0], got2[0]))


def test_apply_more_than_eight_tensors():
    """Nine tensors: the packing loop's second launch.  The five of the hand-written plans and four more plain ones of 1, 2, 4 and 5 floats per
    row (one 16-byte path among them), two of them with moments and two without."""
    P = 257
    d = model(P)[0]
    plan = HAND_PLANS["every-value"](P).astype(np.uint8)
    S = trd.plan_rows(plan)[2]
    noise = d["noise"][:2 * S.size]
    index = np.arange(P, dtype=np.float32)[:, None]
    rng = np.random.default_rng(9)
    more = [rng.standard_normal((P, w)).astype(np.float32) for w in (1, 2, 4, 5)]
    more_m = [rng.standard_normal(t.shape).astype(np.float32) if k % 2 == 0 else None for k, t in enumerate(more)]
    more_v = [None if m is None else rng.uniform(0.5, 1.5, m.shape).astype(np.float32) for m in more_m]
    tensors, roles = [d["xyz"], d["scaling"], d["rotation"], index, d["f_rest"]] + more, [1, 2, 3, 0, 0, 0, 0, 0, 0]
    ms = [d["m_xyz"], None, d["m_rotation"], index + 0.5, d["m_f_rest"]] + more_m
    vs = [d["v_xyz"], None, d["v_rotation"], index + 0.25, d["v_f_rest"]] + more_v
    up = lambda arrays: [None if a is None else dev(a) for a in arrays]
    got = dgr().densify_tensors(torch.from_numpy(plan).cuda(), up(tensors), roles, up(ms), up(vs), dev(noise))
    assert len(got[0]) == 9
    check_apply(plan, tensors, roles, ms, vs, noise, got)


@pytest.mark.parametrize("P", [4097, 349_526])   # 349 526: the smallest P with ceil(3 P / 4096) = 257 tiles, a thread of the tile prefix owns two
def test_scan_offsets_and_counts(P):
    plan = ((np.arange(P) * 5 + 3) % 8).astype(np.uint8)
    offsets, counts = _C().densify_scan(torch.from_numpy(plan).cuda())
    K, C, S = trd.plan_rows(plan)
    assert counts == (K.size, C.size, S.size) and offsets.dtype == torch.int32 and offsets.shape == (3 * P,)
    flags = np.concatenate([plan & 1, (plan >> 1) & 1, (plan >> 2) & 1]).astype(np.int64)
    assert np.array_equal(offsets.cpu().numpy(), np.cumsum(flags) - flags)
    assert _C().densify_scan(torch.empty(0, dtype=torch.uint8, device="cuda"))[1] == (0, 0, 0)


def test_densify_tensors_draws_its_noise_and_refuses_a_split_without_roles():
    d, plan, _ = model(257)
    p = torch.from_numpy(plan).cuda()
    geo = [dev(d["xyz"]), dev(d["scaling"]), dev(d["rotation"])]
    torch.manual_seed(5)
    a = dgr().densify_tensors(p, geo, ["xyz", "scaling", "rotation"])
    torch.manual_seed(5)
    nS = a[3][2]
    b = dgr().densify_tensors(p, geo, ["xyz", "scaling", "rotation"], noise=torch.randn(2 * nS, 3, device="cuda"))
    assert nS > 0 and all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == [None] * 3
    with pytest.raises(RuntimeError, match="a split needs exactly one tensor of each of the roles"):
        dgr().densify_tensors(p, geo)
    with pytest.raises(RuntimeError, match="a split needs exactly one tensor of each of the roles"):
        dgr().densify_tensors(p, [geo[0], geo[1], dev(d["opacity"])], ["xyz", "scaling", "rotation"])


# ---- the optimizer -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["adam", "sparse"])
def test_densify_and_prune_on_a_six_group_optimizer(kind):
    """Parameters and state against the restatement of upstream's own sequence (float64, the same noise); the groups hold the new Parameters
    and a following step() runs."""
    P = 257
    d, plan, _ = model(P)
    K, C, S = trd.plan_rows(plan)
    noise = trd.split_noise(d["noise"], S)
    params = {n: torch.nn.Parameter(dev(d[n])) for n in NAMES}
    groups = [{"params": [params[n]], "lr": 1e-3, "name": n} for n in NAMES]
    opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15) if kind == "adam" else dgr().SparseGaussianAdam(groups, lr=0.0, eps=1e-15)
    with_state = [n for n in NAMES if n != "f_dc"]                                # one group whose state is still empty
    for n in with_state:
        opt.state[params[n]] = {"step": torch.tensor(3.0), "exp_avg": dev(d["m_" + n]), "exp_avg_sq": dev(d["v_" + n])}
    got_plan = dgr().densify_plan(dev(d["accum"]), dev(d["denom"]), params["scaling"], params["opacity"], None, **trd.RULE)
    new = dgr().densify_and_prune(opt, got_plan, noise=dev(noise))
    as64 = lambda prefix, names: {n: torch.from_numpy(d[prefix + n]).double() for n in names}
    ut, um, uv = trd.upstream_densify_and_prune(as64("", NAMES), as64("m_", with_state), as64("v_", with_state), d["accum"], d["denom"], d["noise"], **trd.RULE)
    M, first_child = K.size + C.size + 2 * S.size, K.size + C.size
    assert list(new) == NAMES and len(opt.state) == len(with_state)
    for group, n in zip(opt.param_groups, NAMES):
        p = group["params"][0]
        assert p is new[n] and isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf and p.shape == (M,) + d[n].shape[1:]
        want = ut[n].numpy()
        if n in ("xyz", "scaling"):
            assert same_bits(p[:first_child], want[:first_child].astype(np.float32))
        else:
            assert same_bits(p, want.astype(np.float32))
        if n in with_state:
            state = opt.state[p]
            assert float(state["step"]) == 3.0 and same_bits(state["exp_avg"], um[n].numpy().astype(np.float32)) and same_bits(state["exp_avg_sq"], uv[n].numpy().astype(np.float32))
        else:
            assert p not in opt.state
    # the children against upstream's, in the measures of the bounds
    s = np.exp(d["scaling"][S].astype(np.float64))
    s2, n64 = np.concatenate([s, s]), noise.astype(np.float64)
    ref_xyz, ref_sc = ut["xyz"].numpy()[first_child:], ut["scaling"].numpy()[first_child:]
    err = np.linalg.norm(new["xyz"].detach().cpu().numpy()[first_child:].astype(np.float64) - ref_xyz, axis=1)
    ulp = np.spacing(np.abs(ref_xyz).max(axis=1).astype(np.float32)).astype(np.float64)
    assert np.all(err <= trd.CHILD_XYZ_BOUND * s2.max(axis=1) * np.linalg.norm(n64, axis=1) + ulp)
    assert np.all(np.abs(new["scaling"].detach().cpu().numpy()[first_child:].astype(np.float64) - ref_sc) <= trd.CHILD_SCALING_BOUND * np.maximum(1.0, np.abs(ref_sc)))
    # a following step runs on the new tensors
    before = {n: new[n].detach().clone() for n in NAMES}
    for n in NAMES:
        new[n].grad = torch.ones_like(new[n])
    if kind == "adam":
        opt.step()
    else:
        opt.step(torch.ones(M, dtype=torch.bool, device="cuda"), M)
    torch.cuda.synchronize()
    assert all(not torch.equal(before[n], new[n].detach()) and torch.isfinite(new[n]).all() for n in NAMES)
    assert all(opt.state[new[n]]["exp_avg"].shape == new[n].shape for n in NAMES)
