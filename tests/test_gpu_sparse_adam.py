"""GPU tests of the fused sparse Adam step (SparseGaussianAdam, _C.sparse_adam, _C.adamUpdate; include/stp_raster.h: stp_sparse_adam) against
the float64 yardstick tests/torch_ref_sparse_adam.py.

Visible rows are held to bounds counted from float32 roundings (torch_ref_sparse_adam.bounds), invisible rows to bit equality.  The kernel's
work unit holds U = 4096 elements and a thread owns 16-byte pieces: the shapes are the smallest with element counts that are no multiple of
four, rows that straddle pieces and units, more than one and more than two units, and tensors that start 4 bytes into their storage."""
import copy

import numpy as np
import pytest
import torch

import torch_ref_sparse_adam as tra

pytestmark = pytest.mark.gpu

U = 4096   # elements of the kernel's work unit (csrc/stp_adam.hip: ADAM_UNIT)
HYPER = [(1.6e-4, 1e-15), (5e-2, 1e-8)]
TRAINER_SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}


def _C():
    from diff_gaussian_rasterization import _C as c
    return c


def make_inputs(N, shape, seed):
    """p, g, m, v as float32 arrays (N, *shape): |g| and |m| are 0 or in [1e-8, 1], v is 0 or in [1e-16, 1] (log-uniform) -- no denormals,
    no underflow of g * g in a comparison that is relative.  5 % of the elements have m = v = 0, half of those g = 0 as well (0 / (0 + eps):
    a step of exactly 0); 10 % of g are zeros in all."""
    rng = np.random.default_rng(seed)
    full = (N,) + tuple(shape)
    logu = lambda lo: 10.0 ** rng.uniform(lo, 0.0, full)
    sign = lambda: rng.choice([-1.0, 1.0], full)
    u = rng.random(full)
    g = np.where((u < 0.025) | ((u >= 0.05) & (u < 0.125)), 0.0, sign() * logu(-8)).astype(np.float32)
    m = np.where(u < 0.05, 0.0, sign() * logu(-8)).astype(np.float32)
    v = np.where(u < 0.05, 0.0, logu(-16)).astype(np.float32)
    p = (sign() * logu(-3) * 10.0).astype(np.float32)
    for a, lo in ((g, 1e-8), (m, 1e-8), (v, 1e-16)):
        nz = np.abs(a[a != 0])
        assert nz.size == 0 or (nz.min() >= np.float32(lo) * 0.999 and nz.max() <= 1.0)
    return p, g, m, v


def visibilities(N, seed):
    """(name, tensor-ready array): random at 50 %, all false, all true -- each as bool and as int32 radii with negatives, zeros and positives"""
    rng = np.random.default_rng(seed)
    out = []
    for name, mask in (("half", rng.random(N) < 0.5), ("none", np.zeros(N, bool)), ("all", np.ones(N, bool))):
        radii = np.where(mask, rng.integers(1, 500, N), -rng.integers(0, 3, N)).astype(np.int32)   # invisible: 0, -1, -2
        out += [(name + "-bool", mask), (name + "-radii", radii)]
    return out


def dev(a, offset_floats=0):
    """A contiguous cuda tensor of the array's values; offset_floats = 1: a view that starts 4 bytes into its storage."""
    a = np.ascontiguousarray(a)
    if offset_floats == 0 or a.dtype != np.float32:
        return torch.from_numpy(a).cuda()
    base = torch.empty(a.size + offset_floats, dtype=torch.float32, device="cuda")
    t = base[offset_floats:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * offset_floats
    return t


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def check(label, got, inputs, visible, lr, eps, b1=0.9, b2=0.999):
    """got = (p, m, v) float32 arrays after the kernel; inputs = (p, g, m, v) before it.  Visible rows within the bounds, invisible rows bit-equal;
    an element with g = m = v = 0 takes a step of exactly 0.  Returns the worst error / bound per quantity."""
    p, g, m, v = inputs
    rows = tra.visible_rows(visible)
    p_ref, m_ref, v_ref = tra.step(p, g, m, v, visible, lr, eps, b1, b2)
    bm, bv, bp = tra.bounds(g, m, visible, v_ref, p, lr, eps, b1, b2)
    worst = []
    for name, k, ref, bound, before in (("m", got[1], m_ref, bm, m), ("v", got[2], v_ref, bv, v), ("p", got[0], p_ref, bp, p)):
        assert np.array_equal(k[~rows].view(np.int32), before[~rows].view(np.int32)), f"{label}: {name} of an invisible row changed"
        err = np.abs(k[rows].astype(np.float64) - ref[rows])
        assert np.all(np.isfinite(k[rows])), f"{label}: {name} not finite"
        ok = err <= bound[rows]
        ratio = float(np.max(np.where(bound[rows] > 0, err / np.where(bound[rows] > 0, bound[rows], 1.0), np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
        worst.append(ratio)
        assert np.all(ok), f"{label}: {name} worst error / bound {ratio:.3g} at {int(np.sum(~ok))} of {ok.size} elements"
    still = rows.reshape((-1,) + (1,) * (p.ndim - 1)) & (g == 0) & (m == 0) & (v == 0)
    assert np.array_equal(got[0][still].view(np.int32), p[still].view(np.int32)), f"{label}: 0 / (0 + eps) moved p"
    return worst


def run(inputs, visible, lr, eps, N, offset_floats=0, b1=0.9, b2=0.999):
    """One _C.sparse_adam call on fresh device copies; returns ((p, m, v) as float32 arrays, launches)."""
    p, g, m, v = (dev(a, offset_floats) for a in inputs)
    launches = _C().sparse_adam([p], [g], [m], [v], dev(visible), [lr], [eps], b1, b2, N)
    return tuple(t.cpu().numpy() for t in (p, m, v)), launches


SINGLE = [(M, N) for M in (1, 3, 4, 45, 7) for N in (1, 3, 67, 1031)] + [(45, 92), (45, 183)]   # 45 * 92 = U + 44, 45 * 183 = 2 U + 43


@pytest.mark.parametrize("M, N", SINGLE)
def test_single_tensor(M, N):
    inputs = make_inputs(N, (M,), seed=1000 * M + N)
    worst = [0.0, 0.0, 0.0]
    for name, visible in visibilities(N, seed=N):
        for lr, eps in HYPER:
            got, launches = run(inputs, visible, lr, eps, N)
            assert launches == 1
            w = check(f"M={M} N={N} {name} lr={lr}", got, inputs, visible, lr, eps)
            worst = [max(a, b) for a, b in zip(worst, w)]
    print(f"\nM={M} N={N}: worst error / bound  m {worst[0]:.2f}  v {worst[1]:.2f}  p {worst[2]:.2f}")


def test_unaligned_tensors_take_the_scalar_path():
    M, N = 3, 67
    inputs = make_inputs(N, (M,), seed=5)
    for name, visible in visibilities(N, seed=6):
        for lr, eps in HYPER:
            got, _ = run(inputs, visible, lr, eps, N, offset_floats=1)
            check(f"unaligned {name} lr={lr}", got, inputs, visible, lr, eps)
            aligned, _ = run(inputs, visible, lr, eps, N)
            for a, b in zip(got, aligned):   # the same arithmetic on both paths
                assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # one unaligned pointer of the four is enough to leave the 16-byte path
    p, g, m, v = (dev(a) for a in inputs)
    g1 = dev(inputs[1], 1)
    visible = visibilities(N, seed=6)[0][1]
    _C().sparse_adam([p], [g1], [m], [v], dev(visible), [1e-3], [1e-15], 0.9, 0.999, N)
    check("unaligned grad", tuple(t.cpu().numpy() for t in (p, m, v)), inputs, visible, 1e-3, 1e-15)


@pytest.mark.parametrize("M, N", [(3, 67), (45, 183), (1, 1031)])
def test_invisible_rows_keep_their_bits(M, N):
    p0, g0, m0, v0 = make_inputs(N, (M,), seed=77 + M)
    rng = np.random.default_rng(3)
    for name, visible in visibilities(N, seed=8):
        rows = tra.visible_rows(visible)
        g = g0.copy()
        g[~rows] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), (int(np.sum(~rows)), M))   # never used
        for offset in (0, 1):
            p, gt, m, v = (dev(a, offset) for a in (p0, g, m0, v0))
            clones = [t.clone() for t in (p, m, v)]
            _C().sparse_adam([p], [gt], [m], [v], dev(visible), [5e-2], [1e-8], 0.9, 0.999, N)
            sel = torch.from_numpy(~rows).cuda()
            for t, c in zip((p, m, v), clones):
                assert torch.equal(bits(t)[sel], bits(c)[sel]), f"{name}: an invisible row changed"
                if not rows.any():
                    assert torch.equal(bits(t), bits(c)), f"{name}: nothing visible, yet a tensor changed"
            check(f"nan-grads {name} offset={offset}", tuple(t.cpu().numpy() for t in (p, m, v)), (p0, g0, m0, v0), visible, 5e-2, 1e-8)


def test_non_finite_gradients_of_visible_rows_propagate():
    N, M = 8, 3
    p0, g0, m0, v0 = make_inputs(N, (M,), seed=9)
    g0[2, 1], g0[5, 0] = np.nan, np.inf
    visible = np.ones(N, bool)
    p, g, m, v = (dev(a) for a in (p0, g0, m0, v0))
    _C().sparse_adam([p], [g], [m], [v], dev(visible), [1e-3], [1e-15], 0.9, 0.999, N)
    p, m, v = (t.cpu().numpy() for t in (p, m, v))
    assert np.isnan(p[2, 1]) and np.isnan(m[2, 1]) and np.isnan(v[2, 1])
    assert np.isinf(m[5, 0]) and np.isinf(v[5, 0]) and np.isnan(p[5, 0])   # inf / (inf + eps)
    ok = np.ones((N, M), bool)
    ok[2, 1] = ok[5, 0] = False
    p_ref, m_ref, v_ref = tra.step(p0, g0, m0, v0, visible, 1e-3, 1e-15)
    bm, bv, bp = tra.bounds(g0, m0, visible, v_ref, p0, 1e-3, 1e-15)
    assert np.all(np.abs(p[ok] - p_ref[ok]) <= bp[ok]) and np.all(np.abs(m[ok] - m_ref[ok]) <= bm[ok]) and np.all(np.abs(v[ok] - v_ref[ok]) <= bv[ok])


@pytest.mark.parametrize("M, N", [(45, 183), (7, 1031)])
def test_three_steps_in_a_row(M, N):
    """State carried on the device; every step is held against the yardstick stepped from the kernel's own previous state."""
    p0, _, m0, v0 = make_inputs(N, (M,), seed=21)
    p, m, v = dev(p0), dev(np.zeros_like(m0)), dev(np.zeros_like(v0))   # a fresh optimizer state
    vis = visibilities(N, seed=22)
    for k, (name, visible) in enumerate((vis[0], vis[1], (vis[0][0], ~vis[0][1]))):
        lr, eps = HYPER[k % 2]
        g = make_inputs(N, (M,), seed=30 + k)[1]
        before = (p.cpu().numpy(), g, m.cpu().numpy(), v.cpu().numpy())
        _C().sparse_adam([p], [dev(g)], [m], [v], dev(visible), [lr], [eps], 0.9, 0.999, N)
        check(f"step {k}", tuple(t.cpu().numpy() for t in (p, m, v)), before, visible, lr, eps)


def make_optimizer(N, names, seed, lrs=None, without_grad=()):
    import diff_gaussian_rasterization as dgr
    groups, data = [], {}
    for i, name in enumerate(names):
        shape = TRAINER_SHAPES[name.split("#")[0]]
        p0, g0, _, _ = make_inputs(N, shape, seed=seed + i)
        param = torch.nn.Parameter(dev(p0))
        if name not in without_grad:
            param.grad = dev(g0)
        groups.append({"params": [param], "lr": (lrs or {}).get(name, 1e-3 * (i + 1)), "name": name})
        data[name] = (p0, g0)
    return dgr.SparseGaussianAdam(groups, lr=0.0, eps=1e-15), data


def group_of(opt, name):
    return next(g for g in opt.param_groups if g["name"] == name)


def test_class_six_groups_one_launch():
    N = 1031
    names = list(TRAINER_SHAPES) + ["xyz#frozen"]
    opt, data = make_optimizer(N, names, seed=40, without_grad=("xyz#frozen",))
    frozen = group_of(opt, "xyz#frozen")["params"][0]
    frozen_before = frozen.detach().clone()
    radii = visibilities(N, seed=41)[1][1]   # the forward's int32 radii, as the example passes them
    # two steps: the first from the zero state the class creates, the second from the state it carried
    for k in range(2):
        before = {n: (group_of(opt, n)["params"][0].detach().cpu().numpy(), data[n][1],
                      opt.state[group_of(opt, n)["params"][0]]["exp_avg"].cpu().numpy() if k else np.zeros_like(data[n][0]),
                      opt.state[group_of(opt, n)["params"][0]]["exp_avg_sq"].cpu().numpy() if k else np.zeros_like(data[n][0])) for n in TRAINER_SHAPES}
        assert opt.step(dev(radii), N) is None
        assert opt.last_launches == 1
        for i, n in enumerate(TRAINER_SHAPES):
            param = group_of(opt, n)["params"][0]
            st = opt.state[param]
            assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == k + 1
            assert st["exp_avg"].shape == param.shape and st["exp_avg_sq"].dtype == torch.float32
            got = (param.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy())
            check(f"{n} step {k}", got, before[n], radii, 1e-3 * (i + 1), 1e-15)   # (its own lr: a different one in every group)
    assert frozen not in opt.state and torch.equal(bits(frozen), bits(frozen_before))
    # a schedule writes group["lr"]: honoured by the next step
    g = group_of(opt, "xyz")
    g["lr"] = 0.0
    p_before = g["params"][0].detach().clone()
    opt.step(dev(radii), N)
    assert torch.equal(bits(g["params"][0]), bits(p_before))


def test_class_nine_groups_two_launches():
    N = 67
    names = list(TRAINER_SHAPES) + ["xyz#2", "opacity#2", "f_rest#2"]
    opt, data = make_optimizer(N, names, seed=50)
    visible = visibilities(N, seed=51)[0][1]
    opt.step(dev(visible), N)
    assert opt.last_launches == 2
    for i, n in enumerate(names):
        param = group_of(opt, n)["params"][0]
        st = opt.state[param]
        zero = np.zeros_like(data[n][0])
        check(n, (param.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()), (data[n][0], data[n][1], zero, zero), visible,
              1e-3 * (i + 1), 1e-15)


def test_class_after_the_trainers_densification_moves():
    """cat_tensors_to_optimizer / _prune_optimizer of a 3DGS trainer: a longer Parameter under a new key with the state concatenated, then a
    mask over the rows; the step at the new N matches the yardstick."""
    N = 67
    opt, _ = make_optimizer(N, list(TRAINER_SHAPES), seed=60)
    opt.step(dev(np.ones(N, bool)), N)
    extra = 25
    keep = torch.from_numpy(np.random.default_rng(61).random(N + extra) < 0.7).cuda()
    for group in opt.param_groups:
        old = group["params"][0]
        stored = opt.state.pop(old)
        new_rows = torch.full((extra,) + tuple(old.shape[1:]), 0.25, device="cuda")
        stored["exp_avg"] = torch.cat((stored["exp_avg"], torch.zeros_like(new_rows)), dim=0)
        stored["exp_avg_sq"] = torch.cat((stored["exp_avg_sq"], torch.zeros_like(new_rows)), dim=0)
        group["params"][0] = torch.nn.Parameter(torch.cat((old.detach(), new_rows), dim=0))
        opt.state[group["params"][0]] = stored
    for group in opt.param_groups:   # prune
        old = group["params"][0]
        stored = opt.state.pop(old)
        stored["exp_avg"], stored["exp_avg_sq"] = stored["exp_avg"][keep], stored["exp_avg_sq"][keep]
        group["params"][0] = torch.nn.Parameter(old.detach()[keep])
        opt.state[group["params"][0]] = stored
    N2 = int(keep.sum())
    assert N2 != N
    visible = visibilities(N2, seed=62)[0][1]
    before = {}
    for i, group in enumerate(opt.param_groups):
        param = group["params"][0]
        g = make_inputs(N2, param.shape[1:], seed=70 + i)[1]
        param.grad = dev(g)
        before[group["name"]] = (param.detach().cpu().numpy(), g, opt.state[param]["exp_avg"].cpu().numpy(), opt.state[param]["exp_avg_sq"].cpu().numpy())
    opt.step(dev(visible), N2)
    assert opt.last_launches == 1
    for i, group in enumerate(opt.param_groups):
        param = group["params"][0]
        st = opt.state[param]
        check(group["name"], (param.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()), before[group["name"]], visible,
              1e-3 * (i + 1), 1e-15)
        assert float(st["step"]) == 2


def test_class_state_dict_round_trip():
    import diff_gaussian_rasterization as dgr
    N = 67
    opt, _ = make_optimizer(N, list(TRAINER_SHAPES), seed=80)
    visible = dev(visibilities(N, seed=81)[0][1])
    opt.step(visible, N)
    fresh = dgr.SparseGaussianAdam([{"params": [torch.nn.Parameter(g["params"][0].detach().clone())], "lr": 123.0, "name": g["name"]} for g in opt.param_groups],
                                   lr=0.0, eps=1e-3)
    fresh.load_state_dict(copy.deepcopy(opt.state_dict()))   # (as through torch.save / torch.load: load_state_dict itself keeps the tensors it is given)
    assert [g["lr"] for g in fresh.param_groups] == [g["lr"] for g in opt.param_groups] and all(g["eps"] == 1e-15 for g in fresh.param_groups)
    for a, b in zip(opt.param_groups, fresh.param_groups):
        b["params"][0].grad = a["params"][0].grad.clone()
    other = dev(visibilities(N, seed=82)[0][1])
    opt.step(other, N)
    fresh.step(other, N)
    for a, b in zip(opt.param_groups, fresh.param_groups):
        pa, pb = a["params"][0], b["params"][0]
        assert torch.equal(bits(pa), bits(pb))
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(bits(opt.state[pa][key]), bits(fresh.state[pb][key]))
        assert float(opt.state[pa]["step"]) == float(fresh.state[pb]["step"]) == 2


def test_equal_inputs_give_equal_bits():
    N, M = 1031, 45
    inputs = make_inputs(N, (M,), seed=90)
    visible = visibilities(N, seed=91)[0][1]
    a, _ = run(inputs, visible, 1.6e-4, 1e-15, N)
    b, _ = run(inputs, visible, 1.6e-4, 1e-15, N)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))


def test_upstream_name_and_argument_order():
    N, M = 67, 45
    inputs = make_inputs(N, (M,), seed=95)
    visible = visibilities(N, seed=96)[0][1]
    want, _ = run(inputs, visible, 1.6e-4, 1e-15, N)
    p, g, m, v = (dev(a) for a in inputs)
    assert _C().adamUpdate(p, g, m, v, dev(visible), 1.6e-4, 0.9, 0.999, 1e-15, N, M) is None
    for x, y in zip((p, m, v), want):
        assert np.array_equal(x.cpu().numpy().view(np.int32), y.view(np.int32))
    with pytest.raises(RuntimeError, match="N \\* M"):
        _C().adamUpdate(p, g, m, v, dev(visible), 1.6e-4, 0.9, 0.999, 1e-15, N, M + 1)


def test_binding_refuses_what_it_cannot_update_in_place():
    N = 8
    z = lambda *shape: torch.zeros(*shape, device="cuda")
    vis = torch.ones(N, dtype=torch.bool, device="cuda")
    call = lambda p, g, m, v, visible=vis, n=N: _C().sparse_adam([p], [g], [m], [v], visible, [1e-3], [1e-15], 0.9, 0.999, n)
    with pytest.raises(RuntimeError, match="expected float32"):
        call(z(N, 3).double(), z(N, 3), z(N, 3), z(N, 3))
    with pytest.raises(RuntimeError, match="must be contiguous"):
        call(z(3, N).t(), z(N, 3), z(N, 3), z(N, 3))
    with pytest.raises(RuntimeError, match="has shape"):
        call(z(N, 3), z(N, 4), z(N, 3), z(N, 3))
    with pytest.raises(RuntimeError, match="visible must be bool, uint8 or int32"):
        call(z(N, 3), z(N, 3), z(N, 3), z(N, 3), visible=vis.float())
    with pytest.raises(RuntimeError, match="visible must be contiguous with N = 8 elements"):
        call(z(N, 3), z(N, 3), z(N, 3), z(N, 3), visible=vis[:5])
    with pytest.raises(RuntimeError, match="not a multiple of N"):
        call(z(5, 3), z(5, 3), z(5, 3), z(5, 3))   # 15 elements, N = 8
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(z(N, 3), z(N, 3).cpu(), z(N, 3), z(N, 3))
    # uint8 is read like bool; N == 0 and tensors without elements launch nothing
    p = torch.ones(N, 3, device="cuda")
    assert call(p, torch.ones(N, 3, device="cuda"), z(N, 3), z(N, 3), visible=vis.to(torch.uint8) * 7) == 1 and bool((p != 1).all())
    assert call(z(0, 3), z(0, 3), z(0, 3), z(0, 3), visible=vis[:0], n=0) == 0


def test_the_largest_tensor_is_indexed_exactly():
    """numel = N = 2^31 - 1 (the largest the C ABI takes; odd, so the last three elements are the tensor's tail): a handful of visible rows
    at the start, around 2^30 and at the very end change, to the bits a ten-element call gives, and nothing else does."""
    N = 2 ** 31 - 1
    rows = torch.tensor([0, 1, 5, 2 ** 30 - 1, 2 ** 30, 2 ** 30 + 3, N - 4, N - 3, N - 2, N - 1], device="cuda")
    fills = (1.0, 2.0, 0.5, 0.25)
    p, g, m, v = (torch.full((N,), x, device="cuda") for x in fills)
    visible = torch.zeros(N, dtype=torch.uint8, device="cuda")
    visible[rows] = 1
    assert _C().sparse_adam([p], [g], [m], [v], visible, [5e-2], [1e-8], 0.9, 0.999, N) == 1
    small = [torch.full((len(rows),), x, device="cuda") for x in fills]
    _C().sparse_adam([small[0]], [small[1]], [small[2]], [small[3]], torch.ones(len(rows), dtype=torch.bool, device="cuda"), [5e-2], [1e-8], 0.9, 0.999, len(rows))
    for t, s, x in ((p, small[0], 1.0), (m, small[2], 0.5), (v, small[3], 0.25)):
        assert float(s[0]) != x
        assert torch.equal(bits(t[rows]), bits(s))
        assert int((t != x).sum()) == len(rows)
