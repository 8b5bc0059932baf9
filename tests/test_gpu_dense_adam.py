"""GPU tests of the fused dense Adam step (GaussianAdam, _C.dense_adam; include/stp_raster.h: stp_dense_adam) against the float64 yardstick
tests/torch_ref_dense_adam.py, every element inside bounds counted from float32 roundings.

The kernel's work unit holds U = 4096 elements and a thread owns 16-byte pieces: the element counts are the unit and piece edges, the shapes
the trainers' six, and one tensor starts 4 bytes into its storage."""
import copy

import numpy as np
import pytest
import torch

import torch_ref_dense_adam as trd

pytestmark = pytest.mark.gpu

U = 4096   # elements of the kernel's work unit (csrc/stp_adam.hip: ADAM_UNIT)
HYPER = [(1.6e-4, 1e-15), (5e-2, 1e-8)]
STEPS = (1, 2, 10, 1000)
TRAINER_SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
TRAINER_LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 2.5e-2, "scaling": 5e-3, "rotation": 1e-3}
REGS = {"opacity": ("sigmoid", 0.01), "scaling": ("exp", 0.01)}


def _C():
    from diff_gaussian_rasterization import _C as c
    return c


def dgr():
    import diff_gaussian_rasterization as d
    return d


def dev(a, offset_floats=0):
    """A contiguous cuda tensor of the array's values; offset_floats = 1: a view that starts 4 bytes into its storage."""
    a = np.ascontiguousarray(a)
    if offset_floats == 0:
        return torch.from_numpy(a).cuda()
    base = torch.empty(a.size + offset_floats, dtype=torch.float32, device="cuda")
    t = base[offset_floats:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * offset_floats
    return t


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def worst_ratio(err, bound):
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0


def check(label, got, inputs, lr, eps, t, b1=0.9, b2=0.999, reg=None):
    """got = (p, m, v) float32 arrays after the kernel; inputs = (p, g, m, v) before it.  Every element within the bounds; an element with
    g' = m = v = 0 takes a step of exactly 0.  Returns the worst error / bound per quantity."""
    p, g, m, v = inputs
    p_ref, m_ref, v_ref = trd.step(p, g, m, v, lr, eps, t, b1, b2, reg)
    bm, bv, bp, _ = trd.bounds(p, g, m, v, lr, eps, t, b1, b2, reg)
    worst = []
    for name, k, ref, bound in (("m", got[1], m_ref, bm), ("v", got[2], v_ref, bv), ("p", got[0], p_ref, bp)):
        assert np.all(np.isfinite(k)), f"{label}: {name} not finite"
        err = np.abs(k.astype(np.float64) - ref)
        worst.append(worst_ratio(err, bound))
        assert np.all(err <= bound), f"{label}: {name} worst error / bound {worst[-1]:.3g} at {int(np.sum(err > bound))} of {err.size} elements"
    if reg is None:
        still = (g == 0) & (m == 0) & (v == 0)
        assert np.array_equal(got[0][still].view(np.int32), p[still].view(np.int32)), f"{label}: 0 / (0 + eps) moved p"
    return worst


def run(inputs, lr, eps, t, offset_floats=0, b1=0.9, b2=0.999, reg=None):
    """One _C.dense_adam call of step t on fresh device copies; returns ((p, m, v) as float32 arrays, launches)."""
    p, g, m, v = (dev(a, offset_floats) for a in inputs)
    g_before = g.clone()
    kind, weight = reg if reg is not None else (None, 0.0)
    coefs = [_C().dense_adam_coefficients(lr, b1, b2, eps, t, weight, p.numel())]
    launches = _C().dense_adam([p], [g], [m], [v], coefs, [_C().DENSE_ADAM_REG_KINDS[kind]])
    assert same_bits(g, g_before), "the gradient was written"
    return tuple(host(x) for x in (p, m, v)), launches


@pytest.mark.parametrize("numel", [1, 3, 4, 7, U - 1, U, U + 1, 2 * U + 43])
def test_single_tensor(numel):
    inputs = trd.make_inputs((numel,), seed=numel)
    fresh = (inputs[0], inputs[1], np.zeros_like(inputs[2]), np.zeros_like(inputs[3]))
    worst = [0.0, 0.0, 0.0]
    for t in STEPS:
        for lr, eps in HYPER:
            case = fresh if t == 1 else inputs   # (the first step starts from the zero state)
            got, launches = run(case, lr, eps, t)
            assert launches == 1
            w = check(f"numel={numel} t={t} lr={lr}", got, case, lr, eps, t)
            worst = [max(a, b) for a, b in zip(worst, w)]
    print(f"\nnumel={numel}: worst error / bound  m {worst[0]:.2f}  v {worst[1]:.2f}  p {worst[2]:.2f}")


@pytest.mark.parametrize("P", [67, 1031])
def test_regularisers(P):
    """"sigmoid" on (P, 1), "exp" on (P, 3), |p| log-uniform up to 16 with both signs (a saturated sigmoid on either side), weight 0.01; through
    the class, two steps, .grad bit-unchanged."""
    worst = [0.0, 0.0, 0.0]
    for name, shape in (("opacity", (P, 1)), ("scaling", (P, 3))):
        reg = REGS[name]
        for lr, eps in HYPER:
            p0, g0, _, _ = trd.make_inputs(shape, seed=P + len(name), p_log_uniform_to=16.0)
            assert np.abs(p0).max() > 12 and (p0 > 8).any() and (p0 < -8).any()
            param = torch.nn.Parameter(dev(p0))
            opt = dgr().GaussianAdam([{"params": [param], "lr": lr, "name": name}], lr=0.0, eps=eps)
            opt.set_regularizer(name, *reg)
            plain = torch.nn.Parameter(dev(p0))   # the same step without the regulariser differs
            plain.grad = dev(g0)
            other = dgr().GaussianAdam([{"params": [plain], "lr": lr, "name": name}], lr=0.0, eps=eps)
            other.step()
            for k in (1, 2):
                g = trd.make_inputs(shape, seed=P + 10 * k)[1]
                param.grad = dev(g)
                st = opt.state[param] if param in opt.state else None
                before = (host(param), g, host(st["exp_avg"]) if st else np.zeros_like(p0), host(st["exp_avg_sq"]) if st else np.zeros_like(p0))
                opt.step()
                assert opt.last_launches == 1 and same_bits(param.grad, dev(g)), "the gradient was written"
                st = opt.state[param]
                w = check(f"{name} P={P} lr={lr} step {k}", (host(param), host(st["exp_avg"]), host(st["exp_avg_sq"])), before, lr, eps, k, reg=reg)
                worst = [max(a, b) for a, b in zip(worst, w)]
                if k == 1:
                    assert not same_bits(st["exp_avg"], other.state[plain]["exp_avg"])
    print(f"\nregularisers P={P}: worst error / bound  m {worst[0]:.2f}  v {worst[1]:.2f}  p {worst[2]:.2f}")


def test_unaligned_tensors_take_the_narrow_path_with_equal_bits():
    for numel, reg in ((2 * U + 43, None), (1031, ("sigmoid", 0.01)), (3 * 67, ("exp", 0.01))):
        inputs = trd.make_inputs((numel,), seed=5 + numel, p_log_uniform_to=16.0 if reg else None)
        for lr, eps in HYPER:
            got, _ = run(inputs, lr, eps, 10, offset_floats=1, reg=reg)
            check(f"unaligned numel={numel} lr={lr}", got, inputs, lr, eps, 10, reg=reg)
            aligned, _ = run(inputs, lr, eps, 10, reg=reg)
            for a, b in zip(got, aligned):   # the same arithmetic on both paths
                assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # one unaligned pointer of the four is enough to leave the 16-byte path
    inputs = trd.make_inputs((U + 5,), seed=6)
    p, g, m, v = (dev(a) for a in inputs)
    g1 = dev(inputs[1], 1)
    _C().dense_adam([p], [g1], [m], [v], [_C().dense_adam_coefficients(1e-3, 0.9, 0.999, 1e-15, 3)], [0])
    aligned, _ = run(inputs, 1e-3, 1e-15, 3)
    for a, b in zip((p, m, v), aligned):
        assert np.array_equal(host(a).view(np.int32), b.view(np.int32))


def make_optimizer(N, names, seed, without_grad=(), empty=(), regs=None, cls=None, **group_options):
    """One group per name, the trainers' shapes and learning rates; -> (optimizer, {name: (p0, g0)})"""
    groups, data = [], {}
    for i, name in enumerate(names):
        shape = (0 if name in empty else N,) + TRAINER_SHAPES[name.split("#")[0]]
        p0, g0, _, _ = trd.make_inputs(shape, seed=seed + i)
        param = torch.nn.Parameter(dev(p0))
        if name not in without_grad:
            param.grad = dev(g0)
        groups.append({"params": [param], "lr": TRAINER_LRS[name.split("#")[0]], "name": name, **group_options.get(name, {})})
        data[name] = (p0, g0)
    opt = (cls or dgr().GaussianAdam)(groups, lr=0.0, eps=1e-15)
    for name, reg in (regs or {}).items():
        opt.set_regularizer(name, *reg)
    return opt, data


def group_of(opt, name):
    return next(g for g in opt.param_groups if g["name"] == name)


def check_group(opt, name, data, t, reg=None, b1=0.9, b2=0.999, before=None):
    param = group_of(opt, name)["params"][0]
    st = opt.state[param]
    zero = np.zeros_like(data[name][0])
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == t and st["step"].device.type == "cpu" and st["step"].dtype == torch.float32
    check(name, (host(param), host(st["exp_avg"]), host(st["exp_avg_sq"])), before or (data[name][0], data[name][1], zero, zero),
          group_of(opt, name)["lr"], group_of(opt, name)["eps"], t, b1, b2, reg)


def test_nine_tensors_two_launches_and_what_is_skipped():
    N = 67
    names = list(TRAINER_SHAPES) + ["xyz#2", "opacity#2", "f_rest#2", "xyz#frozen", "scaling#empty"]
    opt, data = make_optimizer(N, names, seed=50, without_grad=("xyz#frozen",), empty=("scaling#empty",))
    frozen = group_of(opt, "xyz#frozen")["params"][0]
    frozen_before = frozen.detach().clone()
    assert opt.step() is None
    assert opt.last_launches == 2   # nine tensors with elements
    for n in names[:9]:
        check_group(opt, n, data, 1)
    assert frozen not in opt.state and same_bits(frozen, frozen_before)
    empty = group_of(opt, "scaling#empty")["params"][0]
    assert empty.numel() == 0 and empty.grad is not None and empty not in opt.state   # (a tensor without elements: skipped like one without a gradient)
    marker = {"step": torch.tensor(4.0), "exp_avg": torch.zeros_like(empty), "exp_avg_sq": torch.zeros_like(empty)}
    opt.state[empty] = marker
    opt.state[frozen] = {"step": torch.tensor(9.0), "exp_avg": torch.full_like(frozen, 0.5), "exp_avg_sq": torch.full_like(frozen, 0.25)}
    opt.step()
    assert opt.last_launches == 2 and opt.state[empty] is marker and float(marker["step"]) == 4.0   # (a state they have is untouched)
    assert float(opt.state[frozen]["step"]) == 9.0 and bool((opt.state[frozen]["exp_avg"] == 0.5).all()) and same_bits(frozen, frozen_before)
    # a schedule writes group["lr"]: honoured by the next step
    g = group_of(opt, "xyz")
    g["lr"] = 0.0
    p_before = g["params"][0].detach().clone()
    opt.step()
    assert same_bits(g["params"][0], p_before) and float(opt.state[g["params"][0]]["step"]) == 3


def test_groups_with_their_own_betas_and_a_group_of_two_tensors():
    N = 1031
    a0, ga, _, _ = trd.make_inputs((N, 3), seed=60)
    b0, gb, _, _ = trd.make_inputs((N, 4), seed=61)
    c0, gc, _, _ = trd.make_inputs((N, 1), seed=62, p_log_uniform_to=16.0)
    pa, pb, pc = (torch.nn.Parameter(dev(x)) for x in (a0, b0, c0))
    opt = dgr().GaussianAdam([{"params": [pa, pb], "lr": 1e-3, "name": "pair"}, {"params": [pc], "lr": 5e-2, "betas": (0.8, 0.99), "eps": 1e-8, "name": "opacity"}],
                             lr=0.0, eps=1e-15)
    opt.set_regularizer("opacity", "sigmoid", 0.01)
    state = {id(p): (np.zeros_like(x), np.zeros_like(x)) for p, x in ((pa, a0), (pb, b0), (pc, c0))}
    for t in (1, 2, 3):
        before = {}
        for i, (p, shape) in enumerate(((pa, (N, 3)), (pb, (N, 4)), (pc, (N, 1)))):
            g = trd.make_inputs(shape, seed=70 + 10 * t + i)[1]
            p.grad = dev(g)
            before[id(p)] = (host(p), g) + state[id(p)]
        opt.step()
        assert opt.last_launches == 1
        for p, (lr, eps, b1, b2, reg) in ((pa, (1e-3, 1e-15, 0.9, 0.999, None)), (pb, (1e-3, 1e-15, 0.9, 0.999, None)), (pc, (5e-2, 1e-8, 0.8, 0.99, ("sigmoid", 0.01)))):
            st = opt.state[p]
            assert float(st["step"]) == t
            got = (host(p), host(st["exp_avg"]), host(st["exp_avg_sq"]))
            check(f"step {t}", got, before[id(p)], lr, eps, t, b1, b2, reg)
            state[id(p)] = got[1:]


def test_equal_inputs_give_equal_bits():
    for shape, reg in (((1031, 15, 3), None), ((1031, 3), ("exp", 0.01))):
        inputs = trd.make_inputs(shape, seed=90)
        a, _ = run(inputs, 1.6e-4, 1e-15, 7, reg=reg)
        b, _ = run(inputs, 1.6e-4, 1e-15, 7, reg=reg)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.int32), y.view(np.int32))


def test_five_steps_as_a_drop_in_for_torch_adam():
    """The trainers' six tensors at P = 1031, the two regularisers on: five GaussianAdam steps, the same five with torch.optim.Adam(foreach=False)
    and the regularisers differentiated by autograd on the GPU, and the same five with the yardstick (float64 state).  Both implementations stay
    within the yardstick's ACCUMULATED bounds (torch_ref_dense_adam.bounds(carried=...)) at every step, and the state_dict of one loads into the other."""
    P = 1031
    names = list(TRAINER_SHAPES)
    p0 = {n: trd.make_inputs((P,) + TRAINER_SHAPES[n], seed=100 + i, p_log_uniform_to=4.0 if n in REGS else None)[0] for i, n in enumerate(names)}
    grads = [{n: trd.make_inputs((P,) + TRAINER_SHAPES[n], seed=200 + 10 * k + i)[1] for i, n in enumerate(names)} for k in range(5)]

    def groups():
        params = {n: torch.nn.Parameter(dev(p0[n])) for n in names}
        return params, [{"params": [params[n]], "lr": TRAINER_LRS[n], "name": n} for n in names]

    ours_p, g1 = groups()
    ours = dgr().GaussianAdam(g1, lr=0.0, eps=1e-15)
    for n, reg in REGS.items():
        ours.set_regularizer(n, *reg)
    theirs_p, g2 = groups()
    theirs = torch.optim.Adam(g2, lr=0.0, eps=1e-15, foreach=False)
    ref = {n: (p0[n].astype(np.float64), np.zeros(p0[n].shape), np.zeros(p0[n].shape)) for n in names}
    carried = {n: (0.0, 0.0, 0.0) for n in names}
    worst = {"ours": 0.0, "torch": 0.0}
    for k in range(5):
        t = k + 1
        for n in names:
            ours_p[n].grad = dev(grads[k][n])
            theirs_p[n].grad = dev(grads[k][n])
        loss = REGS["opacity"][1] * torch.abs(torch.sigmoid(theirs_p["opacity"])).mean() + REGS["scaling"][1] * torch.abs(torch.exp(theirs_p["scaling"])).mean()
        loss.backward()   # (accumulates onto the gradients just set)
        ours.step()
        theirs.step()
        assert ours.last_launches == 1
        for n in names:
            rp, rm, rv = ref[n]
            new = trd.step(rp, grads[k][n], rm, rv, TRAINER_LRS[n], 1e-15, t, reg=REGS.get(n))
            bm, bv, bp, _ = trd.bounds(rp, grads[k][n], rm, rv, TRAINER_LRS[n], 1e-15, t, reg=REGS.get(n), carried=carried[n])
            for who, opt, params in (("ours", ours, ours_p), ("torch", theirs, theirs_p)):
                st = opt.state[params[n]]
                assert float(st["step"]) == t
                for name, x, r, bound in (("p", params[n], new[0], bp), ("m", st["exp_avg"], new[1], bm), ("v", st["exp_avg_sq"], new[2], bv)):
                    err = np.abs(host(x).astype(np.float64) - r)
                    worst[who] = max(worst[who], worst_ratio(err, bound))
                    assert np.all(err <= bound), f"{who} {n} step {t}: {name} worst error / accumulated bound {worst_ratio(err, bound):.3g}"
            ref[n], carried[n] = new, (bp, bm, bv)
    print(f"\nfive steps: worst error / accumulated bound  GaussianAdam {worst['ours']:.2f}  torch.optim.Adam {worst['torch']:.2f}")
    # the state of one loads into the other, and both go on from it
    sd_ours, sd_theirs = copy.deepcopy(ours.state_dict()), copy.deepcopy(theirs.state_dict())
    assert set(sd_ours["state"][0]) == set(sd_theirs["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    fresh_p, g3 = groups()
    fresh = dgr().GaussianAdam(g3, lr=0.0, eps=1e-3)
    fresh.load_state_dict(sd_theirs)
    assert all(g.get("reg") is None and g["eps"] == 1e-15 for g in fresh.param_groups)
    back_p, g4 = groups()
    back = torch.optim.Adam(g4, lr=0.0, eps=1e-3, foreach=False)
    back.load_state_dict(sd_ours)
    assert group_of(back, "opacity")["reg"] == ("sigmoid", 0.01)
    for n in names:
        st = fresh.state[fresh_p[n]]
        assert float(st["step"]) == 5 and st["step"].device.type == "cpu" and same_bits(st["exp_avg"], theirs.state[theirs_p[n]]["exp_avg"])
        assert same_bits(back.state[back_p[n]]["exp_avg_sq"], ours.state[ours_p[n]]["exp_avg_sq"])
        fresh_p[n].grad = dev(grads[0][n])
        back_p[n].grad = dev(grads[0][n])
    fresh.step()
    back.step()
    for n in names:   # the sixth step of a torch state under GaussianAdam, against the yardstick from that state
        st = theirs.state[theirs_p[n]]
        before = (p0[n], grads[0][n], host(st["exp_avg"]), host(st["exp_avg_sq"]))
        st = fresh.state[fresh_p[n]]
        check(f"loaded {n}", (host(fresh_p[n]), host(st["exp_avg"]), host(st["exp_avg_sq"])), before, TRAINER_LRS[n], 1e-15, 6)
        assert float(back.state[back_p[n]]["step"]) == 6


def test_densify_and_prune_and_mcmc_relocate_accept_the_class():
    P = 301
    rng = np.random.default_rng(7)
    names = list(TRAINER_SHAPES)
    opt, data = make_optimizer(P, names, seed=300, regs=REGS)
    opt.step()
    # 3DGS-MCMC's relocation: in place, the Parameters keep their identity
    opacity = group_of(opt, "opacity")["params"][0]
    with torch.no_grad():
        opacity[torch.from_numpy(rng.random(P) < 0.2).cuda()] = -8.0   # dead: sigmoid <= 0.005
    params = [g["params"][0] for g in opt.param_groups]
    plan = dgr().mcmc_relocate_(opt, torch.from_numpy(rng.random(P).astype(np.float32)).cuda())
    assert int((plan[0] >= 0).sum()) > 0 and all(g["params"][0] is p for g, p in zip(opt.param_groups, params))
    for i, n in enumerate(names):
        p = group_of(opt, n)["params"][0]
        g = trd.make_inputs(tuple(p.shape), seed=310 + i)[1]
        p.grad = dev(g)
        data[n] = (host(p), g, host(opt.state[p]["exp_avg"]), host(opt.state[p]["exp_avg_sq"]))
    opt.step()
    assert opt.last_launches == 1
    for n in names:
        check_group(opt, n, data, 2, reg=REGS.get(n), before=data[n])
    # the 3DGS trainer's densify_and_prune by a plan: new Parameters, the state moved onto them
    code = torch.from_numpy(rng.choice(np.array([0, 1, 1, 1, 3, 4], np.uint8), P)).cuda()   # prune, keep, keep + copy, two children
    new = dgr().densify_and_prune(opt, code)
    M = int((code == 1).sum() + 2 * (code == 3).sum() + 2 * (code == 4).sum())
    assert M != P and list(new) == names
    for i, n in enumerate(names):
        p = group_of(opt, n)["params"][0]
        assert p is new[n] and p.shape[0] == M and float(opt.state[p]["step"]) == 2
        g = trd.make_inputs(tuple(p.shape), seed=320 + i)[1]
        p.grad = dev(g)
        data[n] = (host(p), g, host(opt.state[p]["exp_avg"]), host(opt.state[p]["exp_avg_sq"]))
    opt.step()
    assert opt.last_launches == 1
    for n in names:
        check_group(opt, n, data, 3, reg=REGS.get(n), before=data[n])


def test_a_refused_step_changes_nothing():
    """Each refusal names the tensor; no bit of any tensor and no state["step"] changes, also for the good tensors in front of the bad one."""
    N = 67

    def fresh():
        opt, _ = make_optimizer(N, ["xyz", "opacity", "scaling"], seed=400, regs=REGS)
        opt.step()
        for g in opt.param_groups:
            g["params"][0].grad = torch.ones_like(g["params"][0])
        tensors = [t for g in opt.param_groups for t in (g["params"][0], g["params"][0].grad, opt.state[g["params"][0]]["exp_avg"], opt.state[g["params"][0]]["exp_avg_sq"])]
        return opt, tensors, [t.detach().clone() for t in tensors]

    def refused(opt, tensors, before, match):
        with pytest.raises(RuntimeError, match=match):
            opt.step()
        assert all(same_bits(t, b) for t, b in zip(tensors, before))
        assert all(float(opt.state[g["params"][0]]["step"]) == 1 for g in opt.param_groups if g["params"][0] in opt.state)

    opt, tensors, before = fresh()
    last = group_of(opt, "scaling")["params"][0]
    opt.state[last]["exp_avg"] = torch.zeros(3, N, device="cuda").t()
    refused(opt, tensors, before, r"group 'scaling' tensor 0: exp_avg must be contiguous")
    opt, tensors, before = fresh()
    last = group_of(opt, "scaling")["params"][0]
    last.grad = torch.ones(3, N, device="cuda").t()
    refused(opt, tensors, before, r"group 'scaling' tensor 0: grad must be contiguous")
    opt, tensors, before = fresh()
    last = group_of(opt, "scaling")["params"][0]
    opt.state[last]["exp_avg_sq"] = opt.state[last]["exp_avg_sq"].double()
    refused(opt, tensors, before, r"group 'scaling' tensor 0: exp_avg_sq: expected float32, got torch.float64")
    opt, tensors, before = fresh()
    last = group_of(opt, "scaling")["params"][0]
    opt.state[last]["exp_avg"] = opt.state[last]["exp_avg"].cpu()
    refused(opt, tensors, before, r"group 'scaling' tensor 0: exp_avg is on cpu: there is no CPU path")
    opt, tensors, before = fresh()
    last = group_of(opt, "scaling")["params"][0]
    last.grad = last.grad.to_sparse()
    refused(opt, tensors[:9] + tensors[10:], before[:9] + before[10:], r"group 'scaling' tensor 0: sparse gradients are not supported")
    opt, tensors, before = fresh()
    group_of(opt, "scaling")["params"].append(torch.nn.Parameter(torch.ones(N, 3, device="cuda").double()))
    group_of(opt, "scaling")["params"][1].grad = torch.ones(N, 3, device="cuda").double()
    refused(opt, tensors, before, r"group 'scaling' tensor 1: param: expected float32")
    # a new tensor that was to get its state in the refused step has none
    assert group_of(opt, "scaling")["params"][1] not in opt.state
    # and the binding refuses what it cannot update in place
    z = lambda *shape: torch.zeros(*shape, device="cuda")
    co = [_C().dense_adam_coefficients(1e-3, 0.9, 0.999, 1e-8, 1)]
    with pytest.raises(RuntimeError, match="must be contiguous"):
        _C().dense_adam([z(3, N).t()], [z(N, 3)], [z(N, 3)], [z(N, 3)], co, [0])
    with pytest.raises(RuntimeError, match="has shape"):
        _C().dense_adam([z(N, 3)], [z(N, 4)], [z(N, 3)], [z(N, 3)], co, [0])
    with pytest.raises(RuntimeError, match="unknown reg_kind 5"):
        _C().dense_adam([z(N, 3)], [z(N, 3)], [z(N, 3)], [z(N, 3)], co, [5])
    assert _C().dense_adam([z(0, 3)], [z(0, 3)], [z(0, 3)], [z(0, 3)], co, [0]) == 0
