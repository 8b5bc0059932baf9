"""GPU tests of the spatial order and the gather (spatial_order, gather_tensors, reorder_gaussians_; include/stp_raster.h: stp_spatial_order,
stp_gather_rows).

Everything the calls themselves produce is integers or moved bits, so every comparison of them is exact: spatial_order against the numpy
restatement of the header's definition (tests/torch_ref_spatial_order.py) with np.array_equal, the gather against torch.index_select on the
int32 view of the same storage.  Only the render-invariance test at the end compares floating-point sums -- two summation orders of the same
sums -- and it uses the bounds tests/test_gpu_parity.py holds the product to against the oracle on that scene: PSNR >= 100 dB on the image,
1e-4 of the largest entry on every gradient tensor.

A gather's work unit is 1024 items (256 threads x 4), an item 16 bytes on the wide path and one float otherwise; eight tensors go in one
launch.  The spatial order's kernels run one lane per point in workgroups of 256; rocPRIM changes its plan with the size."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import torch_ref_knn as trk
import torch_ref_spatial_order as tso
from helpers import FULL_STP, GpuRun, _rel, _scene_a, api_render, psnr, settings_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dgr():
    import diff_gaussian_rasterization as d
    return d


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


def check_order(points, want_order, want_codes, got):
    order, codes = got
    assert order.dtype == torch.int32 and codes.dtype == torch.int32 and order.shape == codes.shape == (points.shape[0],)
    assert np.array_equal(order.cpu().numpy(), want_order)
    assert np.array_equal(codes.cpu().numpy().view(np.uint32), want_codes)


# ---- 1. spatial_order against the yardstick ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,P", tso.CASES)
def test_spatial_order_bit_equal(name, P):
    p, want_order, want_codes = tso.case(name, P)
    x = torch.tensor(p, device="cuda")
    with no_sync():   # (and with it: on a side stream)
        got = dgr().spatial_order(x, return_codes=True)
        alone = dgr().spatial_order(x)
        again = dgr().spatial_order(x, return_codes=True)
    check_order(p, want_order, want_codes, got)
    assert alone.dtype == torch.int32 and torch.equal(alone, got[0])
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])   # a second call gives equal bits
    assert torch.equal(x, torch.tensor(p, device="cuda"))


def test_spatial_order_signed_zeros_infinities_views_and_empty():
    order, codes = tso.order_and_codes(tso.SIGNS)
    assert order.tolist() == [3, 1, 0, 4, 2]
    check_order(tso.SIGNS, order, codes, dgr().spatial_order(torch.from_numpy(tso.SIGNS).cuda(), True))
    # a non-contiguous view: the columns of a (3, P) tensor, and every second row of a (2 P, 3) one
    p, want_order, want_codes = tso.case("uniform", 257)
    t = torch.tensor(np.ascontiguousarray(p.T), device="cuda").t()
    assert not t.is_contiguous()
    check_order(p, want_order, want_codes, dgr().spatial_order(t, True))
    wide = torch.zeros(2 * 257, 3, device="cuda")
    wide[::2] = torch.tensor(p, device="cuda")
    check_order(p, want_order, want_codes, dgr().spatial_order(wide[::2], True))
    # a leaf that requires grad is detached
    leaf = torch.nn.Parameter(torch.tensor(p, device="cuda"))
    got = dgr().spatial_order(leaf)
    assert not got.requires_grad and np.array_equal(got.cpu().numpy(), want_order)
    # P = 0
    order, codes = dgr().spatial_order(torch.zeros(0, 3, device="cuda"), True)
    assert order.dtype == codes.dtype == torch.int32 and order.shape == codes.shape == (0,)
    assert dgr().spatial_order(torch.zeros(0, 3, device="cuda")).shape == (0,)


# ---- 2. idempotence on the device ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,P", [("clustered", trk.LARGE), ("dups", trk.SMALL)])
def test_order_of_an_ordered_cloud_is_the_identity(name, P):
    x = torch.tensor(tso.case(name, P)[0], device="cuda")
    order, codes = dgr().spatial_order(x, True)
    (sorted_x,), _, _ = dgr().gather_tensors(order, [x])
    assert torch.equal(sorted_x, x[order.long()])
    again, codes2 = dgr().spatial_order(sorted_x, True)
    assert torch.equal(again, torch.arange(x.shape[0], dtype=torch.int32, device="cuda")) and torch.equal(codes2, codes)


# ---- 3. distCUDA2 is untouched -------------------------------------------------------------------------------------------------------------

def test_knn_still_bit_equal_to_the_brute_force():
    p, ref = trk.case("clustered", trk.SMALL)
    got = dgr().knn_mean_dist2(torch.tensor(p, device="cuda")).cpu().numpy()
    assert np.array_equal(got.view(np.int32), ref.view(np.int32))


# ---- 4. gather_tensors ---------------------------------------------------------------------------------------------------------------------

def raw_rows(P, shape, seed, offset_floats=0):
    """(P, *shape) float32 on the device holding random BITS (NaN payloads, infinities, denormals and -0 among them); offset_floats = k: a
    view that starts 4 k bytes into its storage"""
    n = P * int(np.prod(shape))
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(-2 ** 31, 2 ** 31 - 1, (n + offset_floats,), generator=g, dtype=torch.int64).to(torch.int32).cuda().view(torch.float32)
    t = base[offset_floats:].view(P, *shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == (4 * offset_floats) % 16
    return t


def same_rows(got, src, index):
    """got == index_select(src, index), as int32 bits"""
    want = torch.index_select(src.contiguous().view(torch.int32), 0, index.long())
    return got.dtype == src.dtype and got.shape == want.shape and got.is_contiguous() and torch.equal(got.view(torch.int32), want)


def check_gather(index, tensors, ms=None, vs=None):
    before = [t.clone() for t in tensors] + [m.clone() for m in (ms or []) + (vs or []) if m is not None]
    with no_sync():
        new_t, new_m, new_v = dgr().gather_tensors(index, tensors, ms, vs)
    assert len(new_t) == len(new_m) == len(new_v) == len(tensors)
    for k, t in enumerate(tensors):
        assert same_rows(new_t[k], t, index), k
        if ms is not None and ms[k] is not None:
            assert same_rows(new_m[k], ms[k], index) and same_rows(new_v[k], vs[k], index), k
        else:
            assert new_m[k] is None and new_v[k] is None
    after = list(tensors) + [m for m in (ms or []) + (vs or []) if m is not None]
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, after))   # inputs unchanged
    return new_t


# rows of 1, 3, 9 and 45 floats: the one-float path; 4 and 48: 16 bytes per lane; 4 and 48 as views one float into their storage: aligned rows
# that must take the one-float path.  Eight tensors: one launch.
WIDTHS = (((1,), 0), ((3,), 0), ((4,), 0), ((3, 3), 0), ((15, 3), 0), ((16, 3), 0), ((4,), 1), ((16, 3), 1))


@pytest.mark.parametrize("P", [1, 255, 256, 257, 1023, 1024, 1025])   # a work unit is 1024 items: rows of 1 float and rows of 4 cross it at 1024
@pytest.mark.parametrize("moments", [False, True])
def test_gather_permutation_of_every_row_width(P, moments):
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(P)).to(torch.int32).cuda()
    tensors = [raw_rows(P, shape, 10 * k + 1, off) for k, (shape, off) in enumerate(WIDTHS)]
    ms = [raw_rows(P, shape, 10 * k + 2, off) for k, (shape, off) in enumerate(WIDTHS)] if moments else None
    vs = [raw_rows(P, shape, 10 * k + 3, off) for k, (shape, off) in enumerate(WIDTHS)] if moments else None
    check_gather(perm, tensors, ms, vs)


@pytest.mark.parametrize("n", [9, 17])
def test_gather_more_tensors_than_one_table_holds(n):
    P = 300
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(n)).to(torch.int32).cuda()
    shapes = [WIDTHS[k % len(WIDTHS)] for k in range(n)]
    tensors = [raw_rows(P, shape, 100 + k, off) for k, (shape, off) in enumerate(shapes)]
    ms = [raw_rows(P, shape, 200 + k, off) if k % 3 else None for k, (shape, off) in enumerate(shapes)]   # every third tensor has no moments
    vs = [raw_rows(P, shape, 300 + k, off) if k % 3 else None for k, (shape, off) in enumerate(shapes)]
    check_gather(perm, tensors, ms, vs)


def test_gather_subsets_repeats_int32_special_values_and_empty():
    P = 1025
    tensors = [raw_rows(P, shape, 400 + k, off) for k, (shape, off) in enumerate(WIDTHS)]
    g = torch.Generator().manual_seed(5)
    subset = torch.randperm(P, generator=g)[:300].to(torch.int32).cuda()                    # M < P
    repeats = torch.randint(0, P, (2 * P + 3,), generator=g).to(torch.int32).cuda()         # M > P
    check_gather(subset, tensors)
    check_gather(repeats, tensors, [t.clone() for t in tensors], [t.flip(0).contiguous() for t in tensors])
    # an int64 index is converted; an int32 tensor moves like a float one and keeps its dtype
    ints = torch.arange(P * 3, dtype=torch.int32, device="cuda").view(P, 3) - 7
    (got_i, got_f), _, _ = dgr().gather_tensors(subset.long(), [ints, tensors[1]])
    assert got_i.dtype == torch.int32 and torch.equal(got_i, ints[subset.long()]) and same_rows(got_f, tensors[1], subset)
    # NaN payloads, -0, the infinities and a denormal, by name, on both paths
    special = torch.tensor([0x7FC00001, 0xFFC12345 - 2 ** 32, 0x7F800001, 0x80000000 - 2 ** 32, 0x7F800000, 0xFF800000 - 2 ** 32, 1, 0], dtype=torch.int32).cuda()
    for shape in ((2,), (8,)):
        t = special.repeat(P)[:P * shape[0]].view(torch.float32).view(P, *shape).contiguous()
        (got,) = check_gather(repeats, [t])
        assert torch.isnan(got).any() and torch.isnan(t).any()
    # M = 0
    new_t, new_m, new_v = dgr().gather_tensors(subset[:0], tensors[:2], tensors[:2], tensors[:2])
    assert [t.shape for t in new_t] == [(0,) + t.shape[1:] for t in tensors[:2]] and all(m.shape[0] == 0 for m in new_m + new_v)
    assert dgr().gather_tensors(subset, []) == ([], [], [])


# ---- 5. reorder_gaussians_ -----------------------------------------------------------------------------------------------------------------

GROUPS = (("xyz", (3,)), ("f_dc", (1, 3)), ("f_rest", (15, 3)), ("opacity", (1,)), ("scaling", (3,)), ("rotation", (4,)), ("unused", (2,)))
NAMES = [n for n, _ in GROUPS]
P_MODEL = trk.SMALL


def make_optimizer(kind, steps=2):
    """upstream's six groups and one that never gets a gradient, after `steps` steps -> (optimizer, {name: Parameter})"""
    r = np.random.default_rng(17)
    values = {n: r.normal(0.0, 1.0, (P_MODEL,) + shape).astype(np.float32) for n, shape in GROUPS}
    values["xyz"] = trk.clustered(P_MODEL)
    params = {n: torch.nn.Parameter(torch.from_numpy(values[n]).cuda()) for n in NAMES}
    groups = [{"params": [params[n]], "lr": 1e-3 * (k + 1), "name": n} for k, n in enumerate(NAMES)]
    d = dgr()
    opt = {"adam": torch.optim.Adam, "sparse": d.SparseGaussianAdam, "gaussian": d.GaussianAdam}[kind](groups, lr=0.0, eps=1e-15)
    for s in range(steps):
        for n in NAMES[:-1]:
            params[n].grad = torch.from_numpy(r.normal(0.0, 1.0, values[n].shape).astype(np.float32)).cuda()
        step(opt, kind)
    opt.zero_grad(set_to_none=True)
    return opt, params


def step(opt, kind):
    if kind == "sparse":
        vis = (torch.arange(P_MODEL, device="cuda") % 3 != 0)
        opt.step(vis, P_MODEL)
    else:
        opt.step()


def snapshot(opt):
    """{name: (param, exp_avg or None, exp_avg_sq or None, step or None)} as clones"""
    out = {}
    for g in opt.param_groups:
        p = g["params"][0]
        st = opt.state.get(p, {})
        c = lambda t: None if t is None else t.detach().clone()
        out[g["name"]] = (c(p), c(st.get("exp_avg")), c(st.get("exp_avg_sq")), None if "step" not in st else float(st["step"]))
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("kind", ["adam", "sparse", "gaussian"])
def test_reorder_gaussians_on_a_seven_group_optimizer(kind):
    opt, params = make_optimizer(kind)
    before = snapshot(opt)
    options = [{k: v for k, v in g.items() if k != "params"} for g in opt.param_groups]
    want = torch.from_numpy(tso.order_and_codes(before["xyz"][0].cpu().numpy())[0]).cuda()
    accum = torch.rand(P_MODEL, 1, device="cuda")
    radii = torch.arange(P_MODEL, dtype=torch.int32, device="cuda") * 3 - 50
    with no_sync():
        new, order, extra = dgr().reorder_gaussians_(opt, extra=[accum, radii])
    assert order.dtype == torch.int32 and torch.equal(order, want)                               # the returned order is the yardstick's
    sel = lambda t: torch.index_select(t, 0, want.long())
    assert list(new) == NAMES and len(opt.state) == len(NAMES) - 1 and all(old not in opt.state for old in params.values())
    for g, n, old_options in zip(opt.param_groups, NAMES, options):
        p = g["params"][0]
        assert p is new[n] and p is not params[n] and isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf
        assert {k: v for k, v in g.items() if k != "params"} == old_options and g["name"] == n   # "lr", "name" and every other option
        old_p, old_m, old_v, old_step = before[n]
        assert same_bits(p.detach(), sel(old_p))
        if n == "unused":
            assert p not in opt.state                                                            # an empty state stays empty
        else:
            st = opt.state[p]
            assert float(st["step"]) == old_step == 2.0 and same_bits(st["exp_avg"], sel(old_m)) and same_bits(st["exp_avg_sq"], sel(old_v))
    assert len(extra) == 2 and same_bits(extra[0], sel(accum)) and extra[1].dtype == torch.int32 and torch.equal(extra[1], sel(radii))
    # a following step runs on the new tensors
    for n in NAMES[:-1]:
        new[n].grad = torch.ones_like(new[n])
    step(opt, kind)
    assert all(float(opt.state[new[n]]["step"]) == 3.0 and torch.isfinite(new[n]).all() for n in NAMES[:-1])


def test_gaussian_adam_step_commutes_with_the_reorder():
    """The step is elementwise: one more step() on given gradients gives the same bits on the reordered model as on the original model permuted
    afterwards."""
    a, pa = make_optimizer("gaussian")
    b, pb = make_optimizer("gaussian")
    grads = {n: torch.from_numpy(np.random.default_rng(23).normal(0.0, 1.0, tuple(pa[n].shape)).astype(np.float32)).cuda() for n in NAMES[:-1]}
    new, order, _ = dgr().reorder_gaussians_(a)
    for n in NAMES[:-1]:
        new[n].grad = torch.index_select(grads[n], 0, order.long())
        pb[n].grad = grads[n].clone()
    a.step()
    b.step()
    sa, sb = snapshot(a), snapshot(b)
    for n in NAMES:
        for x, y in zip(sa[n][:3], sb[n][:3]):
            assert (x is None and y is None) or same_bits(x, torch.index_select(y, 0, order.long())), n
        assert sa[n][3] == sb[n][3]


def test_reorder_by_an_explicit_order_and_back():
    opt, params = make_optimizer("adam")
    before = snapshot(opt)
    perm = torch.randperm(P_MODEL, generator=torch.Generator().manual_seed(3)).to(torch.int32).cuda()
    inverse = torch.empty_like(perm)
    inverse[perm.long()] = torch.arange(P_MODEL, dtype=torch.int32, device="cuda")
    side = torch.rand(P_MODEL, device="cuda")
    new, order, (moved,) = dgr().reorder_gaussians_(opt, perm, extra=[side])
    assert order is perm and same_bits(new["xyz"].detach(), before["xyz"][0][perm.long()]) and same_bits(moved, side[perm.long()])
    assert not same_bits(new["xyz"].detach(), before["xyz"][0])
    _, _, (back,) = dgr().reorder_gaussians_(opt, inverse, extra=[moved])
    after = snapshot(opt)
    assert same_bits(back, side)
    for n in NAMES:
        for x, y in zip(after[n][:3], before[n][:3]):
            assert (x is None and y is None) or same_bits(x, y), n
        assert after[n][3] == before[n][3]


# ---- 6. render invariance ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sd", [settings_dict(**FULL_STP), settings_dict()], ids=["full_stp", "global"])
def test_a_reordered_model_renders_the_same_frame(sd):
    """The end-to-end check that rows stayed together: the model gathered by spatial_order renders the frame of the original model.  The two
    renders are two summation orders of the same sums, held to the bounds the product is held to against the oracle on this scene."""
    sc = _scene_a()
    names = ("means3D", "opacities", "shs", "scales", "rotations")
    src = [torch.from_numpy(np.ascontiguousarray(getattr(sc, n), np.float32)).cuda() for n in names]
    order = dgr().spatial_order(src[0])
    moved, _, _ = dgr().gather_tensors(order, src)
    o = order.cpu().numpy()
    assert sorted(o.tolist()) == list(range(sc.means3D.shape[0])) and not np.array_equal(o, np.arange(o.size))   # (the scene's rows are in random order)
    sc2 = copy.copy(sc)
    for n, t in zip(names, moved):
        setattr(sc2, n, t.cpu().numpy())
        assert np.array_equal(getattr(sc2, n), getattr(sc, n)[o])
    a, b = api_render(sc, sd), api_render(sc2, sd)
    assert np.array_equal(b["radii"].cpu().numpy(), a["radii"].cpu().numpy()[o]) and int((a["radii"] > 0).sum()) > 0
    assert GpuRun(sc2, sd, backward=False, warm=False).num_rendered == GpuRun(sc, sd, backward=False, warm=False).num_rendered > 0
    ia, ib = a["color"].cpu().numpy(), b["color"].cpu().numpy()
    print(f"\nimage bit-equal: {np.array_equal(ia, ib)}; PSNR {psnr(ib, ia):.1f} dB")
    assert psnr(ib, ia) >= 100.0
    for n in ("means3D", "means2D", "shs", "opacities", "scales", "rotations"):
        ga, gb = a[n].cpu().numpy(), b[n].cpu().numpy()
        back = np.empty_like(gb)
        back[o] = gb                                                   # gathered back: row order[s] of the original is row s of the reordered model
        print(f"{n}: relative difference {_rel(back, ga):.3g}")
        assert float(np.abs(ga).max()) > 0 and _rel(back, ga) < 1e-4, n


# ---- 7. the example ------------------------------------------------------------------------------------------------------------------------

def test_trainer_example_with_reorder():
    """examples/train_render.py --strategy adc --reorder 10 in a child process: the model is re-sorted at iterations 10 and 20, each time just
    before the densification that then appends rows again, and the fit ends with a finite loss."""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_render.py"), "--strategy", "adc", "--reorder", "10", "--iters", "25", "--points", "2000",
           "--size", "96", "64"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=170)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if "reorder:" in ln]
    assert len(lines) == 2 and lines[0].startswith("iter  10  reorder: 2000 rows into Morton order") and lines[1].startswith("iter  20  reorder: "), p.stdout
    last = [ln for ln in p.stdout.splitlines() if ln.startswith("L1 ")][-1]
    first_loss, last_loss = (float(x) for x in last.split(";")[0].replace("L1 ", "").split(" -> "))
    assert np.isfinite(first_loss) and np.isfinite(last_loss), last
