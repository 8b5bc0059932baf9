"""GPU tests of the 3DGS-MCMC kernels (compute_relocation, mcmc_add_noise_, _C.compute_relocation, _C.mcmc_add_noise; include/stp_raster.h:
stp_mcmc_relocation, stp_mcmc_add_noise) against the float64 yardstick tests/torch_ref_mcmc.py.

Tolerances: 4 times the worst error of the CPU restatement of the kernels' evaluation order on exactly these inputs, as
tests/test_mcmc_cpu.py measures it (torch_ref_mcmc.RELOCATION_BOUND = 2.4e-7 from 5.9e-8 measured, NOISE_BOUND = 3.36e-5 from 8.4e-6).

Relocation: relative error of opacity_new and of every scale_new component.  Noise: per Gaussian  |dxyz - ref|_2 <= T max(s)^2 |noise g
noise_scale|_2  where the float64 gate g exceeds 1e-20, dxyz read from a run on xyz = 0 (so that the rounding of the addition to a position
is not in it); a run on real positions must then give fl(xyz + dxyz) bit for bit.  Where g <= 1e-20 the rows are held to the same bound plus
1e-25 absolute.  (Not to |dxyz|_2 <= 1e-25 alone: float32 gates underflow only below 1e-38, and between 1e-38 and 1e-20 -- opacities of
0.47 .. 0.88 -- the yardstick itself moves a Gaussian by up to 1e-19 at noise_scale = 0.8, so that line cannot hold for a correct kernel; the
bound used here asks more of those rows, not less.)

The relocation kernel owns one Gaussian per lane in workgroups of 256; the noise kernel four Gaussians per lane where every pointer is 16-byte
aligned (P % 4 rows in a tail) and one otherwise: the sizes are the wave and workgroup edges, sizes that are no multiple of four, more than
one workgroup on either path, and views that start 4 or 12 bytes into their storage."""
import ctypes

import numpy as np
import pytest
import torch

import torch_ref_mcmc as trm

pytestmark = pytest.mark.gpu


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


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- relocation --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_relocation_against_the_yardstick(n):
    o, s, N = trm.relocation_inputs(n)
    if n == 4097:
        assert set(range(1, 51)) | {0, -3, 51, 1000} <= set(N.tolist())
    first = None
    for n_dtype in (np.int64, np.int32):
        for column in (False, True):
            od, sd, Nd = dev(o[:, None] if column else o), dev(s), dev(N.astype(n_dtype)[:, None] if column else N.astype(n_dtype))
            keep = [t.clone() for t in (od, sd, Nd)]
            o_new, s_new = dgr().compute_relocation(od, sd, Nd)
            assert o_new.shape == od.shape and s_new.shape == (n, 3) and o_new.dtype == s_new.dtype == torch.float32 and o_new.is_cuda
            assert same_bits(od, keep[0]) and same_bits(sd, keep[1]) and torch.equal(Nd, keep[2]), "an input was modified"
            eo, es = trm.relocation_errors(o_new.cpu().numpy(), s_new.cpu().numpy(), o, s, N)
            print(f"\nn={n} {np.dtype(n_dtype).name} column={column}: worst relative error opacity_new {eo:.3g} scale_new {es:.3g} (bound {trm.RELOCATION_BOUND:.3g})")
            assert eo <= trm.RELOCATION_BOUND and es <= trm.RELOCATION_BOUND
            if first is None:
                first = (o_new.reshape(-1), s_new)
            else:   # equal inputs give equal bits, whatever N's type and the opacity's shape
                assert same_bits(o_new.reshape(-1), first[0]) and same_bits(s_new, first[1])
    # N outside [1, 50] behaves as clamped
    o_c, s_c = dgr().compute_relocation(dev(o), dev(s), dev(np.clip(N, 1, 50)))
    assert same_bits(o_c, first[0]) and same_bits(s_c, first[1])
    if n >= 65:
        rows = torch.from_numpy(np.flatnonzero(N == 1)).cuda()   # N = 1: the Gaussian itself
        assert same_bits(first[0][rows], dev(o)[rows]) and same_bits(first[1][rows], dev(s)[rows])


def test_relocation_of_views():
    o, s, N = trm.relocation_inputs(65)
    want = dgr().compute_relocation(dev(o), dev(s), dev(N))
    got = dgr().compute_relocation(dev(o, 1), dev(s, 1), dev(N))   # views that start one float into their storage
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    # non-contiguous inputs are made contiguous
    o2 = torch.stack([dev(o), torch.zeros(65, device="cuda")], dim=1)[:, 0]
    s2 = dev(np.ascontiguousarray(s.T)).t()
    N2 = torch.stack([dev(N), dev(N)], dim=1)[:, 1]
    assert not o2.is_contiguous() and not s2.is_contiguous() and not N2.is_contiguous()
    got = dgr().compute_relocation(o2, s2, N2)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    # a leaf that requires grad is read like any tensor; nothing is recorded
    got = dgr().compute_relocation(dev(o).requires_grad_(True), dev(s).requires_grad_(True), dev(N))
    assert same_bits(got[0], want[0]) and not got[0].requires_grad and not got[1].requires_grad
    empty = dgr().compute_relocation(dev(o[:0]), dev(s[:0]), dev(N[:0]))
    assert empty[0].shape == (0,) and empty[1].shape == (0, 3)


def test_relocation_under_upstreams_name_and_argument_order():
    o, s, N = trm.relocation_inputs(4097)
    want = dgr().compute_relocation(dev(o), dev(s), dev(N))
    binoms = torch.full((51, 51), float("nan"), device="cuda")   # (the contents are not read)
    Nd = dev(N)
    got = _C().compute_relocation(dev(o), dev(s), Nd, binoms, 51)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and torch.equal(Nd, dev(N))
    # n_max is the clamp's upper bound plus one
    got = _C().compute_relocation(dev(o), dev(s), dev(N), torch.zeros(11, 11, device="cuda"), 11)
    want10 = dgr().compute_relocation(dev(o), dev(s), dev(np.clip(N, 1, 10)))
    assert same_bits(got[0], want10[0]) and same_bits(got[1], want10[1])
    with pytest.raises(RuntimeError, match="N: expected all tensors on"):
        _C().compute_relocation(dev(o), dev(s), dev(N).cpu(), binoms, 51)


def test_relocation_through_the_c_abi():
    o, s, N = trm.relocation_inputs(65)
    want = dgr().compute_relocation(dev(o), dev(s), dev(N))
    L = _C()._load()
    for kind, Nd in ((1, dev(N)), (0, dev(N.astype(np.int32)))):
        od, sd = dev(o), dev(s)
        o_new, s_new = torch.empty_like(od), torch.empty_like(sd)
        torch.cuda.synchronize()
        assert L.stp_mcmc_relocation(65, od.data_ptr(), sd.data_ptr(), Nd.data_ptr(), kind, 51, o_new.data_ptr(), s_new.data_ptr(), None) == 1   # one launch
        torch.cuda.synchronize()
        assert same_bits(o_new, want[0]) and same_bits(s_new, want[1])


# ---- noise -------------------------------------------------------------------------------------------------------------------------------

def noise_run(inp, raw, xyz, **kw):
    s, q, o, w = (dev(a) for a in trm.noise_args(inp, raw))
    out = dgr().mcmc_add_noise_(xyz, s, q, o, w, trm.NOISE_SCALE, raw=raw, **kw)
    assert out is xyz
    return out


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("P", trm.NOISE_SIZES)
def test_noise_against_the_yardstick(P, raw):
    inp = trm.noise_inputs(P)
    s, q, o, w = (dev(a) for a in trm.noise_args(inp, raw))
    keep = [t.clone() for t in (s, q, o, w)]
    d = torch.zeros(P, 3, device="cuda")
    assert dgr().mcmc_add_noise_(d, s, q, o, w, trm.NOISE_SCALE, raw=raw) is d
    for t, c in zip((s, q, o, w), keep):
        assert same_bits(t, c), "an input was modified"
    ratio, excess_below_floor = trm.noise_error_ratio(d.cpu().numpy(), inp, raw)   # (rows without noise: exactly zero, checked there)
    print(f"\nP={P} raw={raw}: worst |dxyz - ref| / (max(s)^2 |v|) {ratio:.3g} (bound {trm.NOISE_BOUND:.3g})")
    assert ratio <= trm.NOISE_BOUND
    assert excess_below_floor(trm.NOISE_BOUND) <= 0
    # on real positions: fl(xyz + dxyz), bit for bit; rows whose noise is zero keep their value
    xyz = dev(inp["xyz"])
    before = xyz.clone()
    noise_run(inp, raw, xyz)
    assert same_bits(xyz, before + d)
    still = torch.from_numpy(~inp["noise"].any(axis=1)).cuda()
    assert same_bits(xyz[still], before[still])
    if P >= 7:
        assert bool(still.any()) and not torch.equal(xyz, before)
    # the unaligned path (xyz as a view offset by one row; the noise one float into its storage) gives the same bits
    for offsets in ((3, 0), (0, 1), (3, 1)):
        base = torch.empty(P + 1, 3, device="cuda")
        view = base[1:] if offsets[0] else torch.empty(P, 3, device="cuda")
        view.copy_(before)
        assert view.data_ptr() % 16 == (12 if offsets[0] else 0) and view.is_contiguous()
        dgr().mcmc_add_noise_(view, s, q, o, dev(trm.noise_args(inp, raw)[3], offsets[1]), trm.NOISE_SCALE, raw=raw)
        assert same_bits(view, xyz)


def test_noise_shapes_leaves_and_repeats():
    P = 1000
    inp = trm.noise_inputs(P)
    for raw in (False, True):
        s, q, o, w = (dev(a) for a in trm.noise_args(inp, raw))
        want = noise_run(inp, raw, dev(inp["xyz"]))
        again = noise_run(inp, raw, dev(inp["xyz"]))
        assert same_bits(want, again)                                     # equal inputs give equal bits
        got = dgr().mcmc_add_noise_(dev(inp["xyz"]), s, q, o[:, None], w, trm.NOISE_SCALE, raw=raw)   # opacities as (P, 1)
        assert same_bits(got, want)
        # non-contiguous inputs are made contiguous
        s2, q2 = dev(np.ascontiguousarray(trm.noise_args(inp, raw)[0].T)).t(), torch.cat([q, q], dim=1)[:, 4:]
        assert not s2.is_contiguous() and not q2.is_contiguous()
        assert same_bits(dgr().mcmc_add_noise_(dev(inp["xyz"]), s2, q2, o, w, trm.NOISE_SCALE, raw=raw), want)
        # a leaf that requires grad: accepted, updated in place, nothing recorded
        leaf = torch.nn.Parameter(dev(inp["xyz"]))
        sp, op = torch.nn.Parameter(s), torch.nn.Parameter(o)
        out = dgr().mcmc_add_noise_(leaf, sp, q, op, w, trm.NOISE_SCALE, raw=raw)
        assert out is leaf and leaf.grad_fn is None and leaf.is_leaf and leaf.requires_grad and leaf.grad is None and same_bits(leaf, want)
        # k and x0: the defaults are upstream's op_sigmoid
        assert same_bits(dgr().mcmc_add_noise_(dev(inp["xyz"]), s, q, o, w, trm.NOISE_SCALE, raw=raw, k=100.0, x0=0.995), want)
        assert not same_bits(dgr().mcmc_add_noise_(dev(inp["xyz"]), s, q, o, w, trm.NOISE_SCALE, raw=raw, k=50.0), want)
    with pytest.raises(RuntimeError, match="xyz must be contiguous"):
        dgr().mcmc_add_noise_(dev(np.zeros((3, P), np.float32)).t(), s, q, o, w, trm.NOISE_SCALE)
    with pytest.raises(RuntimeError, match="noise: expected all tensors on"):
        dgr().mcmc_add_noise_(dev(inp["xyz"]), s, q, o, w.cpu(), trm.NOISE_SCALE)
    empty = torch.zeros(0, 3, device="cuda")
    assert dgr().mcmc_add_noise_(empty, empty, torch.zeros(0, 4, device="cuda"), torch.zeros(0, device="cuda"), empty, 1.0) is empty
    assert _C().mcmc_add_noise(empty, empty, torch.zeros(0, 4, device="cuda"), torch.zeros(0, device="cuda"), empty, 1.0, 100.0, 0.995, False) == 0


def test_noise_special_values():
    """A zero quaternion gives NaN in its own row only (both paths); a gate whose exp overflows is 0: the row keeps its bits."""
    P = 64
    inp = trm.noise_inputs(P)
    inp["rotations"][9] = 0.0
    inp["opacities"][10] = 1.0
    inp["noise"][10] = (1.0, -2.0, 3.0)
    for offset_rows in (0, 1):
        base = torch.empty(P + 1, 3, device="cuda")
        xyz = base[offset_rows:offset_rows + P]
        xyz.copy_(dev(inp["xyz"]))
        before = xyz.clone()
        noise_run(inp, False, xyz)
        nan_rows = torch.isnan(xyz).any(dim=1)
        assert nan_rows.tolist() == [i == 9 for i in range(P)] and bool(torch.isnan(xyz[9]).all())
        assert same_bits(xyz[10], before[10])


def test_noise_through_the_c_abi():
    P = 65
    inp = trm.noise_inputs(P)
    L = _C()._load()
    for raw in (0, 1):
        want = noise_run(inp, bool(raw), dev(inp["xyz"]))
        xyz = dev(inp["xyz"])
        s, q, o, w = (dev(a) for a in trm.noise_args(inp, bool(raw)))
        torch.cuda.synchronize()
        assert L.stp_mcmc_add_noise(P, xyz.data_ptr(), s.data_ptr(), q.data_ptr(), o.data_ptr(), w.data_ptr(), trm.NOISE_SCALE, 100.0, 0.995, raw, None) == 1
        torch.cuda.synchronize()
        assert same_bits(xyz, want)
