"""Float64 yardstick of the 3DGS-MCMC kernels (include/stp_raster.h: stp_mcmc_relocation, stp_mcmc_add_noise), the restatements of the
kernels' own evaluation order that fix the tolerances on the CPU, and the inputs the CPU measurement and the GPU tests share.

relocation(): upstream's formulas literally, in float64 from the float32 inputs, WITH the double loop:
    o_new = 1 - (1 - o)^(1/N)     denom = sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k o_new^(k+1) / sqrt(k+1)     s_new = (o / denom) s
noise_step(): upstream's composition literally, in float64 from the float32 inputs, noise_scale, k and x0 rounded to float32 once:
    L = R(q / |q|) diag(s),  Sigma = L L^T,  g = 1 / (1 + exp(-k ((1 - o) - x0))),  dxyz = Sigma (noise * g * noise_scale)
relocation_kernel_order() / noise_kernel_order(): what csrc/stp_mcmc.hip computes, operation by operation, in numpy -- float64 internals
and float32 results for the relocation, float32 throughout for the noise (numpy has no fused multiply-add: the products round once more
than the kernel's, which the factor 4 between the measured error and the GPU bound covers)."""
from math import comb

import numpy as np

N_MAX = 51   # upstream's N_max: N is clamped to [1, N_MAX - 1]

# The worst errors of the two restatements against the yardstick on the inputs below, as tests/test_mcmc_cpu.py measures them (rounded up to
# two digits), and the GPU tests' bounds: 4 times that.
RELOCATION_MEASURED, RELOCATION_BOUND = 6.0e-8, 2.4e-7   # relative, opacity_new and every scale_new component
NOISE_MEASURED, NOISE_BOUND = 8.4e-6, 3.36e-5            # |dxyz - ref|_2 / (max(s)^2 |noise * gate * noise_scale|_2)


def f32(x):
    """A Python float rounded to float32 once, as a float64."""
    return float(np.float32(x))


def clamp_N(N, n_max=N_MAX):
    return np.clip(np.asarray(N).astype(np.int64).reshape(-1), 1, n_max - 1)


def denominator_double_loop(o_new, N):
    """sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k o_new^(k+1) / sqrt(k+1), float64; o_new (n,), N (n,) already clamped."""
    o_new = np.asarray(o_new, np.float64)
    denom = np.zeros_like(o_new)
    for i in range(1, int(N.max()) + 1):
        inner = np.zeros_like(o_new)
        for k in range(i):
            inner += float(comb(i - 1, k)) * (-1.0) ** k / np.sqrt(k + 1.0) * o_new ** (k + 1)
        denom += np.where(i <= N, inner, 0.0)
    return denom


def denominator_hockey_stick(o_new, N):
    """The same sum collapsed with sum_{i=k+1..N} C(i-1, k) = C(N, k+1): sum_{k=0..N-1} C(N, k+1) (-1)^k o_new^(k+1) / sqrt(k+1)."""
    o_new = np.asarray(o_new, np.float64)
    out = np.zeros_like(o_new)
    for j in range(o_new.size):
        n = int(N[j])
        out[j] = sum(float(comb(n, k + 1)) * (-1.0) ** k * o_new[j] ** (k + 1) / np.sqrt(k + 1.0) for k in range(n))
    return out


def relocation(opacity_old, scale_old, N, n_max=N_MAX):
    """-> (opacity_new (n,), scale_new (n, 3), coefficient (n,)) as float64, from the float32 inputs."""
    o = np.asarray(opacity_old, np.float32).astype(np.float64).reshape(-1)
    s = np.asarray(scale_old, np.float32).astype(np.float64).reshape(-1, 3)
    N = clamp_N(N, n_max)
    o_new = 1.0 - np.power(1.0 - o, 1.0 / N)
    coef = o / denominator_double_loop(o_new, N)
    return o_new, coef[:, None] * s, coef


def relocation_kernel_order(opacity_old, scale_old, N, n_max=N_MAX):
    """The kernel's evaluation order: float64 internals, o_new = -expm1(log1p(-o) / N), the collapsed sum in ascending k with the binomial
    and the signed power from their recurrences, each term (c * p) / sqrt(k + 1); the two results rounded to float32 once."""
    o = np.asarray(opacity_old, np.float32).astype(np.float64).reshape(-1)
    s = np.asarray(scale_old, np.float32).astype(np.float64).reshape(-1, 3)
    N = clamp_N(N, n_max)
    x = -np.expm1(np.log1p(-o) / N.astype(np.float64))
    c, p, total = N.astype(np.float64), x.copy(), np.zeros_like(x)
    for k in range(int(N.max())):
        live = k < N
        total = np.where(live, total + (c * p) / np.sqrt(float(k + 1)), total)
        c = (c * (N - k - 1).astype(np.float64)) / float(k + 2)
        p = p * -x
    coef = o / total
    return x.astype(np.float32), (coef[:, None] * s).astype(np.float32)


def relocation_inputs(n=4097, seed=20):
    """(opacity_old (n,), scale_old (n, 3), N (n,) int64) -- the first n rows of ONE pool of 4097, so that every smaller case is a subset of the
    largest: first the cross product of the opacities {0.005, 0.5, 0.9, 0.99, 0.999, 1 - 2^-23} with every N in 1..50 and 0, -3, 51, 1000 (which
    must behave as clamped) in a fixed shuffle, then opacities from U[0.005, 0.999] with N uniform in 1..50.  Scales exp(U[-6, 1])."""
    rng = np.random.default_rng(seed)
    total = 4097
    assert n <= total
    special_o = np.array([0.005, 0.5, 0.9, 0.99, 0.999, 1.0 - 2.0 ** -23], np.float32)
    special_N = np.array(list(range(1, 51)) + [0, -3, 51, 1000], np.int64)
    oo, nn = np.meshgrid(special_o, special_N, indexing="ij")
    order = rng.permutation(oo.size)
    rest = total - oo.size
    o = np.concatenate([oo.reshape(-1)[order], rng.uniform(0.005, 0.999, rest).astype(np.float32)]).astype(np.float32)
    N = np.concatenate([nn.reshape(-1)[order], rng.integers(1, 51, rest)]).astype(np.int64)
    s = np.exp(rng.uniform(-6.0, 1.0, (total, 3))).astype(np.float32)
    return o[:n].copy(), s[:n].copy(), N[:n].copy()


def relocation_errors(got_o, got_s, opacity_old, scale_old, N):
    """The worst relative errors of opacity_new and of the scale_new components against the yardstick."""
    o_ref, s_ref, _ = relocation(opacity_old, scale_old, N)
    eo = np.abs(np.asarray(got_o, np.float64).reshape(-1) - o_ref) / o_ref
    es = np.abs(np.asarray(got_s, np.float64).reshape(-1, 3) - s_ref) / s_ref
    return float(eo.max()), float(es.max())


# ---- the position noise ------------------------------------------------------------------------------------------------------------------

def _rotation(q, dtype):
    """build_rotation: (P, 4) quaternions (w, x, y, z), normalised here, -> (P, 3, 3)"""
    q = q / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3), dtype)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def noise_step(scales, rotations, opacities, noise, noise_scale, raw=False, k=100.0, x0=0.995):
    """-> (dxyz (P, 3), gate (P,), v = noise * gate * noise_scale (P, 3), s (P, 3)) as float64: the displacement upstream's composition adds to
    xyz, and the quantities the tolerance is stated in."""
    s, q, o, w = (np.asarray(a, np.float32).astype(np.float64) for a in (scales, rotations, opacities, noise))
    o = o.reshape(-1)
    noise_scale, k, x0 = f32(noise_scale), f32(k), f32(x0)
    with np.errstate(all="ignore"):
        if raw:
            o, s = 1.0 / (1.0 + np.exp(-o)), np.exp(s)
        L = _rotation(q, np.float64) * s[:, None, :]          # R @ diag(s)
        sigma = L @ np.transpose(L, (0, 2, 1))
        gate = 1.0 / (1.0 + np.exp(-k * ((1.0 - o) - x0)))
        v = w * gate[:, None] * noise_scale
        return (sigma @ v[:, :, None])[:, :, 0], gate, v, s


def noise_kernel_order(scales, rotations, opacities, noise, noise_scale, raw=False, k=100.0, x0=0.995):
    """The kernel's evaluation order in float32: v = (noise * g) * noise_scale, u = R^T v, u *= s * s, d = R u (Sigma is never formed)."""
    one, two = np.float32(1), np.float32(2)
    s, q, o, w = (np.asarray(a, np.float32) for a in (scales, rotations, opacities, noise))
    o = o.reshape(-1)
    noise_scale, k, x0 = np.float32(noise_scale), np.float32(k), np.float32(x0)
    with np.errstate(all="ignore"):
        if raw:
            o, s = one / (one + np.exp(-o)), np.exp(s)
        g = one / (one + np.exp(-(k * ((one - o) - x0))))
        v = (w * g[:, None]) * noise_scale
        s2 = s * s
        norm = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        r, x, y, z = (q[:, j] / norm for j in range(4))
        R = np.empty((q.shape[0], 3, 3), np.float32)
        R[:, 0, 0] = one - two * (z * z + y * y); R[:, 0, 1] = two * (x * y - r * z); R[:, 0, 2] = two * (r * y + x * z)
        R[:, 1, 0] = two * (r * z + x * y); R[:, 1, 1] = one - two * (z * z + x * x); R[:, 1, 2] = two * (y * z - r * x)
        R[:, 2, 0] = two * (x * z - r * y); R[:, 2, 1] = two * (r * x + y * z); R[:, 2, 2] = one - two * (y * y + x * x)
        u = np.stack([((R[:, 0, j] * v[:, 0] + R[:, 1, j] * v[:, 1]) + R[:, 2, j] * v[:, 2]) * s2[:, j] for j in range(3)], axis=1)
        d = np.stack([(R[:, j, 0] * u[:, 0] + R[:, j, 1] * u[:, 1]) + R[:, j, 2] * u[:, 2] for j in range(3)], axis=1)
    assert d.dtype == np.float32
    return d


NOISE_SCALE = 0.8          # noise_lr * xyz_lr of a 3DGS-MCMC run at its end (5e5 * 1.6e-6)
NOISE_SIZES = (1, 63, 64, 65, 1000, 4099)
GATE_FLOOR = 1e-20         # the float64 gate above which the relative bound is asked
ABS_FLOOR = 1e-25          # the absolute allowance below it (float32 gates underflow there)


def noise_inputs(P, seed=30):
    """dict of float32 arrays for P Gaussians: scales exp(U[-6, 1]) with raw_scales = log of them, quaternions of random direction and norm in
    [0.2, 3], opacities U[0, 1] with 0, 1 and 0.005 among them (and raw_opacities = their logits, -inf and +inf included), standard normal
    noise with every seventh row zero, xyz U[-5, 5].  The non-raw and the raw inputs are equivalent up to the float32 rounding of log / logit;
    each mode is held against the yardstick of ITS OWN inputs."""
    rng = np.random.default_rng(seed + P)
    scales = np.exp(rng.uniform(-6.0, 1.0, (P, 3))).astype(np.float32)
    q = rng.standard_normal((P, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.2, 3.0, (P, 1))).astype(np.float32)
    o = rng.uniform(0.0, 1.0, P).astype(np.float32)
    for j, value in enumerate((0.005, 0.0, 1.0)):   # (P = 1: the 0.005 that is relocated next)
        if j < P:
            o[(j * 29) % P if P > 3 else j] = value
    noise = rng.standard_normal((P, 3)).astype(np.float32)
    noise[6::7] = 0.0
    with np.errstate(all="ignore"):
        raw_o = (np.log(o.astype(np.float64)) - np.log1p(-o.astype(np.float64))).astype(np.float32)
    return {"xyz": rng.uniform(-5.0, 5.0, (P, 3)).astype(np.float32), "scales": scales, "raw_scales": np.log(scales.astype(np.float64)).astype(np.float32),
            "rotations": q, "opacities": o, "raw_opacities": raw_o, "noise": noise}


def noise_args(inp, raw):
    return (inp["raw_scales"] if raw else inp["scales"], inp["rotations"], inp["raw_opacities"] if raw else inp["opacities"], inp["noise"])


def noise_error_ratio(dxyz, inp, raw, noise_scale=NOISE_SCALE):
    """(worst |dxyz - ref|_2 / (max(s)^2 |v|_2) over the rows whose float64 gate exceeds GATE_FLOOR,
        worst |dxyz - ref|_2 - ratio_bound over the other rows, as a function ratio -> excess)
    Rows with v = 0 (zero noise) must be exactly zero.  Below GATE_FLOOR the rows are held to  |dxyz - ref|_2 <= T max(s)^2 |v|_2 + ABS_FLOOR:
    the relative bound plus the absolute allowance for the underflow of the float32 gate."""
    ref, gate, v, s = noise_step(*noise_args(inp, raw), noise_scale, raw=raw)
    err = np.linalg.norm(np.asarray(dxyz, np.float64) - ref, axis=1)
    scale = np.max(s, axis=1) ** 2 * np.linalg.norm(v, axis=1)
    still = scale == 0
    assert np.all(np.asarray(dxyz)[still] == 0), "a row without noise moved"
    high = (gate > GATE_FLOOR) & ~still
    low = (gate <= GATE_FLOOR) & ~still
    ratio = float(np.max(err[high] / scale[high])) if high.any() else 0.0
    return ratio, (lambda T: float(np.max(err[low] - T * scale[low] - ABS_FLOOR)) if low.any() else -1.0)
