"""Float64 yardstick of the training loss (include/stp_raster.h: stp_training_loss_forward / _backward; training_terms, training_loss), built
on tests/torch_ref_photometric.py, and the bounds the tests hold the kernels to.  Torch on the CPU.

With x = image (B, 3, H, W), E = exposure (B, 3, 4), y = target:
    v_j = sum_i x_i E[i][j] + E[j][3]           (the row index is the INPUT channel: matmul(x.permute(1, 2, 0), E[:3, :3]) + E[:3, 3])
    v clamped to [0, 1] with clamp              x'' = v * alpha_mask
    out = [mean |x'' - y|, mean SSIM(x'', y), mean |(d - m) * depth_mask|]          (ref.terms_t on x'' for the first two)
    g'_j = g''_j * alpha_mask * [0 <= v_j <= 1 or no clamp],   g'' = dL/dx'' (ref.grad)
    dL/dx_i = sum_j E[i][j] g'_j      dL/dE[i][j] = sum_p x_i g'_j      dL/dE[j][3] = sum_p g'_j      (per image)
    dL/dd = (g2 / n_d) sign((d - m) mask) mask

The kernel (csrc/stp_loss.hip) evaluates v_j as ONE float32 chain fma(E[2][j], x_2, fma(E[1][j], x_1, fma(E[0][j], x_0, E[j][3]))): on the
dyadic family below every product and sum of it is exact, so x'' has the same bits whatever the order, and the GPU tests can demand
bit-equality with the plain photometric call on x''.

The switches (transpose, mask_first, clamp_passes_all, mask_twice; halo_bias_terms) are the mutations of the CPU tests; the yardstick is the
default of every switch."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import torch_ref_photometric as ref

U = ref.U


def batch4(a, dtype=torch.float64):
    """(C, H, W) or (B, C, H, W) values -> (B, C, H, W) tensor of dtype."""
    a = torch.as_tensor(np.asarray(a)) if not isinstance(a, torch.Tensor) else a.detach().cpu()
    return (a[None] if a.dim() == 3 else a).to(dtype)


def exposure3(E, B, dtype=torch.float64):
    """(3, 4) or (B, 3, 4) -> (B, 3, 4) tensor of dtype."""
    E = torch.as_tensor(np.asarray(E)) if not isinstance(E, torch.Tensor) else E.detach().cpu()
    return (E[None].expand(B, 3, 4) if E.dim() == 2 else E).to(dtype)


def pre_clamp(x, E, transpose=False):
    """v (B, 3, H, W) from x (B, 3, H, W) and E (B, 3, 4) or None."""
    if E is None:
        return x
    M = E[:, :, :3].transpose(1, 2) if transpose else E[:, :, :3]
    return torch.einsum("bihw,bij->bjhw", x, M) + E[:, :, 3][:, :, None, None]


def exposed(x, E=None, clamp=False, mask=None, transpose=False, mask_first=False):
    """x'' (B, C, H, W); mask (B, 1, H, W), (1, 1, H, W) or None."""
    if mask_first and mask is not None:
        x = x * mask
    v = pre_clamp(x, E, transpose)
    if clamp:
        v = v.clamp(0.0, 1.0)
    if mask is not None and not mask_first:
        v = v * mask
    return v


def depth_term_t(d, m, mask=None):
    v = d - m
    if mask is not None:
        v = v * mask
    return v.abs().mean()


def terms_t(x, y, E=None, clamp=False, mask=None, d=None, m=None, dmask=None, **switches):
    """The differentiable form on (B, C, H, W) tensors -> (3,) tensor."""
    xpp = exposed(x, E, clamp, mask, **switches)
    two = ref.terms_t(xpp.reshape(-1, 1, *xpp.shape[-2:]), y.reshape(-1, 1, *y.shape[-2:]))
    third = depth_term_t(d, m, dmask) if d is not None else torch.zeros((), dtype=x.dtype)
    return torch.cat([two, third[None]])


def halo_bias_terms(x, y, E, clamp=False):
    """MUTATION: out[:2] when the window's halo outside the image is staged as the exposure's bias E[j][3] (clamped) instead of 0."""
    xpp = exposed(x, E, clamp)
    B, C, H, W = xpp.shape
    fill = E[:, :, 3].clamp(0.0, 1.0) if clamp else E[:, :, 3]
    padded = fill[:, :, None, None].expand(B, C, H + 10, W + 10).clone()
    padded[:, :, 5:-5, 5:-5] = xpp
    xp, yp = padded.reshape(-1, 1, H + 10, W + 10), F.pad(y.reshape(-1, 1, H, W), (5, 5, 5, 5))
    w = ref.WINDOW.to(x.dtype)
    w2 = (w[:, None] * w[None, :])[None, None]
    blur = lambda v: F.conv2d(v, w2)
    m = ref.maps_of(blur(xp), blur(yp), blur(xp * xp), blur(yp * yp), blur(xp * yp))[0]
    return torch.stack([(xpp - y).abs().mean(), m.mean()])


def chain(gpp, x, E=None, clamp=False, mask=None, clamp_passes_all=False):
    """(dL/dx (B, C, H, W), dL/dE (B, 3, 4) or None, g') from g'' = dL/dx'' (B, C, H, W): the formulas of the header in float64."""
    g = gpp
    if mask is not None:
        g = g * mask
    if clamp and not clamp_passes_all:
        v = pre_clamp(x, E)
        g = g * ((v >= 0.0) & (v <= 1.0)).to(g.dtype)
    if E is None:
        return g, None, g
    dx = torch.einsum("bjhw,bij->bihw", g, E[:, :, :3])
    dE = torch.zeros_like(E)
    dE[:, :, :3] = torch.einsum("bihw,bjhw->bij", x, g)
    dE[:, :, 3] = g.sum(dim=(2, 3))
    return dx, dE, g


def depth_grad(d, m, mask, g2, mask_twice=False):
    """(g2 / n_d) sign((d - m) mask) mask"""
    v = d - m
    if mask is not None:
        v = v * mask
    g = (g2 / d.numel()) * torch.sign(v)
    if mask is not None:
        g = g * mask * (mask if mask_twice else 1.0)
    return g


# ---- the bounds, counted from csrc/stp_loss.hip ------------------------------------------------------------------------------------------------
def exposure_chain(rows):
    """The longest chain of additions between a pixel's product and an entry of dL/dE: a thread's four pixels (fused multiply-adds from 0.0),
    the butterfly of a wave64 (6), the four waves (3) -> one row per (image, tile) workgroup; exposure_sum_kernel's thread t adds the rows
    t, t + 256, ... of the `rows` an output sums, then the same butterfly and waves."""
    return 4 + 6 + 3 + math.ceil(rows / 256) + 6 + 3


def tiles_of(H, W):
    TW, TH = ref.tile()
    return math.ceil(H / TH) * math.ceil(W / TW)


SPARE = 2   # see chain_bounds


def _gamma(k):
    return k * U / (1.0 - k * U)


def chain_bounds(gpp, x, E, clamp, mask, shared_exposure=False):
    """(bound of dL/dx, bound of dL/dE or None) for float32 arithmetic as the kernel's:
    g' = g'' * mask is ONE rounding (none without a mask; the clamp's factor is exact).
    dL/dx_i: a chain of three fused multiply-adds from 0 over E[i][j] g'_j: 3 roundings + g's 1 = 4 -> gamma(2 * 4) sum_j |E[i][j] g'_j|;
             without an exposure dL/dx = g': gamma(2 * 1) |g'|.  (SPARE = 2: an exact count of so few roundings is reached to within a few
             per cent by ANY correct float32 evaluation, the plain torch one included, which the CPU test wants inside with a factor 2 to
             spare; a wrong formula is off by a fraction of the value, six orders of magnitude beyond either.)
    dL/dE:   the products are fused into the additions (no rounding of their own): the chain of exposure_chain(rows) additions + g's 1
             -> gamma(L + 1) sum_p |x_i g'_j|, rows = the (image, tile) workgroups an entry sums (all images' for a shared exposure)."""
    _, _, g = chain(gpp, x, E, clamp, mask)
    if E is None:
        return _gamma(SPARE * 1) * g.abs(), None
    dx_bound = _gamma(SPARE * 4) * torch.einsum("bjhw,bij->bihw", g.abs(), E[:, :, :3].abs())
    B, _, H, W = x.shape
    L = exposure_chain(tiles_of(H, W) * (B if shared_exposure else 1))
    dE_bound = torch.zeros_like(E)
    dE_bound[:, :, :3] = torch.einsum("bihw,bjhw->bij", x.abs(), g.abs())
    dE_bound[:, :, 3] = g.abs().sum(dim=(2, 3))
    return dx_bound, _gamma(L + 1) * dE_bound


def depth_bounds(d, m, mask, g2):
    """(bound of out[2], bound of dL/dd).  out[2]: d - m and the product with the mask are a rounding each, the sum is the forward's chain
    (ref.reduction_chain of the depth planes) and the division by n_d one more: gamma(L + 3) out[2].  dL/dd: g2 / n_d and the product with
    sign * mask: 2 -> gamma(2 * 2) |value| (SPARE, as in chain_bounds)."""
    planes, H, W = int(np.prod(d.shape[:-2])), d.shape[-2], d.shape[-1]
    L = ref.reduction_chain(planes, H, W)
    return _gamma(L + 3) * depth_term_t(d, m, mask), _gamma(SPARE * 2) * depth_grad(d, m, mask, g2).abs()


# ---- the input families ---------------------------------------------------------------------------------------------------------------------------
def dyadic(shape, seed=0, bias=None):
    """Exact inputs: (x, y, E, mask) float32 arrays for shape (3, H, W) or (B, 3, H, W).  x: multiples of 2^-8 in [0, 1] (a fifth of them at
    each end); E: multiples of 2^-6, diagonal in [0.75, 1.5], the rest in [-0.25, 0.25] (bias: every E[j][3] set to it), one (3, 4) for a
    (3, H, W) image, (B, 3, 4) for a batch; mask: multiples of 2^-4 in [0, 1], a fifth of them 0, (1, H, W) or (B, 1, H, W); y: any
    float32 in [0, 1].  Every product and sum of the transform needs at most 21 bits: x'' is exact in float32 in any order."""
    rng = np.random.default_rng(seed)
    B = shape[0] if len(shape) == 4 else 1
    H, W = shape[-2:]
    x = np.clip(np.round(rng.uniform(-0.3, 1.3, (B, 3, H, W)) * 256.0) / 256.0, 0.0, 1.0)
    E = np.round(rng.uniform(-0.25, 0.25, (B, 3, 4)) * 64.0) / 64.0
    for i in range(3):
        E[:, i, i] = np.round(rng.uniform(0.75, 1.5, B) * 64.0) / 64.0
    if bias is not None:
        E[:, :, 3] = bias
    mask = np.round(rng.uniform(0.0, 1.0, (B, 1, H, W)) * 16.0) / 16.0
    mask[rng.random((B, 1, H, W)) < 0.2] = 0.0
    y = rng.random((B, 3, H, W), dtype=np.float32)
    f = lambda a: np.ascontiguousarray(a if len(shape) == 4 else a[0], np.float32)
    return f(x), f(y), f(E), f(mask)


def depth_inputs(shape, seed=0):
    """(d, m, mask) float32 arrays (1, H, W) or (B, 1, H, W): a tenth of the pixels with d == m, a fifth with mask == 0, masks in [0, 1]."""
    rng = np.random.default_rng(seed + 1000)
    s = ((shape[0],) if len(shape) == 4 else ()) + (1,) + tuple(shape[-2:])
    d, m = rng.random(s, dtype=np.float32), rng.random(s, dtype=np.float32)
    same = rng.random(s) < 0.1
    m[same] = d[same]
    mask = rng.random(s, dtype=np.float32)
    mask[rng.random(s) < 0.2] = 0.0
    return d, m, mask


def clamp_fractions(x, E):
    """(below 0, above 1, inside) fractions of the elements of v."""
    x = batch4(x)
    v = pre_clamp(x, exposure3(E, x.shape[0]))
    return float((v < 0).double().mean()), float((v > 1).double().mean()), float(((v >= 0) & (v <= 1)).double().mean())
