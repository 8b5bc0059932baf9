"""Float64 yardstick of the fused photometric loss (include/stp_raster.h: stp_photometric_forward / stp_photometric_backward), and the bounds
the tests hold the kernels to.  Torch on the CPU.

With x = image, y = target (float32 values, widened), every (H, W) plane on its own, n = the number of elements:
    w_k = exp(-(k - 5)^2 / 4.5) / sum, k = 0 .. 10: the ELEVEN FLOAT32 ROUNDINGS of these values, widened (WINDOW) -- the kernel's table, so
          that a comparison measures the arithmetic and not the table
    blur = 2-D correlation with the outer product of w, zero padding of 5  (F.conv2d(..., padding=5, groups=C))
    mu1 = blur(x), mu2 = blur(y), s1 = blur(x^2) - mu1^2, s2 = blur(y^2) - mu2^2, s12 = blur(x y) - mu1 mu2, C1 = 0.01^2, C2 = 0.03^2
    A = 2 mu1 mu2 + C1, B = 2 s12 + C2, Cc = mu1^2 + mu2^2 + C1, D = s1 + s2 + C2,   m = A B / (Cc D)
    out = [mean |x - y|, mean m]
    d1 = 2 mu2 B / (Cc D) - 2 mu2 A / (Cc D) - 2 mu1 A B / (Cc^2 D) + 2 mu1 A B / (Cc D^2),  d2 = -A B / (Cc D^2),  d3 = 2 A / (Cc D)
    dL/dx = blur(s d1) + 2 x blur(s d2) + y blur(s d3) + (g0 / n) sign(x - y),   s = g1 / n, sign(0) = 0, (g0, g1) = dL/dout

terms() and grad() take switches (dtype, padding, shift, C2, drop_d2) that the CPU tests use to run the SAME formulas in float32 and to break
them on purpose; the yardstick is the default of every switch."""
import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

U = 2.0 ** -24          # unit roundoff of float32
# K: the roundings a value can meet on its way into one blurred statistic of the kernel, the unit of every bound below.  Counted from
# csrc/stp_loss.hip: the input product (1) + per pass of the window one pair addition and a chain of one product and five fused
# multiply-adds (<= 6) x 2 passes = 13; the gradient's terms: the scale by s (1) + 12 + the combination (2 fused multiply-adds and an
# addition: 3) = 16.  The plain form of the window (11 + 11 fused multiply-adds + the product, 23) is covered as well.
K = 24
C1, C2 = 0.01 ** 2, 0.03 ** 2

_k = np.arange(11, dtype=np.float64)
_w = np.exp(-(_k - 5.0) ** 2 / 4.5)
WINDOW32 = (_w / _w.sum()).astype(np.float32)            # the kernel's constexpr table
WINDOW = torch.from_numpy(WINDOW32.astype(np.float64))   # ... widened


def tile():
    """(TW, TH): the output tile of a workgroup of the kernels, read from the one place that states it (include/stp_raster.h)."""
    h = open(os.path.join(ROOT, "include", "stp_raster.h")).read()
    return tuple(int(re.search(r"#define\s+STP_PHOTOMETRIC_TILE_%s\s+(\d+)\b" % a, h).group(1)) for a in "WH")


def reduction_chain(planes, H, W):
    """L: the longest chain of additions between a pixel's value and a sum of the forward, counted from csrc/stp_loss.hip: a thread adds its
    4 pixels (4, the first to 0.0), the butterfly of a wave64 (6), the four waves in order (3) -> one row per workgroup; the sum kernel's
    thread t adds rows t, t + 256, ... (ceil(groups / 256), the first to 0.0), then the same butterfly (6) and waves (3).  Two of these
    additions are to an exact zero and round nothing; the rounding of |x - y| and of the division by n take their place."""
    TW, TH = tile()
    groups = planes * math.ceil(H / TH) * math.ceil(W / TW)
    return 4 + 6 + 3 + math.ceil(groups / 256) + 6 + 3


def planes_of(a, dtype=torch.float64):
    """(C, H, W) or (B, C, H, W) float32 values -> (planes, 1, H, W) of dtype."""
    a = torch.as_tensor(np.asarray(a, dtype=np.float32)) if not isinstance(a, torch.Tensor) else a.detach().cpu().to(torch.float32)
    assert a.dim() in (3, 4)
    return a.reshape(-1, 1, a.shape[-2], a.shape[-1]).to(dtype)


def blur(v, padding="zeros", shift=0):
    """v: (planes, 1, H, W).  padding "zeros" is the definition; "replicate" and a window shifted by `shift` pixels along x are mutations."""
    w = WINDOW.to(v.dtype)
    w2 = (w[:, None] * w[None, :])[None, None]
    if padding == "zeros" and shift == 0:
        return F.conv2d(v, w2, padding=5)
    mode = "constant" if padding == "zeros" else "replicate"
    return F.conv2d(F.pad(v, (5 + shift, 5 - shift, 5, 5), mode=mode), w2)


def maps_of(mu1, mu2, e11, e22, e12, c2=C2):
    """(m, d1, d2, d3) elementwise from the five blurred statistics."""
    s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    A, B, Cc, D = 2 * mu1 * mu2 + C1, 2 * s12 + c2, mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + c2
    m = A * B / (Cc * D)
    d1 = 2 * mu2 * B / (Cc * D) - 2 * mu2 * A / (Cc * D) - 2 * mu1 * A * B / (Cc * Cc * D) + 2 * mu1 * A * B / (Cc * D * D)
    d2 = -A * B / (Cc * D * D)
    d3 = 2 * A / (Cc * D)
    return m, d1, d2, d3


def _statistics(x, y, **kw):
    return blur(x, **kw), blur(y, **kw), blur(x * x, **kw), blur(y * y, **kw), blur(x * y, **kw)


def terms_t(x, y, padding="zeros", shift=0, c2=C2):
    """The differentiable form: x, y (planes, 1, H, W) tensors -> (2,) tensor."""
    m = maps_of(*_statistics(x, y, padding=padding, shift=shift), c2=c2)[0]
    return torch.stack([(x - y).abs().mean(), m.mean()])


def terms(x, y, dtype=torch.float64, **kw):
    """out = [mean |x - y|, mean SSIM] as a (2,) tensor of dtype."""
    return terms_t(planes_of(x, dtype), planes_of(y, dtype), **kw)


def grad(x, y, g0, g1, dtype=torch.float64, padding="zeros", shift=0, c2=C2, drop_d2=False):
    """dL/dx by the closed form, (planes, 1, H, W) of dtype."""
    x, y = planes_of(x, dtype), planes_of(y, dtype)
    n = x.numel()
    kw = dict(padding=padding, shift=shift)
    _, d1, d2, d3 = maps_of(*_statistics(x, y, **kw), c2=c2)
    s = torch.tensor(g1, dtype=dtype) / n
    g = blur(s * d1, **kw) + y * blur(s * d3, **kw) + (torch.tensor(g0, dtype=dtype) / n) * torch.sign(x - y)
    if not drop_d2:
        g = g + 2 * x * blur(s * d2, **kw)
    return g


def bounds(x, y, g0, g1, K=K):
    """(bound of out (2,), bound of dL/dx (planes, 1, H, W)): what float32 arithmetic with at most K roundings per blurred statistic may be
    off by, counted and not tuned.  Each of the five blurred statistics: K u blur(|.|).  Through m, d1, d2, d3 to first order (the
    elementwise Jacobian by float64 autograd) plus K u |value|.  The gradient: those through the second blur and the products with |x| and
    |y|, plus K u times the blurred magnitudes (and K u |g0 / n| where the L1 term is not zero).  out[1]: the mean of the map's bound plus the
    reduction's own (L + 1) u mean |m|;  out[0]: (L + 1) u out[0]  (L: reduction_chain)."""
    x, y = planes_of(x), planes_of(y)
    n = x.numel()
    L = reduction_chain(x.shape[0], x.shape[2], x.shape[3])
    inputs = (x, y, x * x, y * y, x * y)
    stats = [blur(v).requires_grad_(True) for v in inputs]
    stat_err = [K * U * blur(v.abs()) for v in inputs]
    values = maps_of(*stats)
    value_err = []
    for f in values:
        jac = torch.autograd.grad(f.sum(), stats, retain_graph=True, allow_unused=True)   # (d3 does not depend on every statistic)
        value_err.append(sum(j.abs() * e for j, e in zip(jac, stat_err) if j is not None) + K * U * f.detach().abs())
    m, d1, d2, d3 = (f.detach() for f in values)
    em, e1, e2, e3 = value_err
    out0 = (x - y).abs().mean()
    out_bound = torch.stack([(L + 1) * U * out0, em.mean() + (L + 1) * U * m.abs().mean()])
    s, l1w = abs(g1) / n, abs(g0) / n
    grad_bound = (s * (blur(e1) + 2 * x.abs() * blur(e2) + y.abs() * blur(e3))
                  + K * U * s * (blur(d1.abs()) + 2 * x.abs() * blur(d2.abs()) + y.abs() * blur(d3.abs()))
                  + K * U * l1w * (x != y).to(x.dtype))
    return out_bound, grad_bound


def images(family, planes, H, W, seed=0):
    """The input families of the tests, float32 (planes, H, W) arrays (image, target)."""
    rng = np.random.default_rng(seed)
    if family == "random":
        return rng.random((planes, H, W), dtype=np.float32), rng.random((planes, H, W), dtype=np.float32)
    if family == "smooth":   # what a render looks like: smooth plus 2 % noise (sigma^2 = E[x^2] - mu^2 cancels)
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        base = np.stack([0.5 + 0.4 * np.sin(0.11 * xx + 0.07 * yy + p) * np.cos(0.05 * yy - 0.3 * p) for p in range(planes)])
        img = np.clip(base + 0.02 * rng.standard_normal((planes, H, W)), 0.0, 1.0).astype(np.float32)
        tgt = np.clip(base + 0.02 * rng.standard_normal((planes, H, W)), 0.0, 1.0).astype(np.float32)
        return img, tgt
    if family == "constant":
        return np.full((planes, H, W), 0.7, np.float32), np.full((planes, H, W), 0.2, np.float32)
    if family == "identical":
        a = rng.random((planes, H, W), dtype=np.float32)
        return a, a.copy()
    raise ValueError(family)
