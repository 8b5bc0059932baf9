"""Float64 yardstick of the dense Adam step (include/stp_raster.h: stp_dense_adam; GaussianAdam), and the bounds the tests hold the kernel --
and torch.optim.Adam, the thing it replaces -- to.

step(): from the float32 inputs, in float64, with the coefficients formed as the host forms them (coefficients(): in float64 from the Python
values, 1 - beta from the UNROUNDED beta as torch does, each rounded to float32 once):
    g' = g + r      r = 0 | c s (1 - s), s = 1 / (1 + exp(-p)) | c exp(p)      c = weight / numel
    m <- b1 m + omb1 g'      v <- b2 v + omb2 g' g'      p <- p - step_size m / (sqrt(v) / bias2_sqrt + eps)

bounds(): counted from float32 roundings, u = 2^-24 = 6e-8 being the relative error of one correctly rounded operation.

  dg, the error of g':   6e-7 |r| + 1.2e-7 |g'|   (+ 2e-7 c s for "sigmoid")
      exp: a library expf within 2 ulp (2.4e-7) and the product with c (u): 3e-7 |r|; torch's own exp and the yardstick's libm differ by as
      much again: 6e-7 |r|.  sigmoid: s carries expf (4u on e = exp(-p), which moves s by at most that, relatively), the sum 1 + e (u) and the
      quotient (u): 6u relative; the products s (1 - s) and c (...) add 2u: within 6e-7 |r| as far as the error is relative to s.  The float32
      difference 1 - s is exact (Sterbenz) for s >= 1/2 but inherits the ABSOLUTE error of s, up to 1.5 u near s = 1 (half an ulp of 1 + e and
      the quotient's), which c s multiplies: 1.5 u c s, written 2e-7 c s.  The sum g + r rounds once (u |g'|); a second u |g'| for an
      implementation that accumulates r into g in another order (autograd's sign and mean factors): 1.2e-7 |g'|.
  bm:  5e-7 (|b1 m| + |omb1 g'|) + omb1 dg
      the product omb1 g' (u), the fma (u), a lerp-form m + omb1 (g' - m) (torch's: three roundings on terms no larger than |m| + |g'|) and the
      result's own rounding stay below 8u of the terms' magnitudes; dg passes through omb1.
  bv:  5e-7 v_ref + 2 omb2 |g'| dg
      all terms are positive, so every rounding is relative to v_ref: b2 v (u), omb2 g' (u), times g' (u), the sum (u), within 8u; the
      derivative of omb2 g'^2 carries dg.
  bp:  2.5e-6 S + step_size bm / den + S dden / den + 1.2e-7 |p|
      with den = sqrt(v_ref) / bias2_sqrt + eps, S = step_size (|b1 m| + |omb1 g'|) / den (the step's magnitude, with the cancellation in m
      taken out) and dden = bv / (2 sqrt(v_ref) bias2_sqrt), the error v's passes to den.  The chain's own roundings -- an approximate root
      (1 ulp = 2u), the quotient by bias2_sqrt (u), + eps (u), step_size m (u), the quotient (u), or step_size (m / den) -- are 7u of the step,
      allowed 2.5e-6 S = 42u as the sparse step's yardstick allows 2e-6 and for a root of 2 ulp and a reciprocal-multiply variant of either
      quotient; the final difference rounds once relative to the result (u |p| for a step smaller than |p|, 2u written).
  Where v_ref = 0 (g' = 0 and v = 0: then m's terms are exact) dden is 0.

bounds(carried=(Ep, Em, Ev)) adds what errors of the INPUTS (an implementation that has run k steps of its own in float32 against a yardstick
that has run them in float64) become, to first order: Em and Ev shrink by b1 and b2, Ep passes to p unchanged and, through the regulariser
(|dr/dp| <= |r| for both kinds), into dg; the totals take bm's and bv's place in bp.  That is the ACCUMULATED bound of the multi-step tests."""
import numpy as np


def f32(x):
    """A Python float rounded to float32 once, as a float64."""
    return float(np.float32(x))


def coefficients(lr, eps, t, b1=0.9, b2=0.999, weight=0.0, numel=1):
    """The float32-rounded coefficients (as float64 values) of step t >= 1, formed in float64 from the Python values: torch's convention."""
    return dict(b1=f32(b1), omb1=f32(1.0 - b1), b2=f32(b2), omb2=f32(1.0 - b2), step_size=f32(lr / (1.0 - b1 ** t)),
                bias2_sqrt=f32((1.0 - b2 ** t) ** 0.5), eps=f32(eps), c=f32(weight / max(numel, 1)))


def _widen(*arrays):
    return tuple(np.asarray(a, np.float32).astype(np.float64) if np.asarray(a).dtype != np.float64 else np.asarray(a) for a in arrays)


def regulariser(p64, kind, c):
    """-> (r, s): the regulariser's gradient at p and, for "sigmoid", s (else None)"""
    with np.errstate(all="ignore"):
        if kind is None:
            return np.zeros_like(p64), None
        if kind == "sigmoid":
            s = 1.0 / (1.0 + np.exp(-p64))
            return c * (s * (1.0 - s)), s
        if kind == "exp":
            return c * np.exp(p64), None
    raise ValueError(kind)


def step(p, g, m, v, lr, eps, t, b1=0.9, b2=0.999, reg=None):
    """(p, m, v) after step t, float64 arrays.  p, g, m, v: float32 arrays (or float64 ones: the yardstick's own earlier results, taken as they are);
    reg: None or (kind, weight)."""
    p64, g64, m64, v64 = _widen(p, g, m, v)
    kind, weight = reg if reg is not None else (None, 0.0)
    k = coefficients(lr, eps, t, b1, b2, weight, p64.size)
    r, _ = regulariser(p64, kind, k["c"])
    with np.errstate(all="ignore"):
        gr = g64 + r
        m_new = k["b1"] * m64 + k["omb1"] * gr
        v_new = k["b2"] * v64 + k["omb2"] * gr * gr
        p_new = p64 - k["step_size"] * m_new / (np.sqrt(v_new) / k["bias2_sqrt"] + k["eps"])
    return p_new, m_new, v_new


def bounds(p, g, m, v, lr, eps, t, b1=0.9, b2=0.999, reg=None, carried=None):
    """(bm, bv, bp, dg) of step t from the inputs p, g, m, v (the module's text counts them); carried = (Ep, Em, Ev): the errors the inputs p, m, v
    of the implementation under test already carry against these."""
    p64, g64, m64, v64 = _widen(p, g, m, v)
    kind, weight = reg if reg is not None else (None, 0.0)
    k = coefficients(lr, eps, t, b1, b2, weight, p64.size)
    r, s = regulariser(p64, kind, k["c"])
    Ep, Em, Ev = carried if carried is not None else (0.0, 0.0, 0.0)
    with np.errstate(all="ignore"):
        gr = g64 + r
        v_ref = k["b2"] * v64 + k["omb2"] * gr * gr
        dg = 6e-7 * np.abs(r) + 1.2e-7 * np.abs(gr) + np.abs(r) * Ep
        if kind == "sigmoid":
            dg = dg + 2e-7 * k["c"] * s
        mag = np.abs(k["b1"] * m64) + np.abs(k["omb1"] * gr)
        bm = 5e-7 * mag + k["omb1"] * dg + k["b1"] * Em
        bv = 5e-7 * v_ref + 2.0 * k["omb2"] * np.abs(gr) * dg + k["b2"] * Ev
        root = np.sqrt(v_ref)
        den = root / k["bias2_sqrt"] + k["eps"]
        S = k["step_size"] * mag / den
        dden = np.where(v_ref > 0, bv / np.where(v_ref > 0, 2.0 * root * k["bias2_sqrt"], 1.0), 0.0)
        bp = 2.5e-6 * S + k["step_size"] * bm / den + S * dden / den + 1.2e-7 * np.abs(p64) + Ep
    return bm, bv, bp, dg


def make_inputs(shape, seed, p_log_uniform_to=None):
    """p, g, m, v as float32 arrays: |g| and |m| are 0 or in [1e-8, 1], v is 0 or in [1e-16, 1] (log-uniform): no denormals, no underflow of g * g.
    5 % of the elements have m = v = 0, half of those g = 0 as well; 10 % of g are zeros in all.  p is +-[1e-2, 10] log-uniform, or, for the
    regularisers, +-[1e-3, p_log_uniform_to]."""
    rng = np.random.default_rng(seed)
    logu = lambda lo, hi=0.0: 10.0 ** rng.uniform(lo, hi, shape)
    sign = lambda: rng.choice([-1.0, 1.0], shape)
    u = rng.random(shape)
    g = np.where((u < 0.025) | ((u >= 0.05) & (u < 0.125)), 0.0, sign() * logu(-8)).astype(np.float32)
    m = np.where(u < 0.05, 0.0, sign() * logu(-8)).astype(np.float32)
    v = np.where(u < 0.05, 0.0, logu(-16)).astype(np.float32)
    p = (sign() * (logu(-3) * 10.0 if p_log_uniform_to is None else logu(-3, np.log10(p_log_uniform_to)))).astype(np.float32)
    return p, g, m, v
