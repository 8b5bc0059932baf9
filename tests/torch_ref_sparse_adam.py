"""Float64 yardstick of the sparse Adam step (include/stp_raster.h: stp_sparse_adam), and the bounds the GPU tests hold the kernel to.

step(): from the float32 inputs, in float64, with b1, b2, lr and eps first rounded to float32 and 1 - b formed from the rounded value
(exact in float32 for b in [0.5, 1], so that the float64 difference IS the float32 one):
    m <- b1 m + (1 - b1) g      v <- b2 v + (1 - b2) g g      p <- p - lr m / (sqrt(v) + eps)
for the visible rows; invisible rows are returned unchanged (the float32 values, widened)."""
import numpy as np


def f32(x):
    """A Python float rounded to float32 once, as a float64."""
    return float(np.float32(x))


def visible_rows(visible):
    """bool / uint8: non-zero = visible; int32 radii: > 0 = visible."""
    visible = np.asarray(visible)
    return visible > 0 if visible.dtype == np.int32 else visible != 0


def step(p, g, m, v, visible, lr, eps, b1=0.9, b2=0.999):
    """(p, m, v) after one step, float64 arrays of p's shape.  p, g, m, v: float32 arrays whose first axis is the Gaussian."""
    rows = visible_rows(visible)
    p64, g64, m64, v64 = (np.asarray(a, np.float32).astype(np.float64) for a in (p, g, m, v))
    b1, b2, lr, eps = f32(b1), f32(b2), f32(lr), f32(eps)
    with np.errstate(all="ignore"):
        m_new = b1 * m64 + (1.0 - b1) * g64
        v_new = b2 * v64 + (1.0 - b2) * g64 * g64
        p_new = p64 - lr * m_new / (np.sqrt(v_new) + eps)
    sel = rows.reshape((-1,) + (1,) * (p64.ndim - 1))
    return np.where(sel, p_new, p64), np.where(sel, m_new, m64), np.where(sel, v_new, v64)


def bounds(g, m, visible, v_ref, p, lr, eps, b1=0.9, b2=0.999):
    """The tolerances of the visible rows, from counting float32 roundings (one ulp allowed for reciprocal and square root each):
        m: 5e-7 (|b1 m| + |(1 - b1) g|)     v: 5e-7 v_ref     p: 2e-6 lr (|b1 m| + |(1 - b1) g|) / (sqrt(v_ref) + eps) + 1.2e-7 |p|
    g, m, p: the float32 inputs; v_ref: the yardstick's new v."""
    g64, m64, p64 = (np.asarray(a, np.float32).astype(np.float64) for a in (g, m, p))
    b1, lr, eps = f32(b1), f32(lr), f32(eps)
    mag = np.abs(b1 * m64) + np.abs((1.0 - b1) * g64)
    with np.errstate(all="ignore"):
        return 5e-7 * mag, 5e-7 * v_ref, 2e-6 * lr * mag / (np.sqrt(v_ref) + eps) + 1.2e-7 * np.abs(p64)
