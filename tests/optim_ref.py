"""The clipped step of include/s2vt_hip.h ("clipped step": s2vt_grad_norm + s2vt_adam_step_clipped) restated in numpy: every
product and sum of the step in fp32, one rounding each, the norm's sum of squares in fp64.  A helper of the tests, not a test."""
import numpy as np

f32 = np.float32


def grad_norm_ref(g):
    """fp32(sqrt(sum of fp64 squares)): an fp32 square is exact in fp64, so only the additions and the final rounding round"""
    g64 = np.asarray(g, dtype=np.float64)
    with np.errstate(all="ignore"):
        return f32(np.sqrt(np.sum(g64 * g64)))


def scale_ref(norm, max_norm):
    """clip_grad_norm_'s coefficient in fp32: min(fp32(max_norm) / (norm + 1e-6f), 1), NaN staying NaN; 1 without clipping"""
    if max_norm is None or not max_norm > 0:
        return f32(1.0)
    with np.errstate(all="ignore"):
        coef = f32(max_norm) / (f32(norm) + f32(1e-6))
    return f32(1.0) if coef >= f32(1.0) else f32(coef)


def step_ref(p, g, m, v, t, lr, b1, b2, eps, max_norm=None, wd=0.0, decoupled=False, decay_mask=None, skip_nonfinite=False):
    """One step on the fp32 numpy arrays p, m, v IN PLACE (g is left alone: the clipped gradient is not written back).
    t counts from 1.  decay_mask: per-element bools (None: every element is decayed).  Returns (grad_norm, scale, skipped)."""
    assert p.dtype == g.dtype == m.dtype == v.dtype == np.float32
    norm = grad_norm_ref(g)
    sc = scale_ref(norm, max_norm)
    if skip_nonfinite and not np.isfinite(norm):
        return norm, sc, True
    with np.errstate(all="ignore"):
        gg = g * sc
        if wd != 0.0:
            dm = np.ones(p.shape, dtype=bool) if decay_mask is None else np.asarray(decay_mask, dtype=bool)
            if decoupled:
                p[dm] = p[dm] * f32(1.0 - lr * wd)
            else:
                gg[dm] = gg[dm] + f32(wd) * p[dm]
        w1, w2 = f32(1.0 - b1), f32(1.0 - b2)
        step_size = f32(lr / (1.0 - b1 ** t))
        bc2_sqrt = f32(np.sqrt(1.0 - b2 ** t))
        m[:] = m + (gg - m) * w1
        v[:] = f32(b2) * v + w2 * gg * gg
        denom = np.sqrt(v) / bc2_sqrt + f32(eps)
        p[:] = p - step_size * (m / denom)
    return norm, sc, False
