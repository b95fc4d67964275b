"""gsx_adam_step restated in numpy (include/gsx.h): ``step32`` is the formula in float32, op for op -- every operation a
numpy float32 operation, rounded on its own, divide and sqrt correctly rounded as numpy's are -- and is what a LINEAR
group's parameter and every group's moments must equal bit for bit; the LOG exponential is taken in float64 and rounded
once (the device library's expf is within an ulp of that, not equal to it).  ``step64`` is the same formula in float64
from the same hyper-parameters, i.e. the float32 values the C ABI receives.

The host scalars are the library's: from the float32 beta1 / beta2 / lr, in double, rounded to float32 once.
"""
import math

import numpy as np

F = np.float32
LINEAR, LOG = 0, 1


def host_scalars(lr, beta1, beta2, step, dtype=np.float32):
    """c1, c2, a = lr / (1 - beta1^step), s2 = sqrt(1 - beta2^step) as gsx_adam_step computes them; ``dtype`` float64 keeps
    the doubles (step64)."""
    lr, b1, b2, step = float(F(lr)), float(F(beta1)), float(F(beta2)), int(step)
    assert step >= 1
    t = dtype
    return dict(beta1=t(b1), beta2=t(b2), c1=t(1.0 - b1), c2=t(1.0 - b2), a=t(lr / (1.0 - math.pow(b1, step))),
                s2=t(math.sqrt(1.0 - math.pow(b2, step))))


def live_rows(grads):
    """GSX_ADAM_SKIP_ZERO_ROWS: the rows (bool, n) that are NOT skipped -- some gradient element of the row in some group
    has a bit set besides the sign (NaN counts, -0 does not).  grads: float32 arrays of n rows each."""
    live = None
    for g in grads:
        g = np.ascontiguousarray(g, np.float32)
        bits = (g.view(np.uint32) & np.uint32(0x7FFFFFFF)).reshape(g.shape[0], -1)
        row = (bits != 0).any(axis=1)
        live = row if live is None else (live | row)
    return live


def _step(p, g, m, v, k, eps, transform, dtype, rows):
    with np.errstate(all="ignore"):
        gp = g * p if transform == LOG else g
        m2 = k["beta1"] * m + k["c1"] * gp
        v2 = k["beta2"] * v + (k["c2"] * gp) * gp
        d = np.sqrt(v2) / k["s2"] + eps
        u = k["a"] * (m2 / d)
        if transform == LOG:
            p2 = p * np.exp(-u.astype(np.float64)).astype(dtype)
        else:
            p2 = p - u
    for a in (p2, m2, v2):
        assert a.dtype == dtype, a.dtype
    if rows is not None:
        keep = ~np.asarray(rows, bool)
        p2[keep], m2[keep], v2[keep] = p[keep], m[keep], v[keep]
    return p2, m2, v2


def step32(p, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, transform=LINEAR, rows=None):
    """One step of one group in float32: (p', m', v'), new arrays.  rows: None (dense) or the bool mask of live_rows --
    the other rows keep their bits."""
    p, g, m, v = (np.ascontiguousarray(a, np.float32) for a in (p, g, m, v))
    return _step(p, g, m, v, host_scalars(lr, beta1, beta2, step), F(eps), transform, np.float32, rows)


def step64(p, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, transform=LINEAR, rows=None):
    """The same in float64 (the hyper-parameters are the float32 values the C ABI receives; the host scalars stay double)."""
    p, g, m, v = (np.ascontiguousarray(a, np.float64) for a in (p, g, m, v))
    return _step(p, g, m, v, host_scalars(lr, beta1, beta2, step, np.float64), np.float64(F(eps)), transform, np.float64, rows)
