"""Restatement of gsx_mcmc_regularize / gsx_mcmc_perturb / gsx_mcmc_plan / gsx_mcmc_apply (include/gsx.h) in numpy and
Python integers; nothing of the package's kernels is imported.

The plan is exact integer arithmetic; the apply's relocation is float64 in the written order; the two float32 kernels are
restated twice, in float64 (``*_f64``: the formula) and as a float32 mirror in the kernel's operation order (``*_f32``)."""
import bisect
import math

import numpy as np

N_MAX = 51
TOP = 1.0 - 2.0 ** -24
COPY, ZERO_MOVED, OPACITY, SCALES = 0, 1, 2, 3
f32 = np.float32


def sigmoid64(o):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(o, np.float64)))


# ---------------------------------------------------------------------------------------------------- plan
def dead_rows(opacity, dead_logit):
    """opacity[i] <= dead_logit as a float32 comparison (a NaN fails it)."""
    with np.errstate(invalid="ignore"):
        return np.asarray(opacity, f32) <= f32(dead_logit)


def weights_of(opacity, dead_logit):
    """weights[i] = dead or non-finite ? 0 : max(1, rint(2^22 sigma(o_i))), the sigmoid in double."""
    o = np.asarray(opacity, f32)
    w = np.maximum(1.0, np.rint(4194304.0 * sigmoid64(np.where(np.isfinite(o), o, 0.0))))
    return np.where(dead_rows(o, dead_logit) | ~np.isfinite(o), 0.0, w).astype(np.uint32)


def plan(weights, opacity, dead_logit, n_out, uniforms):
    """(source int32 (n_out), count uint32 (n), (n_dead, n_live, n_new), draws) from the integer rule, on the weights given.
    draws: the (j, t, s) of every drawn row."""
    w = [int(v) for v in np.asarray(weights)]
    n = len(w)
    incl, total = [], 0
    for v in w:
        total += v
        incl.append(total)                      # P[s] + w[s]
    dead = dead_rows(opacity, dead_logit)
    source = np.zeros(n_out, np.int32)
    count = np.zeros(n, np.uint32)
    draws = []
    for j in range(n_out):
        if total == 0:
            source[j] = min(j, n - 1)
            continue
        if j < n and not dead[j]:
            source[j] = j
            continue
        t = min(total - 1, int(math.floor(float(uniforms[j]) * float(total))))
        s = bisect.bisect_right(incl, t)        # the first s with t < P[s] + w[s]; then P[s] <= t because P[s] = incl[s-1] <= t
        source[j] = s
        count[s] += 1
        draws.append((j, t, s))
    counts = (int(np.count_nonzero(dead)), int(np.count_nonzero(np.asarray(weights) != 0)) if total else 0, n_out - n)
    return source, count, counts, draws


# ---------------------------------------------------------------------------------------------------- apply
def relocation(a, N):
    """(x, D, coeff) of the published relocation in float64, the sums in the written order: one accumulator, i outer, k
    inner.  a is clamped to 1 - 2^-24 first."""
    a = min(float(a), TOP)
    x = -math.expm1(math.log1p(-a) / N)
    D = 0.0
    for i in range(1, N + 1):
        C, xp, sign = 1.0, x, 1.0
        for k in range(i):
            D = D + ((C * sign) * xp) / math.sqrt(k + 1.0)
            C = (C * (i - 1 - k)) / (k + 1.0)
            xp = xp * x
            sign = -sign
    return x, D, a / D


def relocated(opacity_logit, N, min_opacity):
    """(new opacity logit as float32, coeff as float64) of a source row with logit opacity_logit moved N-fold."""
    a = float(sigmoid64(f32(opacity_logit)))
    x, _, coeff = relocation(a, N)
    p = min(max(x, float(f32(min_opacity))), TOP)
    return f32(math.log(p / (1.0 - p))), coeff


def apply(groups, source, count, min_opacity):
    """groups: list of (src (n, width) float32, role).  Returns (outputs, moved): per group the (n_out, width) float32 array
    of the float64 restatement rounded to float32, and the boolean N > 1 per output row."""
    source = np.asarray(source, np.int64)
    count = np.asarray(count, np.int64)
    N = np.minimum(count[source] + 1, N_MAX)
    moved = N > 1
    opacity = next((src for src, role in groups if role == OPACITY), None)
    new_logit = np.zeros(len(source), f32)
    coeff = np.ones(len(source), np.float64)
    cache = {}
    for j in np.nonzero(moved)[0]:
        if opacity is None:
            break
        s = int(source[j])
        if s not in cache:
            cache[s] = relocated(opacity.reshape(-1)[s], int(N[j]), min_opacity)
        new_logit[j], coeff[j] = cache[s]
    outs = []
    for src, role in groups:
        src = np.asarray(src, f32).reshape(len(src), -1)
        out = src[source].copy()
        if role == ZERO_MOVED:
            out[moved] = 0.0
        elif role == OPACITY:
            out[moved, 0] = new_logit[moved]
        elif role == SCALES:
            out[moved] = (coeff[moved, None] * src[source[moved]].astype(np.float64)).astype(f32)
        outs.append(out)
    return outs, moved


# ---------------------------------------------------------------------------------------------------- regularize
def regularize_f64(opacity, scales, grad_opacity, grad_scales, lambda_opacity, lambda_scale):
    """The formula in float64 on the float32 inputs: (grad_opacity', grad_scales')."""
    n = len(opacity)
    sg = sigmoid64(opacity)
    go = np.asarray(grad_opacity, np.float64) + (float(lambda_opacity) / n) * sg * (1.0 - sg)
    gs = np.asarray(grad_scales, np.float64) + (float(lambda_scale) / (3.0 * n)) * np.sign(np.asarray(scales, np.float64))
    return go, gs


def regularize_f32(opacity, scales, grad_opacity, grad_scales, lambda_opacity, lambda_scale):
    """The kernel's float32 operation order; a lambda of 0 returns its array untouched."""
    n = len(opacity)
    o, s = np.asarray(opacity, f32), np.asarray(scales, f32)
    go, gs = np.array(grad_opacity, f32), np.array(grad_scales, f32)
    if f32(lambda_opacity) != 0:
        co = f32(float(f32(lambda_opacity)) / n)
        with np.errstate(over="ignore"):
            sg = f32(1) / (f32(1) + np.exp(-o))
        go = go + co * (sg * (f32(1) - sg))
    if f32(lambda_scale) != 0:
        cs = f32(float(f32(lambda_scale)) / (3.0 * n))
        gs = np.where(s > 0, gs + cs, np.where(s < 0, gs - cs, gs))
    return go.astype(f32), gs.astype(f32)


# ---------------------------------------------------------------------------------------------------- perturb
def _rotation(w, x, y, z, one, two):
    return [[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
            [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
            [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]]


def _delta(points, scales, quats, opacity, noise, rate, gate_k, gate_x0, T):
    """delta (n, 3) in the type T, the operation order of include/gsx.h."""
    one, two = T(1), T(2)
    s, q, e = np.asarray(scales, T), np.asarray(quats, T), np.asarray(noise, T)
    o = np.asarray(opacity, T)
    with np.errstate(all="ignore"):
        sg = one / (one + np.exp(-o))
        gate = one / (one + np.exp(-(T(gate_k) * ((one - sg) - T(gate_x0)))))
        nrm = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        w, x, y, z = q[:, 0] / nrm, q[:, 1] / nrm, q[:, 2] / nrm, q[:, 3] / nrm
        R = _rotation(w, x, y, z, one, two)
        v = [(s[:, c] * s[:, c]) * ((R[0][c] * e[:, 0] + R[1][c] * e[:, 1]) + R[2][c] * e[:, 2]) for c in range(3)]
        f = T(rate) * gate
        d = [f * ((R[k][0] * v[0] + R[k][1] * v[1]) + R[k][2] * v[2]) for k in range(3)]
    return np.stack(d, axis=1).astype(T)


def perturb_f64(points, scales, quats, opacity, noise, rate, gate_k, gate_x0):
    """(points', delta, kept): float64 on the float32 inputs; kept: rows whose delta is not finite and keep their bits."""
    d = _delta(points, scales, quats, opacity, noise, float(f32(rate)), float(f32(gate_k)), float(f32(gate_x0)), np.float64)
    kept = ~np.isfinite(d).all(axis=1)
    out = np.asarray(points, np.float64) + np.where(kept[:, None], 0.0, d)
    return out, d, kept


def perturb_f32(points, scales, quats, opacity, noise, rate, gate_k, gate_x0):
    """(points', delta, kept) in the kernel's float32 operation order."""
    d = _delta(points, scales, quats, opacity, noise, rate, gate_k, gate_x0, f32)
    kept = ~np.isfinite(d).all(axis=1)
    p = np.asarray(points, f32)
    with np.errstate(all="ignore"):
        out = np.where(kept[:, None], p, p + d).astype(f32)
    return out, d, kept


def perturb_norm(scales, noise, rate):
    """rate * max_c s_c^2 * |eps|_2 per row, float64: what the perturbation's error is measured against."""
    s, e = np.asarray(scales, np.float64), np.asarray(noise, np.float64)
    return float(f32(rate)) * (s * s).max(axis=1) * np.sqrt((e * e).sum(axis=1))


# ---------------------------------------------------------------------------------------------------- shared inputs
STEP_SIZES = (1, 255, 257, 1000)
STEP_RULES = dict(lambda_opacity=0.01, lambda_scale=0.01, rate=5e5 * 1.6e-4, gate_k=100.0, gate_x0=0.995)


def step_inputs(n, seed=0):
    """The rows tests/test_mcmc_host.py measures the float32 mirrors on and tests/test_hip_mcmc.py runs the two per-step
    kernels on: trained-like magnitudes (scales 0.003 .. 0.3 log-uniform, quaternions not normalised, logits normal(-2, 3),
    gradients of the magnitude of the regularisers' own coefficients) and, from five rows up, row 1 a zero quaternion, row 2
    a NaN in the noise, row 3 opaque (logit 9: gate ~ 0), row 4 nearly dead (logit -7: gate ~ 1), row 0 one zero and one
    negative scale."""
    rs = np.random.RandomState(4000 + 7 * seed + n)
    c = dict(points=rs.normal(0, 3, size=(n, 3)), scales=np.exp(rs.uniform(np.log(0.003), np.log(0.3), size=(n, 3))),
             quats=rs.normal(size=(n, 4)) * np.exp(rs.uniform(-1, 1, size=(n, 1))), opacity=rs.normal(-2, 3, size=n),
             noise=rs.normal(size=(n, 3)), grad_opacity=rs.normal(size=n) * (STEP_RULES["lambda_opacity"] / n),
             grad_scales=rs.normal(size=(n, 3)) * (STEP_RULES["lambda_scale"] / (3 * n)))
    c = {k: np.ascontiguousarray(v, f32) for k, v in c.items()}
    if n >= 5:
        c["scales"][0, 0], c["scales"][0, 1] = 0.0, -0.02
        c["quats"][1] = 0.0
        c["noise"][2, 1] = np.nan
        c["opacity"][3], c["opacity"][4] = 9.0, -7.0
    return c


def regularize_error(got_opacity, got_scales, c, lambda_opacity, lambda_scale):
    """max |got - float64 restatement| in units of the regulariser's own coefficient (lambda / n, lambda / (3 n)): the
    larger of the two sides; a side whose lambda is 0 does not enter."""
    n = len(c["opacity"])
    go, gs = regularize_f64(c["opacity"], c["scales"], c["grad_opacity"], c["grad_scales"], lambda_opacity, lambda_scale)
    err = 0.0
    if lambda_opacity:
        err = max(err, float(np.abs(np.asarray(got_opacity, np.float64) - go).max() / (lambda_opacity / n)))
    if lambda_scale:
        err = max(err, float(np.abs(np.asarray(got_scales, np.float64) - gs).max() / (lambda_scale / (3.0 * n))))
    return err
