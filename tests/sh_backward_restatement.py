"""Float64 restatement of the SH colour (gsx_sh_to_rgb) and of its backward (gsx_sh_backward), with a per-entry error scale.

Forward: colour_c = max(0, 0.5 + sum_k Y_k(d) sh[k][c]), d = v / |v|, v = mean - camera centre.  Backward, for g = dL/dcolour
and m_c = [pre-clamp value > 0]:
    dL/dsh[k][c] = Y_k(d) m_c g_c
    dL/dmean     = (g_d - d (d . g_d)) / |v|,   g_d = sum_k (sum_c m_c g_c sh[k][c]) dY_k/dd
Every Y_k is held as a list of monomials (coefficient, power of x, of y, of z): its value, its derivative (term by term, so
the derivatives here are not the hand-written ones of csrc/gsx_sh_device.h) and its ERROR SCALE all come from that one
list.  The error scale of an output is the same formula evaluated on absolute values of every term and factor --
|C2c| (2 zz + xx + yy) stands for basis 6, sum |g_c| |sh[k][c]| |dY_k| for the mean -- which is what a float32 evaluation
can lose per unit roundoff, whatever order it sums in.

The constants are the float32 values the kernels hold.
"""
import numpy as np

_f = lambda v: float(np.float32(v))  # noqa: E731
C0 = _f(0.28209479177387814)
C1 = _f(0.4886025119029199)
C2 = [_f(1.0925484305920792), _f(-1.0925484305920792), _f(0.31539156525252005), _f(-1.0925484305920792),
      _f(0.5462742152960396)]
C3 = [_f(-0.5900435899266435), _f(2.890611442640554), _f(-0.4570457994644658), _f(0.3731763325901154),
      _f(-0.4570457994644658), _f(1.445305721320277), _f(-0.5900435899266435)]

# Y_k as monomials (coefficient, ex, ey, ez) of the unit direction (x, y, z)
TERMS = [
    [(C0, 0, 0, 0)],
    [(-C1, 0, 1, 0)],
    [(C1, 0, 0, 1)],
    [(-C1, 1, 0, 0)],
    [(C2[0], 1, 1, 0)],
    [(C2[1], 0, 1, 1)],
    [(2 * C2[2], 0, 0, 2), (-C2[2], 2, 0, 0), (-C2[2], 0, 2, 0)],
    [(C2[3], 1, 0, 1)],
    [(C2[4], 2, 0, 0), (-C2[4], 0, 2, 0)],
    [(3 * C3[0], 2, 1, 0), (-C3[0], 0, 3, 0)],
    [(C3[1], 1, 1, 1)],
    [(4 * C3[2], 0, 1, 2), (-C3[2], 2, 1, 0), (-C3[2], 0, 3, 0)],
    [(2 * C3[3], 0, 0, 3), (-3 * C3[3], 2, 0, 1), (-3 * C3[3], 0, 2, 1)],
    [(4 * C3[4], 1, 0, 2), (-C3[4], 3, 0, 0), (-C3[4], 1, 2, 0)],
    [(C3[5], 2, 0, 1), (-C3[5], 0, 2, 1)],
    [(C3[6], 3, 0, 0), (-3 * C3[6], 1, 2, 0)],
]


def _derivative(terms, axis):
    out = []
    for term in terms:
        e = list(term[1:])
        if e[axis] == 0:
            continue
        coef = term[0] * e[axis]
        e[axis] -= 1
        out.append((coef, e[0], e[1], e[2]))
    return out


def _poly(terms, d, absolute):
    """sum of the monomials at d (n,3); absolute: every coefficient and coordinate by its absolute value."""
    d = np.abs(d) if absolute else d
    out = np.zeros(d.shape[0])
    for coef, ex, ey, ez in terms:
        out += (abs(coef) if absolute else coef) * d[:, 0] ** ex * d[:, 1] ** ey * d[:, 2] ** ez
    return out


def basis(d, degree, absolute=False):
    """Y (n,K) at unit directions d (n,3)."""
    k = (degree + 1) ** 2
    return np.stack([_poly(TERMS[i], d, absolute) for i in range(k)], axis=1)


def basis_gradient(d, degree, absolute=False):
    """dY_k/d(x,y,z) (n,K,3) of the polynomials, unconstrained (the caller projects onto the sphere's tangent plane)."""
    k = (degree + 1) ** 2
    return np.stack([np.stack([_poly(_derivative(TERMS[i], a), d, absolute) for a in range(3)], axis=1) for i in range(k)],
                    axis=1)


def forward(points, sh, degree, center):
    """(pre-clamp colour (n,3), mask (n,3) bool, d (n,3), |v| (n,), Y (n,K)) in float64."""
    v = np.asarray(points, np.float64) - np.asarray(center, np.float64)[None, :]
    norm = np.sqrt((v * v).sum(1))
    d = v / norm[:, None]
    Y = basis(d, degree)
    pre = 0.5 + np.einsum("nk,nkc->nc", Y, np.asarray(sh, np.float64))
    return pre, pre > 0, d, norm, Y


def colors(points, sh, degree, center):
    return np.maximum(forward(points, sh, degree, center)[0], 0.0)


def backward(points, sh, degree, center, grad_colors):
    """(dL/dsh (n,K,3), dL/dmean (n,3), scale of dL/dsh (n,K,3), scale of dL/dmean (n,3)) in float64.
    The zero-row rule (include/gsx.h, gsx_sh_backward): a row whose dL/dcolour is zero in all three channels -- every row
    the frame listed nowhere -- gets exact zeros in all four, whatever its mean and coefficients hold; no view direction is
    formed for it (a NaN mean, or a mean on the camera centre, has none)."""
    sh = np.asarray(sh, np.float64)
    g = np.asarray(grad_colors, np.float64)
    live = g.any(1)
    if not live.all():
        n, k = sh.shape[0], sh.shape[1]
        out = [np.zeros((n, k, 3)), np.zeros((n, 3)), np.zeros((n, k, 3)), np.zeros((n, 3))]
        if live.any():
            for full, part in zip(out, backward(np.asarray(points)[live], sh[live], degree, center, g[live])):
                full[live] = part
        return tuple(out)
    pre, mask, d, norm, Y = forward(points, sh, degree, center)
    gm = np.where(mask, g, 0.0)
    grad_sh = Y[:, :, None] * gm[:, None, :]
    scale_sh = basis(d, degree, absolute=True)[:, :, None] * np.abs(g)[:, None, :]
    t = np.einsum("nc,nkc->nk", gm, sh)
    t_abs = np.einsum("nc,nkc->nk", np.abs(gm), np.abs(sh))
    gd = np.einsum("nk,nka->na", t, basis_gradient(d, degree))
    gd_abs = np.einsum("nk,nka->na", t_abs, basis_gradient(d, degree, absolute=True))
    grad_mean = (gd - d * (d * gd).sum(1, keepdims=True)) / norm[:, None]
    scale_mean = (gd_abs + np.abs(d) * (np.abs(d) * gd_abs).sum(1, keepdims=True)) / norm[:, None]
    if degree == 0:
        grad_mean, scale_mean = np.zeros_like(grad_mean), np.zeros_like(scale_mean)
    return grad_sh, grad_mean, scale_sh, scale_mean


def scaled_error(got, ref, scale, keep=None):
    """max |got - ref| / scale over the entries `keep` (bool, broadcastable) selects; an entry whose scale is 0 must be
    exact (its error counts as infinite otherwise)."""
    diff = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(scale > 0, diff / scale, np.where(diff == 0, 0.0, np.inf))
    if keep is not None:
        e = np.where(np.broadcast_to(keep, e.shape), e, 0.0)
    return float(e.max()) if e.size else 0.0


# The inputs of the kernel test (tests/test_hip_sh_backward.py) and of the float32 reference error
# (tests/test_sh_backward_host.py): the shapes of the forward's edge test, because the staging is the same code.
CASES = [(1, 3, 0), (255, 1, 0), (256, 2, 0), (257, 3, 0), (1000, 2, 1), (513, 0, 0), (70001, 3, 0)]
CENTER = np.array([0.3, -0.2, 4.0], np.float32)
NEAR_ZERO = 1e-5        # channels whose pre-clamp value is nearer to 0 may clamp either way in float32: left out


def case_inputs(n, degree, skip):
    """(points (n+skip,3), sh (n+skip,K,3), grad_colors (n+skip,3)) float32, seeded by n + degree."""
    rs = np.random.RandomState(n + degree)
    k = (degree + 1) ** 2
    pts = rs.normal(size=(n + skip, 3)).astype(np.float32)
    sh = rs.normal(size=(n + skip, k, 3)).astype(np.float32)
    gc = rs.normal(size=(n + skip, 3)).astype(np.float32)
    return pts, sh, gc
