"""Similarity transforms of the world, x' = s R x + t: the host side of gsx_transform_gaussians (include/gsx.h).

Everything the kernel is handed is made here, in float64, and rounded to float32 once: the validated triple
(``similarity``), the quaternion of the rotation (``rotation_quaternion``, w >= 0) and the matrices that rotate the
spherical-harmonic coefficients of bands 1..3 in THIS build's basis, the constants and signs of csrc/gsx_sh_device.h
(``sh_rotation_matrices``).  ``compose`` and ``inverse`` work on such triples.  Host arithmetic only (numpy); the arrays of
a container are transformed by ``Gaussians.transform`` / ``GaussianScene.transform``, on the GPU, and nowhere else.
"""
from __future__ import annotations

from typing import NamedTuple, Tuple

import numpy as np

# csrc/gsx_sh_device.h, in double
_C1 = 0.4886025119029199
_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
       1.445305721320277, -0.5900435899266435)


def _band(l: int, d: np.ndarray) -> np.ndarray:
    """(m, 2 l + 1) float64: the basis functions of band ``l`` (1..3) at the unit directions ``d`` (m, 3), as
    sh::basis_at of csrc/gsx_sh_device.h writes them."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    if l == 1:
        cols = [-_C1 * y, _C1 * z, -_C1 * x]
    elif l == 2:
        cols = [_C2[0] * xy, _C2[1] * yz, _C2[2] * (2.0 * zz - xx - yy), _C2[3] * xz, _C2[4] * (xx - yy)]
    else:
        cols = [_C3[0] * y * (3.0 * xx - yy), _C3[1] * xy * z, _C3[2] * y * (4.0 * zz - xx - yy),
                _C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), _C3[4] * x * (4.0 * zz - xx - yy), _C3[5] * z * (xx - yy),
                _C3[6] * x * (xx - 3.0 * yy)]
    return np.stack(cols, axis=1)


def _fixed_directions(m: int = 64) -> np.ndarray:
    """``m`` unit directions spread evenly over the sphere (a golden-angle spiral): a fixed set, so the matrices are a
    function of R alone."""
    i = np.arange(m, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / m
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


_DIRS = _fixed_directions()
# Band l is orthonormal on the sphere, so Y_l(R d) = D_l(R) Y_l(d) with D_l orthogonal, and the defining property
# Y_l(R d)^T M_l c = Y_l(d)^T c for all d and c says M_l = D_l.  With B = Y_l at the fixed directions (64 x (2 l + 1), full
# column rank, condition number below 1.2) and B' = Y_l at the rotated ones: B'^T = D_l B^T, so D_l = B'^T pinv(B^T) -- exact
# up to float64 rounding, since B' lies in the column space that pinv inverts.
_PINV = {l: np.linalg.pinv(_band(l, _DIRS).T) for l in (1, 2, 3)}


def _as_rotation(R) -> np.ndarray:
    R = np.array(R, dtype=np.float64)
    if R.shape != (3, 3):
        raise ValueError("R must be a 3 x 3 matrix, got shape %s" % (R.shape,))
    if not np.isfinite(R).all():
        raise ValueError("R holds a value that is not finite")
    if np.abs(R @ R.T - np.eye(3)).max() > 1e-6:
        raise ValueError("R is not orthonormal to 1e-6: max|R R^T - I| = %.3g" % np.abs(R @ R.T - np.eye(3)).max())
    if np.linalg.det(R) < 0.0:
        raise ValueError("det R < 0: R is a reflection, which has no quaternion")
    return R


def sh_rotation_matrices(R) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(M1, M2, M3)``, float64, 3 x 3, 5 x 5 and 7 x 7: the matrices that take the SH coefficients of bands 1..3 of a
    Gaussian into the world rotated by ``R``, in this build's basis: ``Y_l(R d)^T M_l c = Y_l(d)^T c`` for every unit ``d``.
    Orthogonal, ``M_l(I) = I`` and ``M_l(R1 R2) = M_l(R1) M_l(R2)``, all to float64 rounding."""
    R = _as_rotation(R)
    rotated = _DIRS @ R.T
    return tuple(_band(l, rotated).T @ _PINV[l] for l in (1, 2, 3))


def rotation_quaternion(R) -> np.ndarray:
    """(w, x, y, z) float64, unit, w >= 0: the quaternion of the proper rotation ``R`` in the convention of the R[i][j]
    table of include/gsx.h.  The largest of the four candidates is taken from the diagonal (no cancellation)."""
    R = _as_rotation(R)
    t = np.array([R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2],
                  R[2, 2] - R[0, 0] - R[1, 1]])
    k = int(np.argmax(t))
    r = np.sqrt(1.0 + t[k])
    if k == 0:
        q = np.array([r * r, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif k == 1:
        q = np.array([R[2, 1] - R[1, 2], r * r, R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif k == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], r * r, R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], r * r])
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0.0 else q


class Similarity(NamedTuple):
    """x' = s R x + t: ``R`` (3, 3) and ``t`` (3,) float64, ``s`` a float.  Unpacks as ``(R, s, t)``."""
    R: np.ndarray
    s: float
    t: np.ndarray

    @property
    def q(self) -> np.ndarray:
        """The quaternion of ``R``, (w, x, y, z), w >= 0."""
        return rotation_quaternion(self.R)

    def apply(self, x) -> np.ndarray:
        """float64 (..., 3): the transform of the points ``x`` (host arithmetic: for cameras and tests)."""
        return self.s * (np.asarray(x, np.float64) @ self.R.T) + self.t


def similarity(R, s: float = 1.0, t=0) -> Similarity:
    """The validated triple.  Refused with ValueError: ``R`` not 3 x 3 or not orthonormal to 1e-6, ``det R < 0`` (a
    reflection has no quaternion), ``s <= 0``, anything that is not finite."""
    R = _as_rotation(R)
    s = float(s)
    if not np.isfinite(s):
        raise ValueError("s = %r is not finite" % (s,))
    if not s > 0.0:
        raise ValueError("s = %r is not positive" % (s,))
    t = np.zeros(3) if t is None else np.array(t, dtype=np.float64)
    if t.shape == ():
        t = np.full(3, float(t))
    if t.shape != (3,):
        raise ValueError("t must be 3 numbers, got shape %s" % (t.shape,))
    if not np.isfinite(t).all():
        raise ValueError("t holds a value that is not finite")
    return Similarity(R, s, t)


def compose(outer, inner) -> Similarity:
    """``outer`` after ``inner``: x -> outer(inner(x))."""
    a, b = similarity(*outer), similarity(*inner)
    return Similarity(a.R @ b.R, a.s * b.s, a.s * (a.R @ b.t) + a.t)


def inverse(triple) -> Similarity:
    """The transform that undoes ``triple``: x = R^T (x' - t) / s."""
    a = similarity(*triple)
    return Similarity(a.R.T.copy(), 1.0 / a.s, -(a.R.T @ a.t) / a.s)
