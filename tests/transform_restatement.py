"""gsx_transform_gaussians (include/gsx.h) restated in numpy float32, operation for operation: every product and every sum
is one float32 operation on float32 arrays, in the order the header states (the library is built with -ffp-contract=off), so
the kernel's arrays are reproducible from here bit for bit.  ``host_arguments`` makes the float32 arguments from a validated
triple exactly as ``Gaussians.transform`` does (float64 on the host, rounded once)."""
import numpy as np

F = np.float32


def host_arguments(sim):
    """dict of float32 arrays R (3,3), s (), t (3,), q (4,), M1, M2, M3: what the kernel is handed for ``sim``."""
    from intro_to_gaussian_splatting_amd.transform import sh_rotation_matrices

    M1, M2, M3 = sh_rotation_matrices(sim.R)
    return dict(R=np.asarray(sim.R, np.float64).astype(F), s=F(sim.s), t=np.asarray(sim.t, np.float64).astype(F),
                q=np.asarray(sim.q, np.float64).astype(F), M1=M1.astype(F), M2=M2.astype(F), M3=M3.astype(F))


def transform(points, scales, quats, sh, degree, a):
    """(points', scales', quats', sh' or None) float32, from float32 inputs and the float32 arguments ``a``."""
    p, c, q = (np.ascontiguousarray(v, F) for v in (points, scales, quats))
    R, s, t = a["R"].astype(F), F(a["s"]), a["t"].astype(F)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    P = np.stack([s * ((R[k, 0] * x + R[k, 1] * y) + R[k, 2] * z) + t[k] for k in range(3)], axis=1)
    C = s * c
    aw, ax, ay, az = (F(v) for v in a["q"])
    bw, bx, by, bz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    Q = np.stack([((aw * bw - ax * bx) - ay * by) - az * bz,
                  ((aw * bx + ax * bw) + ay * bz) - az * by,
                  ((aw * by - ax * bz) + ay * bw) + az * bx,
                  ((aw * bz + ax * by) - ay * bx) + az * bw], axis=1)
    for out in (P, C, Q):
        assert out.dtype == F
    if sh is None:
        return P, C, Q, None
    S = np.array(sh, dtype=F, copy=True)
    assert S.shape[1:] == ((degree + 1) ** 2, 3)
    for l in range(1, degree + 1):
        M = a["M%d" % l].astype(F)
        m, o = 2 * l + 1, l * l
        v = np.array(S[:, o:o + m, :], copy=True)          # (n, m, 3)
        for i in range(m):
            acc = M[i, 0] * v[:, 0, :]
            for j in range(1, m):
                acc = acc + M[i, j] * v[:, j, :]
            assert acc.dtype == F
            S[:, o + i, :] = acc
    return P, C, Q, S


def sh_colors_float32(points, sh, degree, center):
    """The float32 mirror of gsx_sh_to_rgb's chain (csrc/gsx_sh_device.h: basis_at, pre_clamp, eval), every operation a
    float32 one in the device's order, except that the direction is normalised here by a float32 division by the float32
    root where the device multiplies by the reciprocal.  (n, 3) float32."""
    import sh_backward_restatement as sr

    p = np.ascontiguousarray(points, F)
    cx, cy, cz = (F(v) for v in center)
    dx, dy, dz = p[:, 0] - cx, p[:, 1] - cy, p[:, 2] - cz
    norm = np.sqrt(dx * dx + dy * dy + dz * dz)
    x, y, z = dx / norm, dy / norm, dz / norm
    C0, C1 = F(sr.C0), F(sr.C1)
    C2, C3 = [F(v) for v in sr.C2], [F(v) for v in sr.C3]
    basis = [np.full(len(p), C0, F)]
    if degree > 0:
        basis += [-C1 * y, C1 * z, -C1 * x]
    if degree > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        two, three, four = F(2), F(3), F(4)
        basis += [C2[0] * xy, C2[1] * yz, C2[2] * (two * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy)]
        if degree > 2:
            basis += [C3[0] * y * (three * xx - yy), C3[1] * xy * z, C3[2] * y * (four * zz - xx - yy),
                      C3[3] * z * (two * zz - three * xx - three * yy), C3[4] * x * (four * zz - xx - yy),
                      C3[5] * z * (xx - yy), C3[6] * x * (xx - three * yy)]
    S = np.ascontiguousarray(sh, F)
    acc = np.zeros((len(p), 3), F)
    for k, b in enumerate(basis):
        acc = acc + b[:, None] * S[:, k, :]
    out = np.maximum(acc + F(0.5), F(0))
    assert out.dtype == F
    return out
