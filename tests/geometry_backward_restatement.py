"""Float64 restatement of the geometry gradients of the reference's frame (the CPU pin of gsx_render_backward_geometry).

The reference's graph reaches the points, scales and quaternions once its Gaussian weight stays a tensor
(tools/capture_geometry_grad_golden.py).  What that graph computes, restated:

Compositing.  Per (record k, pixel p): d = mean_k - pixel, power = -1/2 d^T Q d with Q the record's 2x2 inverse
covariance as stored, alpha = exp(power) op, and u = dL/dalpha alpha = dL/dpower with dL/dalpha as
tests/backward_restatement.py has it.  Then
    dL/dQ_ij = -1/2 sum_p u d_i d_j          dL/dmean = -1/2 (Q + Q^T) sum_p u d
so five moments per Gaussian: S = (sum u d0, sum u d1, sum u d0^2, sum u d0 d1, sum u d1^2) (`moments`).  Everything is
float64 except the stop decision, which follows the reference's float32 T and alpha (backward_restatement._alpha32).

Chain (`chain`), per Gaussian, float64 from the float32 inputs:
  1  Q = adj(cov2d) / max(det, 1e-3), det = c00 c11 - c01 c10; where det < 1e-3 only the adjugate carries gradient
  2  cov2d = (T Sigma T^T)[:2,:2], T = J W; J00 = fx / z, J02 = -fx cx / z^2, J11 = fy / z, J12 = -fy cy / z^2,
     cx = clamp(tx / z, +-1.3 tan_fovx) z (active clamp: d cx / d tx = 0, d cx / d z = the clamp value)
  3  Sigma = M M^T, M = R diag(s), linear scales
  4  R of the quaternion (w, x, y, z) normalised twice
  5  pixel mean = ((h_xy / h_w) + 1)(dim - 1) / 2, h = [p, 1] @ full_proj
  6  dL/dpoint = 5 through full_proj + the view-space point's gradient of 2 through world2view
The tile rectangle, radius, culling and depth order are piecewise constant: no gradient.

with_scale=True also returns a per-Gaussian error scale for each output: the same chain run on ABSOLUTE values -- the
moments replaced by sum ua |d0|, ... with ua the bound of the terms u itself adds up (`moments`), every Jacobian entry by its absolute value, every difference by a sum -- i.e. the
sum of the absolute values of the terms the gradient adds up.  A float32 implementation's error on a Gaussian is a small
multiple of the unit roundoff times that scale, however small the gradient itself is through cancellation
(backward_restatement.per_gaussian_error; `per_gaussian_error` here applies it per output).
"""
from __future__ import annotations

import numpy as np

from backward_restatement import SUBNORMAL, _alpha32
from oracle import cpu_ref

f32 = np.float32


def stage1(points, scales, quats, cam) -> dict:
    """Float64 stage 1 of every row (no culling): pixel mean `xy`, `Q` (2,2) and the intermediates `chain` needs."""
    p = np.asarray(points, np.float64)
    s = np.asarray(scales, np.float64)
    q = np.asarray(quats, np.float64)
    V, F = np.asarray(cam.world2view, np.float64), np.asarray(cam.full_proj, np.float64)
    n1 = np.maximum(np.sqrt((q * q).sum(1)), 1e-12)
    a = q / n1[:, None]
    n2 = np.sqrt((a * a).sum(1))
    b = a / n2[:, None]
    w, x, y, z = b.T
    R = np.empty((p.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    M = R * s[:, None, :]
    Sg = M @ M.transpose(0, 2, 1)
    ph = np.concatenate([p, np.ones((p.shape[0], 1))], 1)
    t = (ph @ V)[:, :3]
    tz = t[:, 2]
    limx, limy = 1.3 * float(cam.tan_fovx), 1.3 * float(cam.tan_fovy)
    rx, ry = t[:, 0] / tz, t[:, 1] / tz
    kx, ky = np.clip(rx, -limx, limx), np.clip(ry, -limy, limy)
    inx, iny = (rx >= -limx) & (rx <= limx), (ry >= -limy) & (ry <= limy)
    cx, cy = kx * tz, ky * tz
    fx, fy = float(cam.fx), float(cam.fy)
    J = np.zeros((p.shape[0], 2, 3))
    J[:, 0, 0] = fx / tz; J[:, 0, 2] = -fx * cx / tz ** 2
    J[:, 1, 1] = fy / tz; J[:, 1, 2] = -fy * cy / tz ** 2
    Wm = V[:3, :3].T
    T = J @ Wm
    cov = T @ Sg @ T.transpose(0, 2, 1)
    det_raw = cov[:, 0, 0] * cov[:, 1, 1] - cov[:, 0, 1] * cov[:, 1, 0]
    floored = det_raw < 1e-3
    det = np.maximum(det_raw, 1e-3)
    Q = np.empty((p.shape[0], 2, 2))
    Q[:, 0, 0] = cov[:, 1, 1] / det; Q[:, 1, 1] = cov[:, 0, 0] / det
    Q[:, 0, 1] = -cov[:, 0, 1] / det; Q[:, 1, 0] = -cov[:, 1, 0] / det
    h = ph @ F
    sx, sy = (float(cam.width) - 1) * 0.5, (float(cam.height) - 1) * 0.5
    xy = np.stack([(h[:, 0] / h[:, 3] + 1) * sx, (h[:, 1] / h[:, 3] + 1) * sy], 1)
    return dict(xy=xy, Q=Q, cov=cov, det=det, floored=floored, T=T, Sg=Sg, M=M, R=R, s=s, a=a, b=b, n1=n1, n2=n2, t=t,
                kx=kx, ky=ky, inx=inx, iny=iny, cx=cx, cy=cy, h=h, V=V, F=F, Wm=Wm, fx=fx, fy=fy, sx=sx, sy=sy,
                clamped=~(inx & iny))


def chain(st: dict, Q, S, absolute: bool = False):
    """(dL/dpoints, dL/dscales, dL/dquaternions) of the rows of `st` (stage1) from their moments S (m,5) and the conic Q
    (m,2,2) the compositing used.  absolute: S holds the absolute moments; every factor enters by its absolute value and
    every difference becomes a sum -- the error scale of the module doc."""
    A = np.abs if absolute else (lambda v: v)
    sg = 1.0 if absolute else -1.0           # the sign of a subtracted term
    S = np.asarray(S, np.float64)
    Q = A(np.asarray(Q, np.float64))
    S1, S2, S3, S4, S5 = S.T
    half = 0.5 if absolute else -0.5
    gQ = np.empty_like(Q)
    gQ[:, 0, 0] = half * S3; gQ[:, 0, 1] = half * S4; gQ[:, 1, 0] = half * S4; gQ[:, 1, 1] = half * S5
    qs = Q[:, 0, 1] + Q[:, 1, 0]
    gmx = half * (2 * Q[:, 0, 0] * S1 + qs * S2)
    gmy = half * (qs * S1 + 2 * Q[:, 1, 1] * S2)
    # 1
    cov, det = A(st["cov"]), st["det"]
    G = np.empty_like(Q)
    G[:, 0, 0] = gQ[:, 1, 1] / det; G[:, 1, 1] = gQ[:, 0, 0] / det
    G[:, 0, 1] = sg * gQ[:, 0, 1] / det
    G[:, 1, 0] = sg * gQ[:, 1, 0] / det
    g_det = sg * (gQ * Q).sum((1, 2)) / det
    g_det = np.where(st["floored"], 0.0, g_det)
    G[:, 0, 0] += g_det * cov[:, 1, 1]; G[:, 1, 1] += g_det * cov[:, 0, 0]
    G[:, 0, 1] += sg * g_det * cov[:, 1, 0]; G[:, 1, 0] += sg * g_det * cov[:, 0, 1]
    # 2
    T, Sg, Wm = A(st["T"]), A(st["Sg"]), A(st["Wm"])
    GT, GtT = G @ T, G.transpose(0, 2, 1) @ T
    dS = T.transpose(0, 2, 1) @ GT
    dT = GT @ Sg.transpose(0, 2, 1) + GtT @ Sg
    dJ = dT @ Wm.T
    fx, fy = st["fx"], st["fy"]
    t, tz = A(st["t"]), st["t"][:, 2]
    cx, cy, kx, ky = A(st["cx"]), A(st["cy"]), A(st["kx"]), A(st["ky"])
    z2, z3 = tz ** 2, tz ** 3
    g_cx, g_cy = sg * dJ[:, 0, 2] * fx / z2, sg * dJ[:, 1, 2] * fy / z2
    g_z = sg * dJ[:, 0, 0] * fx / z2 + sg * dJ[:, 1, 1] * fy / z2 + dJ[:, 0, 2] * 2 * fx * cx / z3 + dJ[:, 1, 2] * 2 * fy * cy / z3
    g_z = g_z + g_cx * kx + g_cy * ky
    g_rx, g_ry = np.where(st["inx"], g_cx * tz, 0.0), np.where(st["iny"], g_cy * tz, 0.0)
    g_t = np.stack([g_rx / tz, g_ry / tz, g_z + sg * (g_rx * t[:, 0] + g_ry * t[:, 1]) / z2], 1)
    # 3
    M, R, s = A(st["M"]), A(st["R"]), A(st["s"])
    dM = (dS + dS.transpose(0, 2, 1)) @ M
    gs = (dM * R).sum(1)
    dR = dM * s[:, None, :]
    # 4
    w, x, y, z = A(st["b"]).T
    d = dR
    m = sg      # d[..] - d[..] in the skew parts
    gb = np.stack([
        2 * (z * (d[:, 1, 0] + m * d[:, 0, 1]) + y * (d[:, 0, 2] + m * d[:, 2, 0]) + x * (d[:, 2, 1] + m * d[:, 1, 2])),
        2 * (y * (d[:, 0, 1] + d[:, 1, 0]) + z * (d[:, 0, 2] + d[:, 2, 0]) + w * (d[:, 2, 1] + m * d[:, 1, 2])
             + m * 2 * x * (d[:, 1, 1] + d[:, 2, 2])),
        2 * (x * (d[:, 0, 1] + d[:, 1, 0]) + z * (d[:, 1, 2] + d[:, 2, 1]) + w * (d[:, 0, 2] + m * d[:, 2, 0])
             + m * 2 * y * (d[:, 0, 0] + d[:, 2, 2])),
        2 * (x * (d[:, 0, 2] + d[:, 2, 0]) + y * (d[:, 1, 2] + d[:, 2, 1]) + w * (d[:, 1, 0] + m * d[:, 0, 1])
             + m * 2 * z * (d[:, 0, 0] + d[:, 1, 1]))], 1)
    b4, a4 = A(st["b"]), A(st["a"])
    ga = (gb + sg * b4 * (b4 * gb).sum(1, keepdims=True)) / st["n2"][:, None]
    gq = (ga + sg * a4 * (a4 * ga).sum(1, keepdims=True)) / st["n1"][:, None]
    # 5, 6
    h, F, V = A(st["h"]), A(st["F"]), A(st["V"])
    h3 = st["h"][:, 3]
    gn0, gn1 = gmx * st["sx"], gmy * st["sy"]
    gh = np.zeros((S.shape[0], 4))
    gh[:, 0] = gn0 / np.abs(h3) if absolute else gn0 / h3
    gh[:, 1] = gn1 / np.abs(h3) if absolute else gn1 / h3
    gh[:, 3] = sg * (gn0 * h[:, 0] + gn1 * h[:, 1]) / h3 ** 2
    gp = gh @ F[:3, :].T + g_t @ V[:3, :3].T
    return gp, gs, gq


def moments(pre, frame, grad_frame, width: int, height: int, tile: int, tiles=None, means=None, conics=None):
    """(S (m,5), Sabs (m,5)) in the depth-sorted order of `pre`: the moments of u over every composited (record, pixel) and
    the same sums with |d| for d and, for u, the bound of the terms u adds up that backward_restatement's scale_o uses:
    alpha (|C_fin|_1 + |c_k|_1) |g|_1 / (1 - alpha).  The walk, the float32 stop decision and dL/dalpha are backward_restatement's.
    means / conics: float64 (m,2) / (m,2,2) used for d and for alpha in place of pre's float32 values (the stop decision
    stays pre's float32)."""
    m = pre.points_xy.shape[0]
    mean32 = np.asarray(pre.points_xy, f32)
    inv32 = np.asarray(pre.inverse_covariance_2d, f32)
    mu = np.asarray(mean32 if means is None else means, np.float64)
    Qd = np.asarray(inv32 if conics is None else conics, np.float64)
    s = np.asarray(pre.sigmoid_opacity, f32).reshape(-1)
    op32 = (f32(1) / (f32(1) + np.exp(-s.astype(np.float64)).astype(f32))).astype(f32)
    cols = np.asarray(pre.colors, np.float64)
    cols_l1 = np.abs(cols).sum(1)
    S = np.zeros((m, 5))
    Sabs = np.zeros((m, 5))
    if tiles is None:
        tiles = [(x0, y0) for x0 in cpu_ref.tile_origins(width, tile) for y0 in cpu_ref.tile_origins(height, tile)]
    for x0, y0 in tiles:
        lst = cpu_ref.tile_list(pre, x0, y0, tile)
        if lst.size == 0:
            continue
        xs, ys = np.meshgrid(np.arange(x0, x0 + tile), np.arange(y0, y0 + tile), indexing="ij")
        px, py = xs.reshape(-1), ys.reshape(-1)
        g = np.asarray(grad_frame[px, py], np.float64)
        cf_g = (np.asarray(frame[px, py], np.float64) * g).sum(1)
        g_l1 = np.abs(g).sum(1)
        f_l1 = np.abs(np.asarray(frame[px, py], np.float64)).sum(1)
        P = px.size
        T32 = np.ones(P, f32)
        T = np.ones(P)
        Acc = np.zeros(P)
        live = np.ones(P, bool)
        pxf, pyf = px.astype(f32), py.astype(f32)
        for k in lst:
            a32 = _alpha32(mean32[k, 0], mean32[k, 1], inv32[k], op32[k], pxf, pyf)
            test32 = (T32 * (f32(1) - a32).astype(f32)).astype(f32)
            live &= test32 >= f32(1e-6)
            if not live.any():
                break
            d0, d1 = mu[k, 0] - px, mu[k, 1] - py
            if means is None and conics is None:
                a64 = a32.astype(np.float64)
            else:
                power = -0.5 * (Qd[k, 0, 0] * d0 * d0 + (Qd[k, 0, 1] + Qd[k, 1, 0]) * d0 * d1 + Qd[k, 1, 1] * d1 * d1)
                a64 = np.exp(power) * float(op32[k])
            alpha = np.where(live, a64, 0.0)
            ta = T * alpha
            cg = g @ cols[k]
            Acc = Acc + ta * cg
            da = np.where(live, T * cg - (cf_g - Acc) / np.where(live, 1.0 - alpha, 1.0), 0.0)
            u = da * alpha
            S[k] += np.stack([u * d0, u * d1, u * d0 * d0, u * d0 * d1, u * d1 * d1], 1).sum(0)
            # what u itself sums, in absolute value: backward_restatement's bound of dL/dalpha alpha (its scale_o)
            ua = np.where(live, alpha * (f_l1 + cols_l1[k]) * g_l1 / np.where(live, 1.0 - alpha, 1.0), 0.0)
            a0, a1 = np.abs(d0), np.abs(d1)
            Sabs[k] += np.stack([ua * a0, ua * a1, ua * a0 * a0, ua * a0 * a1, ua * a1 * a1], 1).sum(0)
            T = np.where(live, T * (1.0 - alpha), T)
            T32 = np.where(live, test32, T32)
    return S, Sabs


def listed_only(pre, width: int, height: int, tile: int, tiles=None):
    """(the rows of `pre` that are on at least one tile list, in their order; on, bool (m,): which rows those are).  The
    lists of the result are the lists of `pre` (cpu_ref.tile_list compares a row's own box with the tile), so every sum over
    composited (record, pixel) pairs is the same sum.  A row on no list has zero moments and a zero gradient whatever its
    stage 1 holds -- a NaN box is how a non-finite row gets there -- so no float64 stage 1 is formed for it at all."""
    on = np.zeros(np.asarray(pre.points_xy).shape[0], bool)
    if tiles is None:
        tiles = [(x0, y0) for x0 in cpu_ref.tile_origins(width, tile) for y0 in cpu_ref.tile_origins(height, tile)]
    for x0, y0 in tiles:
        on[cpu_ref.tile_list(pre, x0, y0, tile)] = True
    return type(pre)(*[np.asarray(a)[on] for a in pre]), on


def geometry_backward(pre, points, scales, quats, cam, frame, grad_frame, width: int, height: int, tile: int, tiles=None,
                      with_scale: bool = False):
    """(dL/dpoints (n,3), dL/dscales (n,3), dL/dquaternions (n,4)) in ORIGINAL row order; rows that are culled or on no
    composited pixel are zero.  pre: the depth-sorted float32 stage 1 (its means and conics enter the compositing, as in
    the reference); points, scales, quats: the float32 inputs.  with_scale: also (scale_p, scale_s, scale_q), each (n,)."""
    n = np.asarray(points).shape[0]
    pre, _ = listed_only(pre, width, height, tile, tiles)
    order = np.asarray(pre.order, np.int64)
    S, Sabs = moments(pre, frame, grad_frame, width, height, tile, tiles)
    st = stage1(np.asarray(points)[order], np.asarray(scales)[order], np.asarray(quats)[order], cam)
    Q = np.asarray(pre.inverse_covariance_2d, np.float64)
    out = []
    for arr, width_ in zip(chain(st, Q, S), (3, 3, 4)):
        full = np.zeros((n, width_))
        full[order] = arr
        out.append(full)
    if not with_scale:
        return tuple(out)
    for arr in chain(st, Q, Sabs, absolute=True):
        full = np.zeros(n)
        full[order] = np.abs(arr).sum(1)
        out.append(full)
    return tuple(out)


def per_gaussian_error(got, ref, scale) -> float:
    """max over Gaussians and components of (|got - ref| - SUBNORMAL) / scale: backward_restatement.per_gaussian_error's
    rule for one output of k components, scale (n,).  A Gaussian of zero scale must match to SUBNORMAL (its ratio is inf
    otherwise)."""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) - SUBNORMAL
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d <= 0, 0.0, d / np.asarray(scale, np.float64).reshape(-1, 1))
    return float(r.max()) if r.size else 0.0
