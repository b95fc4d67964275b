"""Float64 restatement of the camera gradients of the reference's frame (the CPU pin of gsx_render_backward_camera).

The reference's graph reaches the camera through two leaves (tools/capture_camera_grad_golden.py): world2view V, which
gives the view-space point t = ([p, 1] V)[:3] and W = V[:3,:3]^T of the EWA projection T = J W, and full_proj F, which
gives the homogeneous point h = [p, 1] F of the pixel mean.  geometry_backward_restatement.chain computes, per Gaussian,
the gradients of exactly these three -- g_t, dT and gh -- and contracts them with V and F into dL/dpoint.  Contracted with
the point instead (`terms`, steps 1, 2 and 5 of that chain restated up to there):

    dL/dV[k][c] = sum p_k g_t[c]  +  sum (J[0][c] dT[0][k] + J[1][c] dT[1][k])      k, c < 3   (W[c][k] = V[k][c])
    dL/dV[3][c] = sum g_t[c]                                                        c < 3
    dL/dF[k][c] = sum p_k gh[c],   dL/dF[3][c] = sum gh[c]                          c in {0, 1, 3}

summed over the Gaussians on a tile list.  Column 3 of V and column 2 of F reach nothing the frame computes: exact zeros.
J enters T as a factor; its own dependence on t is inside g_t.  The two matrices are independent leaves; everything else
of the camera (fx, fy, tan_fov) is constant.

absolute=True: the same sums over ABSOLUTE values (the absolute moments, every factor by its absolute value, every
difference a sum): the sum of |terms| per entry, the error scale of a float32 implementation.
"""
from __future__ import annotations

import numpy as np

import geometry_backward_restatement as gbr


def terms(st: dict, points, Q, S, absolute: bool = False):
    """(tV (m,4,4), tF (m,4,4)): every row's own contribution to dL/dV and dL/dF.  st: gbr.stage1 of the rows; points
    (m,3) the same rows' points; Q (m,2,2) the conic the compositing used; S (m,5) the moments."""
    A = np.abs if absolute else (lambda v: v)
    sg = 1.0 if absolute else -1.0
    half = 0.5 if absolute else -0.5
    S = np.asarray(S, np.float64)
    Q = A(np.asarray(Q, np.float64))
    p = A(np.asarray(points, np.float64))
    m = S.shape[0]
    S1, S2, S3, S4, S5 = S.T
    gQ = np.empty_like(Q)
    gQ[:, 0, 0] = half * S3; gQ[:, 0, 1] = half * S4; gQ[:, 1, 0] = half * S4; gQ[:, 1, 1] = half * S5
    qs = Q[:, 0, 1] + Q[:, 1, 0]
    gmx = half * (2 * Q[:, 0, 0] * S1 + qs * S2)
    gmy = half * (qs * S1 + 2 * Q[:, 1, 1] * S2)
    # 1: Q = adj(cov) / max(det, 1e-3)
    cov, det = A(st["cov"]), st["det"]
    G = np.empty_like(Q)
    G[:, 0, 0] = gQ[:, 1, 1] / det; G[:, 1, 1] = gQ[:, 0, 0] / det
    G[:, 0, 1] = sg * gQ[:, 0, 1] / det
    G[:, 1, 0] = sg * gQ[:, 1, 0] / det
    g_det = np.where(st["floored"], 0.0, sg * (gQ * Q).sum((1, 2)) / det)
    G[:, 0, 0] += g_det * cov[:, 1, 1]; G[:, 1, 1] += g_det * cov[:, 0, 0]
    G[:, 0, 1] += sg * g_det * cov[:, 1, 0]; G[:, 1, 0] += sg * g_det * cov[:, 0, 1]
    # 2: cov = T Sigma T^T, T = J W
    T, Sg, Wm = A(st["T"]), A(st["Sg"]), A(st["Wm"])
    dT = (G @ T) @ Sg.transpose(0, 2, 1) + (G.transpose(0, 2, 1) @ T) @ Sg
    dJ = dT @ Wm.T
    fx, fy = st["fx"], st["fy"]
    t, tz = A(st["t"]), st["t"][:, 2]
    cx, cy, kx, ky = A(st["cx"]), A(st["cy"]), A(st["kx"]), A(st["ky"])
    z2, z3 = tz ** 2, np.abs(tz ** 3) if absolute else tz ** 3
    atz = np.abs(tz) if absolute else tz
    g_cx, g_cy = sg * dJ[:, 0, 2] * fx / z2, sg * dJ[:, 1, 2] * fy / z2
    g_z = sg * dJ[:, 0, 0] * fx / z2 + sg * dJ[:, 1, 1] * fy / z2 + dJ[:, 0, 2] * 2 * fx * cx / z3 + dJ[:, 1, 2] * 2 * fy * cy / z3
    g_z = g_z + g_cx * kx + g_cy * ky
    g_rx, g_ry = np.where(st["inx"], g_cx * atz, 0.0), np.where(st["iny"], g_cy * atz, 0.0)
    g_t = np.stack([g_rx / atz, g_ry / atz, g_z + sg * (g_rx * t[:, 0] + g_ry * t[:, 1]) / z2], 1)
    J = np.zeros((m, 2, 3))
    J[:, 0, 0] = fx / atz; J[:, 0, 2] = sg * fx * cx / z2
    J[:, 1, 1] = fy / atz; J[:, 1, 2] = sg * fy * cy / z2
    J = A(J)
    # 5: pixel mean = ((h_xy / h_w) + 1)(dim - 1) / 2
    h = A(st["h"])
    h3 = np.abs(st["h"][:, 3]) if absolute else st["h"][:, 3]
    gn0, gn1 = gmx * st["sx"], gmy * st["sy"]
    gh = np.zeros((m, 4))
    gh[:, 0] = gn0 / h3
    gh[:, 1] = gn1 / h3
    gh[:, 3] = sg * (gn0 * h[:, 0] + gn1 * h[:, 1]) / h3 ** 2
    ph = np.concatenate([p, np.ones((m, 1))], 1)
    tV = np.zeros((m, 4, 4))
    tV[:, :, :3] = ph[:, :, None] * g_t[:, None, :]
    # dL/dW[c][k] = sum_i J[i][c] dT[i][k], and W[c][k] = V[k][c]
    tV[:, :3, :3] += (J.transpose(0, 2, 1) @ dT).transpose(0, 2, 1)
    tF = ph[:, :, None] * gh[:, None, :]
    return tV, tF


def camera_backward(pre, points, scales, quats, cam, frame, grad_frame, width: int, height: int, tile: int,
                    absolute: bool = False, moments=None, per_gaussian: bool = False):
    """(gV (4,4), gF (4,4)) float64: dL/dworld2view and dL/dfull_proj of the frame of `pre` (the depth-sorted float32 stage
    1: its means and conics enter the compositing, as in the reference).  absolute: the sum of |terms| per entry instead.
    moments: (S, Sabs) of gbr.moments when the caller has them already.  per_gaussian: (gV, gF, tV (m,4,4), tF (m,4,4))
    instead, the terms the two sums are over, one per listed Gaussian in depth-rank order."""
    pre, on = gbr.listed_only(pre, width, height, tile)         # a row on no list adds 32 exact zeros, whatever it holds
    order = np.asarray(pre.order, np.int64)
    S, Sabs = gbr.moments(pre, frame, grad_frame, width, height, tile) if moments is None else moments
    if len(S) != order.size:                                    # the caller's moments are of all the visible rows
        S, Sabs = S[on], Sabs[on]
    pts = np.asarray(points)[order]
    st = gbr.stage1(pts, np.asarray(scales)[order], np.asarray(quats)[order], cam)
    Q = np.asarray(pre.inverse_covariance_2d, np.float64)
    tV, tF = terms(st, pts, Q, Sabs if absolute else S, absolute)
    if per_gaussian:
        return tV.sum(0), tF.sum(0), tV, tF
    return tV.sum(0), tF.sum(0)


def centre_share(world2view, grad_centre):
    """dL/dworld2view (4,4) float64 of a loss that reads the pose only through the camera centre c = inverse(V)[3,:3],
    given dL/dc (3,): d inverse(V) = -inverse(V) dV inverse(V), so dL/dV = -inverse(V)^T G inverse(V)^T with G zero but
    G[3,:3] = dL/dc.  An SH scene's view direction is (point - c) / |point - c|: dL/dc = -sum of the rows of the
    view-direction share of dL/dpoints (sh_backward_restatement.backward's second output)."""
    inv = np.linalg.inv(np.asarray(world2view, np.float64))
    G = np.zeros((4, 4))
    G[3, :3] = np.asarray(grad_centre, np.float64)
    return -(inv.T @ G @ inv.T)


def scaled_error(got, ref, scale) -> float:
    """max over the 16 entries of |got - ref| / scale; an entry of zero scale (the structural zeros, an empty frame) must
    match exactly."""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).reshape(-1)
    s = np.asarray(scale, np.float64).reshape(-1)
    assert not d[s == 0].any(), (got, ref)
    return float((d[s > 0] / s[s > 0]).max()) if (s > 0).any() else 0.0
