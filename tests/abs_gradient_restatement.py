"""The absolute screen statistic restated in float64 (the CPU pin of gsx_render_backward_screen_abs; include/gsx.h).

tests/screen_gradient_restatement.py states dL/d(NDC mean) from the two moments S1 = sum u d0 and S2 = sum u d1: a SIGNED
sum over the pixels a Gaussian touches.  Here the same walk -- geometry_backward_restatement.moments': every tile's list
front to back, the float32 stop decision, alpha the float32 a32 widened to float64, dL/dalpha as
tests/backward_restatement.py has it -- keeps each (record, pixel) term on its own.  With u = dL/dalpha alpha,
d = mean - pixel and Q the record's conic as stored:
    cx = -1/2 u (2 q00 d0 + (q01 + q10) d1)        cy = -1/2 u ((q01 + q10) d0 + 2 q11 d1)
    abs = (sum |cx| |sx|, sum |cy| |sy|)             signed = (sum cx sx, sum cy sy)
sx = (width - 1) / 2, sy = (height - 1) / 2.  `signed` is screen_gradient_restatement.screen_gradient's value (the sums in
another order); `abs` is what AbsGS and gsplat's absgrad accumulate.  The reference's own autograd gives sum |cx|, sum |cy| in
pixel units once every (record, pixel) use of the mean is a leaf of its own: tests/golden/absgrad_*.npz,
tools/capture_abs_grad_golden.py.
"""
from __future__ import annotations

import numpy as np

import geometry_backward_restatement as gbr
from backward_restatement import _alpha32
from oracle import cpu_ref
from screen_gradient_restatement import half_extents

f32 = np.float32


def abs_gradient(pre, n: int, frame, grad_frame, width: int, height: int, tile: int, tiles=None, with_scale: bool = False):
    """(abs (n,2), signed (n,2)) float64 in NDC units and ORIGINAL row order; rows that are culled or on no composited pixel
    are zero.  with_scale: also the per-Gaussian error scale (n,) of screen_gradient_restatement.screen_gradient -- its
    construction (geometry_backward_restatement.moments' Sabs1, Sabs2 through from_moments) from this one walk."""
    pre, _ = gbr.listed_only(pre, width, height, tile, tiles)        # the conic of a row on no list may be NaN
    m = pre.points_xy.shape[0]
    mean32 = np.asarray(pre.points_xy, f32)
    inv32 = np.asarray(pre.inverse_covariance_2d, f32)
    mu = mean32.astype(np.float64)
    Q = inv32.astype(np.float64)
    s = np.asarray(pre.sigmoid_opacity, f32).reshape(-1)
    op32 = (f32(1) / (f32(1) + np.exp(-s.astype(np.float64)).astype(f32))).astype(f32)
    cols = np.asarray(pre.colors, np.float64)
    cols_l1 = np.abs(cols).sum(1)
    A, S, Sabs = np.zeros((m, 2)), np.zeros((m, 2)), np.zeros((m, 2))
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
        T32, T, Acc, live = np.ones(P, f32), np.ones(P), np.zeros(P), np.ones(P, bool)
        pxf, pyf = px.astype(f32), py.astype(f32)
        for k in lst:
            a32 = _alpha32(mean32[k, 0], mean32[k, 1], inv32[k], op32[k], pxf, pyf)
            test32 = (T32 * (f32(1) - a32).astype(f32)).astype(f32)
            live &= test32 >= f32(1e-6)
            if not live.any():
                break
            d0, d1 = mu[k, 0] - px, mu[k, 1] - py
            alpha = np.where(live, a32.astype(np.float64), 0.0)
            cg = g @ cols[k]
            Acc = Acc + T * alpha * cg
            da = np.where(live, T * cg - (cf_g - Acc) / np.where(live, 1.0 - alpha, 1.0), 0.0)
            u = da * alpha
            off = Q[k, 0, 1] + Q[k, 1, 0]
            cx = -0.5 * u * (2.0 * Q[k, 0, 0] * d0 + off * d1)
            cy = -0.5 * u * (off * d0 + 2.0 * Q[k, 1, 1] * d1)
            A[k] += (np.abs(cx).sum(), np.abs(cy).sum())
            S[k] += (cx.sum(), cy.sum())
            if with_scale:
                ua = np.where(live, alpha * (f_l1 + cols_l1[k]) * g_l1 / np.where(live, 1.0 - alpha, 1.0), 0.0)
                Sabs[k] += ((ua * np.abs(d0)).sum(), (ua * np.abs(d1)).sum())
            T = np.where(live, T * (1.0 - alpha), T)
            T32 = np.where(live, test32, T32)
    sxy = np.array(half_extents(width, height))
    order = np.asarray(pre.order, np.int64)
    full_abs, full_signed = np.zeros((n, 2)), np.zeros((n, 2))
    full_abs[order], full_signed[order] = A * np.abs(sxy), S * sxy
    if not with_scale:
        return full_abs, full_signed
    asym = np.abs(Q) + np.abs(Q).transpose(0, 2, 1)
    full_scale = np.zeros(n)
    full_scale[order] = (0.5 * np.einsum("kij,kj->ki", asym, Sabs) * sxy).sum(1)
    return full_abs, full_signed, full_scale
