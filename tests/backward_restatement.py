"""Float64 restatement of the backward pass of the reference's frame (the CPU pin of gsx_render_backward).

The reference (splat/gaussian_scene.py:146-171, splat/utils.py:357-365) differentiates its image with respect to the
colours and the opacity logits only.  Per pixel, g = dL/dpixel, the list walked front to back, alpha_k = w_k sigmoid(s_k)
with s_k = sigmoid(logit_k), the walk stopping BEFORE record k when T_k (1 - alpha_k) < 1e-6, C_fin the frame's pixel and
A_k = sum_{j <= k} T_j alpha_j (c_j . g):
    dL/dc_k     += T_k alpha_k g
    dL/dalpha_k += T_k (c_k . g) - (C_fin . g - A_k) / (1 - alpha_k)
    dL/ds_k     += dL/dalpha_k w_k sigmoid(s_k) (1 - sigmoid(s_k))
    dL/dlogit_k  = dL/ds_k s_k (1 - s_k)
Here everything is float64 except the stop decision, which follows the reference's float32 T and alpha (so that a
pixel stops where the reference's does).  C_fin is the caller's frame (the reference's float32 image for a fixture).
"""
from __future__ import annotations

import numpy as np

from oracle import cpu_ref

f32 = np.float32


def _alpha32(x, y, q, op32, px, py):
    """The reference's float32 alpha at pixels (px, py) (float32 operations, exp rounded from float64)."""
    e0 = (f32(x) - px).astype(f32)
    e1 = (f32(y) - py).astype(f32)
    d0 = (f32(-0.5) * e0).astype(f32)
    d1 = (f32(-0.5) * e1).astype(f32)
    t0 = (d1.astype(np.float64) * np.float64(q[1, 0]) + (d0 * q[0, 0]).astype(f32).astype(np.float64)).astype(f32)
    t1 = (d1.astype(np.float64) * np.float64(q[1, 1]) + (d0 * q[0, 1]).astype(f32).astype(np.float64)).astype(f32)
    power = ((t0 * e0).astype(f32) + (t1 * e1).astype(f32)).astype(f32)
    w = np.exp(power.astype(np.float64)).astype(f32)
    return (w * op32).astype(f32)


def backward(pre: cpu_ref.Preprocessed, frame: np.ndarray, grad_frame: np.ndarray, width: int, height: int, tile: int,
             n: int, tiles=None):
    """(dL/dcolors (n,3), dL/dopacity_logit (n,1)) in ORIGINAL row order.  pre: the depth-sorted stage-1 arrays
    (pre.order = original index of each sorted row); frame, grad_frame: (width, height, 3) indexed [x, y].
    tiles: the tile origins (x0, y0) where grad_frame is non-zero (None: every tile of the frame)."""
    m = pre.points_xy.shape[0]
    means = np.asarray(pre.points_xy, f32)
    inv = np.asarray(pre.inverse_covariance_2d, f32)
    s = np.asarray(pre.sigmoid_opacity, f32).reshape(-1)
    op32 = (f32(1) / (f32(1) + np.exp(-s.astype(np.float64)).astype(f32))).astype(f32)
    op = op32.astype(np.float64)
    cols = np.asarray(pre.colors, np.float64)
    gc = np.zeros((m, 3))
    gu = np.zeros(m)           # sum over pixels of dL/dalpha * alpha
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
        P = px.size
        T32 = np.ones(P, f32)
        T = np.ones(P)
        A = np.zeros(P)
        live = np.ones(P, bool)
        pxf, pyf = px.astype(f32), py.astype(f32)
        for k in lst:
            a32 = _alpha32(means[k, 0], means[k, 1], inv[k], op32[k], pxf, pyf)
            test32 = (T32 * (f32(1) - a32).astype(f32)).astype(f32)
            live &= test32 >= f32(1e-6)
            if not live.any():
                break
            alpha = np.where(live, a32.astype(np.float64), 0.0)
            ta = T * alpha
            cg = g @ cols[k]
            A = A + ta * cg
            da = np.where(live, T * cg - (cf_g - A) / np.where(live, 1.0 - alpha, 1.0), 0.0)
            gc[k] += (ta[:, None] * g).sum(0)
            gu[k] += (da * alpha).sum()
            T = np.where(live, T * (1.0 - alpha), T)
            T32 = np.where(live, test32, T32)
    sd = s.astype(np.float64)
    glogit = gu * (1.0 - op) * sd * (1.0 - sd)
    out_c = np.zeros((n, 3))
    out_o = np.zeros((n, 1))
    order = np.asarray(pre.order, np.int64)
    out_c[order] = gc
    out_o[order, 0] = glogit
    return out_c, out_o
