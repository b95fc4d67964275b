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

with_scale=True also returns each Gaussian's error scale: float64 sums over the pixels where record k is composited,
    scale_c[k] = sum_p T_k alpha_k |g|_1
    scale_o[k] = (1 - sigmoid(s_k)) s_k (1 - s_k) sum_p alpha_k (|C_fin|_1 + |c_k|_1) |g|_1 / (1 - alpha_k)
bounds of the terms each gradient sums, so that a float32 implementation's error on Gaussian k is a small multiple of
the unit roundoff times its own scale, however small its gradient is next to the largest one (per_gaussian_error).
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
             n: int, tiles=None, with_scale: bool = False):
    """(dL/dcolors (n,3), dL/dopacity_logit (n,1)) in ORIGINAL row order.  pre: the depth-sorted stage-1 arrays
    (pre.order = original index of each sorted row); frame, grad_frame: (width, height, 3) indexed [x, y].
    tiles: the tile origins (x0, y0) where grad_frame is non-zero (None: every tile of the frame).
    with_scale: also the per-Gaussian error scales (scale_c (n,), scale_o (n,)), original row order (module doc)."""
    m = pre.points_xy.shape[0]
    means = np.asarray(pre.points_xy, f32)
    inv = np.asarray(pre.inverse_covariance_2d, f32)
    s = np.asarray(pre.sigmoid_opacity, f32).reshape(-1)
    op32 = (f32(1) / (f32(1) + np.exp(-s.astype(np.float64)).astype(f32))).astype(f32)
    op = op32.astype(np.float64)
    cols = np.asarray(pre.colors, np.float64)
    gc = np.zeros((m, 3))
    gu = np.zeros(m)           # sum over pixels of dL/dalpha * alpha
    sc_ = np.zeros(m)          # sum over pixels of T alpha |g|_1
    so_ = np.zeros(m)          # sum over pixels of alpha (|C_fin|_1 + |c_k|_1) |g|_1 / (1 - alpha)
    cols_l1 = np.abs(cols).sum(1)
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
            if with_scale:
                sc_[k] += (ta * g_l1).sum()
                so_[k] += (alpha * (f_l1 + cols_l1[k]) * g_l1 / np.where(live, 1.0 - alpha, 1.0)).sum()
            T = np.where(live, T * (1.0 - alpha), T)
            T32 = np.where(live, test32, T32)
    sd = s.astype(np.float64)
    glogit = gu * (1.0 - op) * sd * (1.0 - sd)
    out_c = np.zeros((n, 3))
    out_o = np.zeros((n, 1))
    order = np.asarray(pre.order, np.int64)
    out_c[order] = gc
    out_o[order, 0] = glogit
    if not with_scale:
        return out_c, out_o
    scale_c = np.zeros(n)
    scale_o = np.zeros(n)
    scale_c[order] = sc_
    scale_o[order] = so_ * (1.0 - op) * sd * (1.0 - sd)
    return out_c, out_o, scale_c, scale_o


# Below float32's smallest normal number its relative precision is gone: a gradient of 4e-45 carries one significant
# bit (tiny_48x48_n600 has such a Gaussian, and the reference's own autograd is 9 % of its scale off there).  Errors up
# to this absolute floor are not counted.
SUBNORMAL = float(np.finfo(np.float32).tiny)


def per_gaussian_error(gc, go, ref_c, ref_o, scale_c, scale_o):
    """(max over Gaussians and channels of (|gc - ref_c| - SUBNORMAL) / scale_c, the same of the opacity logits): the
    error of every Gaussian in units of its own error scale.  A Gaussian of zero scale (on no composited pixel, or
    where g = 0) must match to SUBNORMAL: its ratio is inf otherwise."""
    def ratio(a, b, scale):
        d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) - SUBNORMAL
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(d <= 0, 0.0, d / scale)
        return float(r.max()) if r.size else 0.0

    return (ratio(np.asarray(gc).reshape(-1, 3), np.asarray(ref_c).reshape(-1, 3), np.asarray(scale_c).reshape(-1, 1)),
            ratio(np.asarray(go).reshape(-1), np.asarray(ref_o).reshape(-1), np.asarray(scale_o).reshape(-1)))
