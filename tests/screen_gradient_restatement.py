"""The screen-space densification statistic restated (the CPU pin of gsx_render_backward_screen, gsx_density_accumulate_screen
and gsx_density_plan_screen; include/gsx.h).

Float64, the gradient.  tests/geometry_backward_restatement.py sums five moments of u = dL/dpower per Gaussian over every
composited (record, pixel); the first two, S1 = sum u d0 and S2 = sum u d1 with d = mean - pixel, are all the pixel mean's
gradient needs:
    dL/dmean = -1/2 (Q + Q^T) (S1, S2)            grad_means2d = (dL/dmean_x sx, dL/dmean_y sy)
with Q the record's conic as stored, sx = (width - 1) / 2, sy = (height - 1) / 2: dL/d(NDC mean), the published trainer's
viewspace_points.grad[:, :2].  (The reference's own autograd reports dL/dmean, in pixels: tests/golden/screengrad_*.npz,
tools/capture_screen_grad_golden.py.)  The error scale of a Gaussian is the same construction on absolute values --
1/2 (|Q| + |Q|^T) (Sabs1, Sabs2) times sx, sy, the two components added -- as geometry_backward_restatement's is.

Float32, op for op, the two density calls, in the style of tests/density_restatement.py: every operation a numpy float32
operation rounded on its own.  The calls must equal these bit for bit.
"""
from __future__ import annotations

import numpy as np

import density_restatement as dr
import geometry_backward_restatement as gbr
from oracle import cpu_ref

F = np.float32


def half_extents(width: int, height: int):
    return (float(width) - 1.0) * 0.5, (float(height) - 1.0) * 0.5


def from_moments(Q, S, Sabs, width: int, height: int):
    """(gn (m,2), scale (m,)) in the order of the moments: dL/d(NDC mean) and its error scale."""
    Q = np.asarray(Q, np.float64)
    S, Sabs = np.asarray(S, np.float64), np.asarray(Sabs, np.float64)
    sxy = np.array(half_extents(width, height))
    sym, asym = Q + Q.transpose(0, 2, 1), np.abs(Q) + np.abs(Q).transpose(0, 2, 1)
    gm = -0.5 * np.einsum("kij,kj->ki", sym, S[:, :2])
    ga = 0.5 * np.einsum("kij,kj->ki", asym, Sabs[:, :2])
    return gm * sxy, (ga * sxy).sum(1)


def listed(pre, width: int, height: int, tile: int) -> np.ndarray:
    """bool (m,), depth order: the Gaussian is on at least one tile list of the frame (cpu_ref.tile_list)."""
    on = np.zeros(np.asarray(pre.points_xy).shape[0], bool)
    for x0 in cpu_ref.tile_origins(width, tile):
        for y0 in cpu_ref.tile_origins(height, tile):
            on[cpu_ref.tile_list(pre, x0, y0, tile)] = True
    return on


def screen_gradient(pre, n: int, frame, grad_frame, width: int, height: int, tile: int, tiles=None, moments=None):
    """(grad_means2d (n,2) float64, scale (n,)) in ORIGINAL row order; rows that are culled or on no composited pixel are
    zero.  moments: (S, Sabs) of geometry_backward_restatement.moments if the caller has them already."""
    pre, on = gbr.listed_only(pre, width, height, tile, tiles)      # the conic of a row on no list may be NaN
    S, Sabs = gbr.moments(pre, frame, grad_frame, width, height, tile, tiles) if moments is None else moments
    if len(S) != len(pre.order):                                    # the caller's moments are of all the visible rows
        S, Sabs = S[on], Sabs[on]
    gn, scale = from_moments(pre.inverse_covariance_2d, S, Sabs, width, height)
    order = np.asarray(pre.order, np.int64)
    full, full_scale = np.zeros((n, 2)), np.zeros(n)
    full[order], full_scale[order] = gn, scale
    return full, full_scale


def screen_radius(pre, n: int, on) -> np.ndarray:
    """(n,) float32 in ORIGINAL row order: the stage-1 radius of every listed Gaussian, +0 elsewhere."""
    out = np.zeros(n, np.float32)
    order = np.asarray(pre.order, np.int64)
    on = np.asarray(on, bool)
    out[order[on]] = np.asarray(pre.radius, np.float32).reshape(-1)[on]
    return out


def through_projection(st: dict, gn) -> np.ndarray:
    """dL/dpoint (m,3) that dL/d(NDC mean) gn (m,2) alone gives: gn through the float64 Jacobian of point -> NDC,
    NDC_i = h_i / h_3, h = [p, 1] @ full_proj (st: geometry_backward_restatement.stage1 of the rows)."""
    h, Fm = st["h"], st["F"]
    h3 = h[:, 3]
    gp = np.zeros((h.shape[0], 3))
    for i in range(2):
        jac = Fm[None, :3, i] / h3[:, None] - h[:, i, None] * Fm[None, :3, 3] / (h3 ** 2)[:, None]     # d NDC_i / d p_k
        gp += np.asarray(gn, np.float64)[:, i, None] * jac
    return gp


# ---- the two density calls, float32 op for op
def accumulate_screen(grad_means2d, radius, grad_sum, seen, radius_max):
    """(grad_sum', seen', radius_max'), new arrays.  Where radius > 0 (a NaN fails): norm = sqrt(g0 g0 + g1 g1) added, one
    counted, radius_max = r > radius_max ? r : radius_max; every other row untouched."""
    g = np.ascontiguousarray(grad_means2d, np.float32).reshape(-1, 2)
    r = np.ascontiguousarray(radius, np.float32).reshape(-1)
    out_sum, out_seen, out_max = np.array(grad_sum, np.float32), np.array(seen, np.uint32), np.array(radius_max, np.float32)
    with np.errstate(all="ignore"):
        live = r > F(0.0)
        norm = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
        assert norm.dtype == np.float32
        out_sum[live] = out_sum[live] + norm[live]
        out_seen[live] += np.uint32(1)
        out_max[live] = np.where(r[live] > out_max[live], r[live], out_max[live])
    return out_sum, out_seen, out_max


def plan_screen(grad_sum, seen, scales, opacity_logit, radius_max, prune_radius, r):
    """density_restatement.plan with PRUNE also where radius_max > prune_radius (radius_max None: the rule is off).
    (action uint8 (n), prefix int64 (n), counts = (n_out, n_pruned, n_cloned, n_split))."""
    action, prefix, counts = dr.plan(grad_sum, seen, scales, opacity_logit, r)
    if radius_max is None:
        return action, prefix, counts
    with np.errstate(all="ignore"):
        big = np.ascontiguousarray(radius_max, np.float32).reshape(-1) > F(prune_radius)
    action = action.copy()
    action[big] = dr.PRUNE
    count = dr.ROWS_OF[action]
    prefix = np.cumsum(count) - count
    return action, prefix.astype(np.int64), (int(count.sum()), int((action == dr.PRUNE).sum()), int((action == dr.CLONE).sum()),
                                             int((action == dr.SPLIT).sum()))
