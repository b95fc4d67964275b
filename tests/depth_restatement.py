"""Float64 restatement of expected depth and coverage and of their gradients (the CPU pin of gsx_render_depth and
gsx_render_backward_depth).

Per pixel, over its tile's list in list order, with alpha_k the reference's alpha, T_1 = 1 and the walk stopping BEFORE
the first record with T_k (1 - alpha_k) < 1e-6:
    D = sum T_k alpha_k z_k          A = sum T_k alpha_k
z_k the view-space depth of record k (the reference's points_view[:, 2], PreprocessedScene.depths).  The reference
composites linearly in the colours, so (D, A) are the first two channels of its own frame over the colours (z, 1, 0),
and for L(frame, D, A) the compositing backward is backward_restatement's with FIVE channels: colour (r, g, b, z, 1),
final pixel (frame, D, A), pixel gradient (dL/dframe, gD, gA).  With E_k = sum_{j<=k} T_j alpha_j (c_j . g) over the five:
    dL/dalpha_k = T_k (c_k . g) - (F . g - E_k) / (1 - alpha_k)            u = dL/dalpha_k alpha_k
    dL/dc_k (rgb) = sum_p T_k alpha_k g_rgb            Sz_k = dL/dz_k = sum_p T_k alpha_k gD
u feeds the opacity sum and the five moments of geometry_backward_restatement, whose `chain` carries them to the points,
scales and quaternions; dL/dpoint gains Sz world2view[0:3, 2] (z = p . world2view[:3, 2] + world2view[3, 2]).  The tile
rectangle, culling, depth order and stop decision are piecewise constant.  Everything is float64 except the stop
decision, which follows the reference's float32 T and alpha (backward_restatement._alpha32).

with_scale=True also returns a per-Gaussian error scale for each output, built the way the two restatements this one
stands on build theirs -- the sum of the absolute values of the terms the gradient adds up: the chain run on absolute
moments with ua = alpha (|F|_1 + |c_k|_1) |g|_1 / (1 - alpha), the 1-norms over the five channels, in place of u
(backward_restatement's scale_o and geometry_backward_restatement.moments, with two more channels), plus
|world2view[0:3, 2]| sum_p T alpha |gD| for the points; ua's sum through the sigmoid chain for the opacity; sum_p T alpha
|g_rgb|_1 for the colours.
"""
from __future__ import annotations

import numpy as np

import geometry_backward_restatement as gbr
from backward_restatement import _alpha32
from oracle import cpu_ref

f32 = np.float32


def _op32(pre):
    s = np.asarray(pre.sigmoid_opacity, f32).reshape(-1)
    return (f32(1) / (f32(1) + np.exp(-s.astype(np.float64)).astype(f32))).astype(f32)


def _walk(pre, width, height, tile, tiles=None, means=None, conics=None, ops=None):
    """For every tile with a list: (px, py, records, info) with records a generator of (k, live, alpha) per list entry, in
    list order, until no pixel of the tile is live: alpha float64 (0 where the pixel has stopped), live the pixels that
    composite record k.  info["stopped"]: once records is exhausted, how many pixels of the tile the stop rule ended.
    The stop decision is the reference's float32 one on pre's own values.  means (m,2), conics (m,2,2), ops (m,): float64
    values alpha is formed from instead (all None: the float32 alpha itself)."""
    mean32 = np.asarray(pre.points_xy, f32)
    inv32 = np.asarray(pre.inverse_covariance_2d, f32)
    op32 = _op32(pre)
    exact = means is None and conics is None and ops is None
    mu = np.asarray(mean32 if means is None else means, np.float64)
    Qd = np.asarray(inv32 if conics is None else conics, np.float64)
    op = np.asarray(op32 if ops is None else ops, np.float64)
    if tiles is None:
        tiles = [(x0, y0) for x0 in cpu_ref.tile_origins(width, tile) for y0 in cpu_ref.tile_origins(height, tile)]
    for x0, y0 in tiles:
        lst = cpu_ref.tile_list(pre, x0, y0, tile)
        if lst.size == 0:
            continue
        xs, ys = np.meshgrid(np.arange(x0, x0 + tile), np.arange(y0, y0 + tile), indexing="ij")
        px, py = xs.reshape(-1), ys.reshape(-1)

        info = {"stopped": 0}

        def records(lst=lst, px=px, py=py, info=info):
            T32 = np.ones(px.size, f32)
            live = np.ones(px.size, bool)
            pxf, pyf = px.astype(f32), py.astype(f32)
            for k in lst:
                a32 = _alpha32(mean32[k, 0], mean32[k, 1], inv32[k], op32[k], pxf, pyf)
                test32 = (T32 * (f32(1) - a32).astype(f32)).astype(f32)
                live = live & (test32 >= f32(1e-6))
                info["stopped"] = int((~live).sum())
                if not live.any():
                    return
                if exact:
                    a64 = a32.astype(np.float64)
                else:
                    d0, d1 = mu[k, 0] - px, mu[k, 1] - py
                    power = -0.5 * (Qd[k, 0, 0] * d0 * d0 + (Qd[k, 0, 1] + Qd[k, 1, 0]) * d0 * d1 + Qd[k, 1, 1] * d1 * d1)
                    a64 = np.exp(power) * op[k]
                yield k, live, np.where(live, a64, 0.0)
                T32 = np.where(live, test32, T32)

        yield px, py, records(), info


def forward(pre, width: int, height: int, tile: int, z=None, colors=None, tiles=None, means=None, conics=None, ops=None):
    """(frame (W,H,3), D (W,H), A (W,H), info) in float64: the frame over `colors` (pre's) and the two maps over `z`
    (pre.depths), zeros where no tile is rendered; info: z_listed, the largest z on any tile list (0 without one),
    stopped, the pixels the stop rule ended, and longest, the longest tile list."""
    z = np.asarray(pre.depths if z is None else z, np.float64).reshape(-1)
    cols = np.asarray(pre.colors if colors is None else colors, np.float64)
    frame = np.zeros((width, height, 3))
    D = np.zeros((width, height))
    A = np.zeros((width, height))
    z_listed, stopped, longest = 0.0, 0, 0
    for px, py, records, info in _walk(pre, width, height, tile, tiles, means, conics, ops):
        T = np.ones(px.size)
        C = np.zeros((px.size, 3))
        d = np.zeros(px.size)
        a = np.zeros(px.size)
        walked = 0
        for k, live, alpha in records:
            walked += 1
            ta = T * alpha
            C += ta[:, None] * cols[k]
            d += ta * z[k]
            a += ta
            T = T * (1.0 - alpha)
            z_listed = max(z_listed, float(z[k]))
        frame[px, py] = C
        D[px, py] = d
        A[px, py] = a
        stopped += info["stopped"]
        longest = max(longest, walked)
    return frame, D, A, dict(z_listed=z_listed, stopped=stopped, longest=longest)


def sums(pre, frame, grad_frame, depth, grad_depth, width: int, height: int, tile: int, z=None, colors=None, tiles=None,
         means=None, conics=None, ops=None) -> dict:
    """The per-record sums of the module doc in the depth-sorted order of `pre`: gc (m,3), gu (m,), S (m,5), Sz (m,) and
    their absolute counterparts sc (m,), so (m,), Sabs (m,5), Szabs (m,).  frame, grad_frame: (W,H,3); depth, grad_depth:
    (W,H,2) holding (D, A) and (gD, gA)."""
    m = pre.points_xy.shape[0]
    z = np.asarray(pre.depths if z is None else z, np.float64).reshape(-1)
    cols3 = np.asarray(pre.colors if colors is None else colors, np.float64)
    cols = np.concatenate([cols3, z[:, None], np.ones((m, 1))], 1)
    cols_l1 = np.abs(cols).sum(1)
    mu = np.asarray(np.asarray(pre.points_xy, f32) if means is None else means, np.float64)
    out = dict(gc=np.zeros((m, 3)), gu=np.zeros(m), S=np.zeros((m, 5)), Sz=np.zeros(m), sc=np.zeros(m), so=np.zeros(m),
               Sabs=np.zeros((m, 5)), Szabs=np.zeros(m))
    for px, py, records, _ in _walk(pre, width, height, tile, tiles, means, conics, ops):
        g = np.concatenate([np.asarray(grad_frame[px, py], np.float64), np.asarray(grad_depth[px, py], np.float64)], 1)
        F = np.concatenate([np.asarray(frame[px, py], np.float64), np.asarray(depth[px, py], np.float64)], 1)
        fg = (F * g).sum(1)
        ga = np.abs(g)
        g_l1, f_l1 = ga.sum(1), np.abs(F).sum(1)
        T = np.ones(px.size)
        E = np.zeros(px.size)
        for k, live, alpha in records:
            ta = T * alpha
            cg = g @ cols[k]
            E = E + ta * cg
            one = np.where(live, 1.0 - alpha, 1.0)
            da = np.where(live, T * cg - (fg - E) / one, 0.0)
            u = da * alpha
            d0, d1 = mu[k, 0] - px, mu[k, 1] - py
            out["gc"][k] += (ta[:, None] * g[:, :3]).sum(0)
            out["gu"][k] += u.sum()
            out["S"][k] += np.stack([u * d0, u * d1, u * d0 * d0, u * d0 * d1, u * d1 * d1], 1).sum(0)
            out["Sz"][k] += (ta * g[:, 3]).sum()
            ua = np.where(live, alpha * (f_l1 + cols_l1[k]) * g_l1 / one, 0.0)
            a0, a1 = np.abs(d0), np.abs(d1)
            out["sc"][k] += (ta * ga[:, :3].sum(1)).sum()
            out["so"][k] += ua.sum()
            out["Sabs"][k] += np.stack([ua * a0, ua * a1, ua * a0 * a0, ua * a0 * a1, ua * a1 * a1], 1).sum(0)
            out["Szabs"][k] += (ta * ga[:, 3]).sum()
            T = T * (1.0 - alpha)
    return out


OUTPUTS = ("points", "scales", "quaternions", "colors", "opacity")


def finish(pre, sm: dict, st: dict, Q, n: int, sig=None, ops=None, with_scale: bool = False):
    """The five gradients in ORIGINAL row order from the sums `sm`, the float64 stage 1 `st` of the sorted rows
    (geometry_backward_restatement.stage1) and the conic Q (m,2,2) the compositing used: (gp (n,3), gs (n,3), gq (n,4),
    gc (n,3), go (n,1)), and with_scale the five scales, each (n,).  sig, ops: float64 sigmoid(logit) and
    sigmoid(sigmoid(logit)) of the sorted rows (None: pre's float32 values)."""
    order = np.asarray(pre.order, np.int64)
    s = np.asarray(pre.sigmoid_opacity, np.float64).reshape(-1) if sig is None else np.asarray(sig, np.float64)
    op = _op32(pre).astype(np.float64) if ops is None else np.asarray(ops, np.float64)
    col = st["V"][:3, 2]
    gp, gs, gq = gbr.chain(st, Q, sm["S"])
    gp = gp + sm["Sz"][:, None] * col[None, :]
    go = (sm["gu"] * (1.0 - op) * s * (1.0 - s))[:, None]

    def full(arr):
        a = np.zeros((n,) + arr.shape[1:])
        a[order] = arr
        return a

    out = [full(gp), full(gs), full(gq), full(sm["gc"]), full(go)]
    if not with_scale:
        return tuple(out)
    ap, as_, aq = gbr.chain(st, Q, sm["Sabs"], absolute=True)
    scale_p = np.abs(ap).sum(1) + sm["Szabs"] * np.abs(col).sum()
    out += [full(scale_p), full(np.abs(as_).sum(1)), full(np.abs(aq).sum(1)), full(sm["sc"]),
            full(sm["so"] * (1.0 - op) * s * (1.0 - s))]
    return tuple(out)


def depth_backward(pre, points, scales, quats, cam, frame, grad_frame, depth, grad_depth, width: int, height: int, tile: int,
                   tiles=None, with_scale: bool = False):
    """The five gradients of L(frame, D, A) (and with_scale their scales) in ORIGINAL row order for the reference's scene:
    pre the depth-sorted float32 stage 1 (its means, conics, opacities, colours and depths enter the compositing, as in
    the reference); points, scales, quats the float32 inputs; frame, depth the forward's images (the reference's float32
    ones for a fixture)."""
    n = np.asarray(points).shape[0]
    pre, _ = gbr.listed_only(pre, width, height, tile, tiles)
    order = np.asarray(pre.order, np.int64)
    sm = sums(pre, frame, grad_frame, depth, grad_depth, width, height, tile, tiles=tiles)
    st = gbr.stage1(np.asarray(points)[order], np.asarray(scales)[order], np.asarray(quats)[order], cam)
    return finish(pre, sm, st, np.asarray(pre.inverse_covariance_2d, np.float64), n, with_scale=with_scale)


def per_output_errors(got, ref, scales) -> dict:
    """name -> geometry_backward_restatement.per_gaussian_error of that output (five of each, in OUTPUTS' order)."""
    return {name: gbr.per_gaussian_error(np.asarray(g).reshape(np.asarray(r).shape[0], -1), np.asarray(r).reshape(np.asarray(r).shape[0], -1), s)
            for name, g, r, s in zip(OUTPUTS, got, ref, scales)}
