"""float64 restatement of gsx_render_contribution: per Gaussian the largest blend weight, the sum of its blend weights and
the number of pixels that composited it, under both rule sets, with the decisions float32 could have taken otherwise.

TEST INFRASTRUCTURE ONLY.  Plain numpy.  Like depth_restatement.py it starts from the float32 stage-1 records -- REF_CPU: a
cpu_ref.Preprocessed (the reference's depth-sorted rows, tile lists by its own bounding-box rule); STD_3DGS: the
rule_set_restatement.Records of the C oracle's rows -- and walks them in float64.

For a (record k, pixel) pair the walk composites, w = T_k alpha_k, T_1 = 1, T_(k+1) = T_k (1 - alpha_k):
    REF_CPU   alpha = exp(power) op, power = t0 e0 + t1 e1 with e = mean - pixel, d = -e / 2, t = d @ Q (the reference's
              form), op = sigmoid(sigmoid(logit)); every listed record is evaluated; the pixel stops BEFORE the first record
              with T (1 - alpha) < 1e-6; the last row and column of tiles are not walked.
    STD_3DGS  rule_set_restatement's walk: skip where power > 0, alpha = min(0.99f, opacity exp(power)), skip where
              alpha < 1/255, stop BEFORE the first used record with T (1 - alpha) < 1e-4; every pixel of the frame.
    weight_max = max w        weight_sum = sum w        pixels = number of composited pairs         (per Gaussian)

Margins.  A decision is AMBIGUOUS where the values float32 could have given the tested quantity straddle the threshold.
STD_3DGS takes rule_set_restatement's bounds as they are (_pair, _stop_test, _decisions).  REF_CPU has one decision, the
stop, and the same first-order bound with u = 2^-24: the exponent is four products of three factors each added up, at most
eight roundings per term with the scaling by log2 e, so |power32 - power| <= 8 u S, S the sum of the four terms' absolute
values; v_exp_f32 is good to 2 ulp and its argument carries one more rounding of |power| <= S, the opacity product one:
    r_alpha = 10 u S + 5 u
    |test32 - test| <= test (e_T + 2u) + T alpha (r_alpha + u),      e_T' = e_T + 2u + alpha / (1 - alpha) (r_alpha + u)
(the kernel forms T - T alpha, the reference T (1 - alpha): both lie inside).  From a pixel's first ambiguous decision on,
which records it composites is float32's choice: every Gaussian the float64 walk composites in such a pixel, and every
Gaussian on the pixel's list from the ambiguous record on, is EXCLUDED from the weight_max / pixels comparison.  weight_sum
needs no exclusion in the GPU tests (it is pinned bit for bit to the backward entry).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import rule_set_restatement as rsr
from oracle import cpu_ref

f32 = np.float32
U = rsr.U
STOP_REF_CPU = float(f32(0.000001))
K_EXPONENT_REF = 10.0
K_ALPHA_REF = 5.0


class Contribution(NamedTuple):
    weight_max: np.ndarray        # (n,) float64, original row order; 0 for a row nothing composited
    weight_sum: np.ndarray        # (n,) float64
    pixels: np.ndarray            # (n,) int64
    listed: np.ndarray            # (n,) bool: on some walked tile's list (REF_CPU) / has a pixel rectangle (STD_3DGS)
    excluded: np.ndarray          # (n,) bool: touched by an ambiguous decision (module doc)
    ambiguous_pixels: int
    stopped_pixels: int


def _op32(pre):
    s = np.asarray(pre.sigmoid_opacity, f32).reshape(-1)
    return (f32(1) / (f32(1) + np.exp(-s.astype(np.float64)).astype(f32))).astype(f32)


def ref_cpu(pre, width: int, height: int, tile: int, n: int) -> Contribution:
    """GSX_SEM_REF_CPU.  pre: the depth-sorted float32 stage 1 (pre.order = original row of each sorted row)."""
    order = np.asarray(pre.order, np.int64)
    m = order.shape[0]
    mu = np.asarray(pre.points_xy, f32).astype(np.float64)
    Q = np.asarray(pre.inverse_covariance_2d, f32).astype(np.float64).reshape(-1, 2, 2)
    op = _op32(pre).astype(np.float64)
    wmax, wsum, pix = np.zeros(m), np.zeros(m), np.zeros(m, np.int64)
    listed, excluded = np.zeros(m, bool), np.zeros(m, bool)
    n_amb = n_stop = 0
    for x0 in cpu_ref.tile_origins(width, tile):
        for y0 in cpu_ref.tile_origins(height, tile):
            lst = cpu_ref.tile_list(pre, x0, y0, tile)
            if lst.size == 0:
                continue
            listed[lst] = True
            xs, ys = np.meshgrid(np.arange(x0, x0 + tile), np.arange(y0, y0 + tile), indexing="ij")
            px, py = xs.reshape(-1).astype(np.float64), ys.reshape(-1).astype(np.float64)
            T, e_T = np.ones(px.size), np.zeros(px.size)
            live, amb = np.ones(px.size, bool), np.zeros(px.size, bool)
            for pos, k in enumerate(lst):
                if not live.any() and not amb.any():
                    break
                e0, e1 = mu[k, 0] - px, mu[k, 1] - py
                d0, d1 = -0.5 * e0, -0.5 * e1
                terms = (d0 * Q[k, 0, 0] * e0, d1 * Q[k, 1, 0] * e0, d0 * Q[k, 0, 1] * e1, d1 * Q[k, 1, 1] * e1)
                power = (terms[0] + terms[1]) + (terms[2] + terms[3])
                S = sum(np.abs(t) for t in terms)
                with np.errstate(over="ignore", under="ignore", invalid="ignore"):
                    alpha = np.exp(power) * op[k]
                    r_alpha = K_EXPONENT_REF * U * S + K_ALPHA_REF * U
                    test = T * (1.0 - alpha)
                    err = np.abs(test) * (e_T + 2 * U) + T * alpha * (r_alpha + U)
                    e_next = e_T + 2 * U + alpha / np.abs(1.0 - alpha) * (r_alpha + U)
                ok = test >= STOP_REF_CPU                   # (NaN stops, as in the kernel)
                undecided = live & ~((test - err >= STOP_REF_CPU) | (test + err < STOP_REF_CPU))
                amb |= undecided
                acc = live & ok
                if amb.any():       # from a pixel's first ambiguous decision on, every record of its list is float32's choice
                    excluded[k] = True
                w = np.where(acc, T * alpha, 0.0)
                if acc.any():
                    wmax[k] = max(wmax[k], float(w.max()))
                    wsum[k] += float(w.sum())
                    pix[k] += int(acc.sum())
                n_stop += int((live & ~ok).sum())
                T = np.where(acc, test, T)
                e_T = np.where(acc, e_next, e_T)
                live = acc
            if amb.any():
                n_amb += int(amb.sum())
                # the Gaussians the float64 walk composited in an ambiguous pixel BEFORE its ambiguous record are the
                # same either way; the issue's rule leaves them out all the same: walk the list once more for them
                T = np.ones(px.size)
                live = np.ones(px.size, bool)
                for k in lst:
                    if not live.any():
                        break
                    e0, e1 = mu[k, 0] - px, mu[k, 1] - py
                    d0, d1 = -0.5 * e0, -0.5 * e1
                    power = (d0 * Q[k, 0, 0] * e0 + d1 * Q[k, 1, 0] * e0) + (d0 * Q[k, 0, 1] * e1 + d1 * Q[k, 1, 1] * e1)
                    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
                        alpha = np.exp(power) * op[k]
                        test = T * (1.0 - alpha)
                    live = live & (test >= STOP_REF_CPU)
                    if (live & amb).any():
                        excluded[k] = True
                    T = np.where(live, test, T)

    def full(a):
        out = np.zeros(n, a.dtype)
        out[order] = a
        return out

    return Contribution(full(wmax), full(wsum), full(pix), full(listed), full(excluded), n_amb, n_stop)


def std_3dgs(R: rsr.Records, width: int, height: int, n: int) -> Contribution:
    """GSX_SEM_STD_3DGS.  R: the records in walk order (R.index = original row), rectangles in pixels."""
    rules = rsr.STD_3DGS
    H, W = height, width
    T, e_T = np.ones((H, W)), np.zeros((H, W))
    live, amb = np.ones((H, W), bool), np.zeros((H, W), bool)
    PY, PX = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    wmax, wsum, pix = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    listed, excluded = np.zeros(n, bool), np.zeros(n, bool)
    accs = []
    for i in range(R.x.shape[0]):
        x0, x1, y0, y1 = R.rect[i]
        if x1 <= x0 or y1 <= y0:
            accs.append(None)
            continue
        row = int(R.index[i])
        listed[row] = True
        s = (slice(y0, y1), slice(x0, x1))
        lv = live[s]
        if amb[s].any():
            excluded[row] = True                        # on the list of an ambiguous pixel, behind its ambiguous record
        if not lv.any():
            accs.append(None)
            continue
        power, e_power, alpha, r_alpha = rsr._pair(rules, R, i, PX[s], PY[s])
        test, lo, hi, e_next = rsr._stop_test(T[s], e_T[s], alpha, r_alpha)
        skip_p, amb_p, skip_a, amb_a, stop, amb_s = rsr._decisions(rules, power, e_power, alpha, r_alpha, test, lo, hi)
        took_a = lv & ~skip_p
        used = took_a & ~skip_a
        undecided = (lv & amb_p) | (took_a & amb_a) | (used & amb_s)
        if undecided.any():
            excluded[row] = True
        amb[s] |= undecided
        acc = used & ~stop
        w = np.where(acc, T[s] * alpha, 0.0)
        if acc.any():
            wmax[row] = max(wmax[row], float(w.max()))
            wsum[row] += float(w.sum())
            pix[row] += int(acc.sum())
        T[s] = np.where(acc, test, T[s])
        e_T[s] = np.where(acc, e_next, e_T[s])
        live[s] = lv & ~(used & stop)
        accs.append((s, acc))
    # the issue's rule: a Gaussian the walk composited in an ambiguous pixel is left out, wherever in the list it stands
    for i, item in enumerate(accs):
        if item is not None and (item[1] & amb[item[0]]).any():
            excluded[int(R.index[i])] = True
    return Contribution(wmax, wsum, pix, listed, excluded, int(amb.sum()), int((~live).sum()))


def compare(got_max, got_pixels, ref: Contribution):
    """(worst |weight_max - restatement| over the rows not excluded, rows whose pixel count differs among them)."""
    keep = ~ref.excluded
    err = np.abs(np.asarray(got_max, np.float64).reshape(-1) - ref.weight_max)[keep]
    bad = np.nonzero(keep & (np.asarray(got_pixels).reshape(-1).astype(np.int64) != ref.pixels))[0]
    return (float(err.max()) if err.size else 0.0), bad
