"""float64 restatement of the two discontinuous rule sets (GSX_SEM_STD_3DGS, GSX_SEM_REF_CUDA) that knows, for every
decision it takes, how far the tested quantity is from its threshold and what float32 could have made of it.

TEST INFRASTRUCTURE ONLY.  Plain numpy.  Input: the float32 stage-1 arrays the C oracle returns (std_3dgs: the (n, 8) rows
of c_oracle.render_std3dgs, tile lists by depth and then index; ref_cuda: a cpu_ref.Preprocessed, all rows in order).  The
walk itself is one function, parameterised by a `Rules` tuple:

    per (pixel, record)   d = mean - pixel;  power = -1/2 (A dx^2 + C dy^2) - B dx dy
      [std_3dgs]          power > 0                       -> skip                      (decision "power")
                          alpha = min(0.99f, opacity exp(power))
      [std_3dgs]          alpha < 1/255                   -> skip                      (decision "alpha")
                          T (1 - alpha) < stop threshold  -> the pixel is done         (decision "stop")
                          C += colour alpha T;  T <- T (1 - alpha);  at the end  out = C + T background
    ref_cuda: the mean is truncated to int and only pixels inside the inclusive bounding box see a record; both tests
    are exact in float32 (integers against float32 values) and are not decisions.

Margins.  u = 2^-24 is the relative rounding of one float32 operation.  Everything below is a first-order bound with the
constants rounded up (7 -> 8, 1 -> 2), which absorbs the second-order terms.

  exponent (gsx_blend.hip, blend_std16_kernel / blend_rules_kernel; packing: gsx_project.hip pack_record).  The record
    holds Q'' = fl(q * k), k = fl(-1/2 log2 e): two roundings per coefficient.  e_x = x - px, e_y = y - py: one rounding
    each (the float64 walk has them exact).  The kernel evaluates  pw = fma(e_y, fma(e_y, Q11, e_x Qs), (e_x e_x) Q00):
        (e_x e_x) Q00 : e_x twice (2u) + square (u) + Q00 (2u) + product (u) + the last fma's rounding (u)       = 7u
        e_x e_y Qs    : e_x (u) + Qs (2u; B + B is exact) + product (u) + inner fma (u) + e_y (u) + last fma (u) = 7u
        e_y e_y Q11   : e_y twice (2u) + Q11 (2u) + inner fma (u) + last fma (u)                                 = 6u
    so  |pw32 - pw| <= 8 u S,  S = |A dx^2|/2 + |C dy^2|/2 + |B dx dy|  (in natural-log units after the factor ln 2 that
    exp2 brings back).  The C port (-0.5f (A dx dx + C dy dy) - B dx dy, at most 6 roundings per term) lies inside the
    same bound.  ref_cuda folds log2f(opacity) into the exponent (one more fma, log2f good to 2 ulp): S gains
    |ln opacity| and the bound keeps its form.  A zero S means dx = dy = 0: the exponent is exactly 0 on both sides.
  alpha.  v_exp_f32 and libm's expf are good to 1 ulp (relative 2u); std_3dgs multiplies by the opacity (u):
        relative error of alpha  r_alpha = 8 u S + 3u,
    and exactly 0 where even alpha (1 - r_alpha) clamps: alpha is then the constant 0.99f on every path.
  T.  The kernel computes ta = fl(T alpha), T' = fl(T - ta) (std_composite; blend_rules_kernel:1431), the port
    fl(T fl(1 - alpha)); a compiler may contract T - T alpha into one fma.  With e_T the relative error of T so far:
        |test32 - test| <= test (e_T + 2u) + T alpha (r_alpha + u)
        e_T' = e_T + 2u + alpha / (1 - alpha) (r_alpha + u)                 (alpha <= 0.99: the factor is at most 99)
    Where T is exact so far (e_T = 0) and alpha is the clamp constant, the inputs of the test ARE float32 numbers and the
    three float32 evaluations (kernel order, port order, contracted) are simply carried out: the test's possible values
    are those three and the float64 one, and e_T' is their largest distance from it.  This is what decides the knife
    edge of two clamped alphas in a row: T = 1 - 0.99f exactly, and every order gives T (1 - 0.99f) = 9.99998e-5 < 1e-4.

A decision is DECIDED when every value float32 could have given the tested quantity lies on the float64 value's side of
the threshold, AMBIGUOUS otherwise.  A pixel is decided when every decision it took while live is decided.  An ambiguous
pixel is walked again record by record with its ambiguous decisions taken both ways -- at most MAX_FLIPS along one walk,
ambiguous decisions met later in an alternative branch again within the same limit -- and gets the list of the resulting
colours; a pixel that would need more is LEFT OUT.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

f32 = np.float32
U = 2.0 ** -24
K_EXPONENT = 8.0          # |pw32 - pw| <= K_EXPONENT u S
K_EXP_MUL = 3.0           # exp (2u) and the opacity product (u)
CLAMP = float(f32(0.99))
MAX_FLIPS = 3
NEAR = 1e-3               # "near the threshold" for the coverage counts (relative)


class Rules(NamedTuple):
    name: str
    skip_threshold: Optional[float]      # alpha below this float32 constant is skipped; None: no such rule
    stop_threshold: float                # the pixel is done when T (1 - alpha) is below this float32 constant
    power_skip: bool                     # skip where the exponent is > 0
    log_opacity_in_exponent: bool        # the kernel adds log2(opacity) to the exponent instead of multiplying


STD_3DGS = Rules("std_3dgs", float(f32(1.0) / f32(255.0)), float(f32(0.0001)), True, False)
REF_CUDA = Rules("ref_cuda", None, float(f32(0.001)), False, True)


class Records(NamedTuple):
    """Records in walk order; `rect` = x0, x1, y0, y1 (pixels, exclusive upper ends): the pixels that see the record."""
    x: np.ndarray
    y: np.ndarray
    A: np.ndarray
    B: np.ndarray
    C: np.ndarray
    opacity: np.ndarray
    colors: np.ndarray
    rect: np.ndarray
    index: np.ndarray     # row of the input arrays


class Walk(NamedTuple):
    colour: np.ndarray            # (H, W, 3) float64
    n_ambiguous: np.ndarray       # (H, W) ambiguous decisions on the float64 path
    alternatives: Dict[Tuple[int, int], np.ndarray]     # (y, x) -> (k, 3) colours, the float64 path's first
    left_out: List[Tuple[int, int]]
    stopped: np.ndarray           # (H, W) bool
    composited: np.ndarray        # (H, W) records accumulated
    stop_position: np.ndarray     # (H, W) position in the pixel's list of the record that stopped it, -1 if none
    list_length: np.ndarray       # (H, W) length of the pixel's list
    near_skip_below: int          # decided alpha-skip decisions within NEAR (relative) of the threshold, skipped
    near_skip_above: int          # ... and used
    single_pixel_blocks: int      # (record, 8x8 block) combinations in which the record is used at exactly one pixel
    max_ambiguous: int

    @property
    def ambiguous(self):
        return self.n_ambiguous > 0


def _tile_index(v, nt):
    nan = np.isnan(v)
    c = np.trunc(np.clip(np.where(nan, f32(0.0), v), f32(-1073741824.0), f32(1073741824.0))).astype(np.int64)
    return np.where(nan, -1, np.clip(c, 0, nt))


def records_std3dgs(stage1_rows, colors, width, height, tile) -> Records:
    """From the (n, 8) float32 rows x, y, A, B, C, radius, depth, opacity (NaN where culled): the tile rectangle of the
    published rule, lists by depth and then index (oracle/std3dgs_ref.py)."""
    g = np.asarray(stage1_rows, f32).reshape(-1, 8)
    col = np.asarray(colors, f32).reshape(-1, 3)
    x, y, r = g[:, 0], g[:, 1], g[:, 5]
    T = f32(tile)
    ntx, nty = (width + tile - 1) // tile, (height + tile - 1) // tile
    with np.errstate(invalid="ignore"):
        lx, hx = _tile_index((x - r) / T, ntx), _tile_index(((x + r + T) - f32(1.0)) / T, ntx)
        ly, hy = _tile_index((y - r) / T, nty), _tile_index(((y + r + T) - f32(1.0)) / T, nty)
    keep = ~np.isnan(x) & (lx >= 0) & (hx >= 0) & (ly >= 0) & (hy >= 0)
    keep &= np.where(keep, (hx - lx) * (hy - ly), 0) > 0
    idx = np.nonzero(keep)[0]
    idx = idx[np.argsort(g[idx, 6], kind="stable")]
    rect = np.stack([lx[idx] * tile, np.minimum(hx[idx] * tile, width), ly[idx] * tile, np.minimum(hy[idx] * tile, height)],
                    axis=1).astype(np.int64)
    d = g[idx].astype(np.float64)
    return Records(d[:, 0], d[:, 1], d[:, 2], d[:, 3], d[:, 4], d[:, 7], col[idx].astype(np.float64), rect, idx)


def records_ref_cuda(pre, width, height) -> Records:
    """From the reference's preprocessed arrays, all rows in order: truncated means, a, b, c = inv[0,0], inv[0,1],
    inv[1,1], the inclusive bounding box as a pixel rectangle."""
    mean = np.asarray(pre.points, f32).reshape(-1, 2)
    inv = np.asarray(pre.inverse_covariance_2d, f32).reshape(-1, 4).astype(np.float64)
    n = mean.shape[0]
    flat = lambda a: np.asarray(a, f32).reshape(-1).astype(np.float64)  # noqa: E731
    x0 = np.clip(np.ceil(flat(pre.min_x)), 0, width)
    x1 = np.clip(np.floor(flat(pre.max_x)) + 1, 0, width)
    y0 = np.clip(np.ceil(flat(pre.min_y)), 0, height)
    y1 = np.clip(np.floor(flat(pre.max_y)) + 1, 0, height)
    rect = np.stack([x0, np.maximum(x1, x0), y0, np.maximum(y1, y0)], axis=1).astype(np.int64)
    t = np.trunc(mean.astype(np.float64))
    return Records(t[:, 0], t[:, 1], inv[:, 0], inv[:, 1], inv[:, 3], flat(pre.sigmoid_opacity),
                   np.asarray(pre.colors, f32).reshape(-1, 3).astype(np.float64), rect, np.arange(n))


def _pair(rules: Rules, R: Records, i: int, px, py):
    """power, its absolute bound, alpha and its relative bound for record i at the pixels (px, py)."""
    dx, dy = R.x[i] - px, R.y[i] - py
    t1, t2, t3 = 0.5 * R.A[i] * dx * dx, 0.5 * R.C[i] * dy * dy, R.B[i] * dx * dy
    power = -(t1 + t2) - t3
    S = np.abs(t1) + np.abs(t2) + np.abs(t3)
    if rules.log_opacity_in_exponent:
        S = S + abs(np.log(R.opacity[i])) if R.opacity[i] > 0 else S
    e_power = K_EXPONENT * U * S
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        raw = R.opacity[i] * np.exp(power)
    r_alpha = e_power + K_EXP_MUL * U
    r_alpha = np.where(raw * (1.0 - r_alpha) >= CLAMP, 0.0, r_alpha)
    return power, e_power, np.minimum(CLAMP, raw), r_alpha


def _stop_test(T, e_T, alpha, r_alpha):
    """test = T (1 - alpha), the interval float32 could have put it in, and the relative error of T if it is taken."""
    test = T * (1.0 - alpha)
    err = test * (e_T + 2 * U) + T * alpha * (r_alpha + U)
    lo, hi = test - err, test + err
    e_next = e_T + 2 * U + alpha / (1.0 - alpha) * (r_alpha + U)
    exact = (e_T == 0.0) & (r_alpha == 0.0)
    if np.any(exact):
        T32, a32 = np.asarray(T, np.float64).astype(f32), np.asarray(alpha, np.float64).astype(f32)
        kernel = (T32 - (T32 * a32).astype(f32)).astype(np.float64)
        port = (T32 * (f32(1.0) - a32).astype(f32)).astype(np.float64)
        fused = np.asarray(test, np.float64).astype(f32).astype(np.float64)
        lo_x = np.minimum(np.minimum(test, kernel), np.minimum(port, fused))
        hi_x = np.maximum(np.maximum(test, kernel), np.maximum(port, fused))
        lo, hi = np.where(exact, lo_x, lo), np.where(exact, hi_x, hi)
        e_next = np.where(exact, np.maximum(hi_x - test, test - lo_x) / test, e_next)
    return test, lo, hi, e_next


def _decisions(rules: Rules, power, e_power, alpha, r_alpha, test, lo, hi):
    """(value, ambiguous) of the three decisions; a rule the set does not have is (False, False)."""
    no = np.zeros(np.shape(power), bool)
    if rules.power_skip:
        skip_p, amb_p = power > 0.0, (np.abs(power) <= e_power) & (e_power > 0.0)
    else:
        skip_p, amb_p = no, no
    if rules.skip_threshold is not None:
        thr = rules.skip_threshold
        skip_a, amb_a = alpha < thr, np.abs(alpha - thr) <= alpha * r_alpha
    else:
        skip_a, amb_a = no, no
    stop = test < rules.stop_threshold
    amb_s = ~((hi < rules.stop_threshold) | (lo >= rules.stop_threshold))
    return skip_p, amb_p, skip_a, amb_a, stop, amb_s


def walk(rules: Rules, R: Records, width: int, height: int, background=(0.0, 0.0, 0.0)) -> Walk:
    bg = np.asarray(background, np.float64)
    H, W = height, width
    colour = np.zeros((H, W, 3))
    T, e_T = np.ones((H, W)), np.zeros((H, W))
    live = np.ones((H, W), bool)
    n_amb = np.zeros((H, W), np.int64)
    composited = np.zeros((H, W), np.int64)
    position = np.zeros((H, W), np.int64)
    stop_position = np.full((H, W), -1, np.int64)
    near_below = near_above = single = 0
    PY, PX = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for i in range(R.x.shape[0]):
        x0, x1, y0, y1 = R.rect[i]
        if x1 <= x0 or y1 <= y0:
            continue
        s = (slice(y0, y1), slice(x0, x1))
        lv = live[s]
        if lv.any():
            power, e_power, alpha, r_alpha = _pair(rules, R, i, PX[s], PY[s])
            test, lo, hi, e_next = _stop_test(T[s], e_T[s], alpha, r_alpha)
            skip_p, amb_p, skip_a, amb_a, stop, amb_s = _decisions(rules, power, e_power, alpha, r_alpha, test, lo, hi)
            took_a = lv & ~skip_p                       # decisions taken on the float64 path
            used = took_a & ~skip_a
            n_amb[s] += (lv & amb_p).astype(np.int64) + (took_a & amb_a) + (used & amb_s)
            if rules.skip_threshold is not None:
                near = took_a & ~amb_a & (np.abs(alpha - rules.skip_threshold) <= NEAR * rules.skip_threshold)
                near_below += int((near & skip_a).sum())
                near_above += int((near & ~skip_a).sum())
            if used.any():
                ys, xs = np.nonzero(used)
                _, counts = np.unique(((ys + y0) // 8) * ((W + 7) // 8) + (xs + x0) // 8, return_counts=True)
                single += int((counts == 1).sum())
            stops, acc = used & stop, used & ~stop
            w = np.where(acc, alpha * T[s], 0.0)
            colour[s] += w[..., None] * R.colors[i]
            T[s] = np.where(acc, test, T[s])
            e_T[s] = np.where(acc, e_next, e_T[s])
            composited[s] += acc
            stop_position[s] = np.where(stops, position[s], stop_position[s])
            live[s] = lv & ~stops
        position[s] += 1
    colour += T[..., None] * bg
    alternatives, left_out = {}, []
    for y, x in zip(*np.nonzero(n_amb > 0)):
        alts = pixel_alternatives(rules, R, int(x), int(y), bg)
        if alts is None:
            left_out.append((int(y), int(x)))
        else:
            alternatives[(int(y), int(x))] = alts
    return Walk(colour, n_amb, alternatives, left_out, ~live, composited, stop_position, position, near_below, near_above,
                single, int(n_amb.max()) if n_amb.size else 0)


class _LeftOut(Exception):
    pass


def pixel_alternatives(rules: Rules, R: Records, px: int, py: int, bg) -> Optional[np.ndarray]:
    """Every colour pixel (px, py) can take when its ambiguous decisions fall either way (the float64 path's first);
    None when one walk meets more than MAX_FLIPS of them."""
    lst = np.nonzero((R.rect[:, 0] <= px) & (px < R.rect[:, 1]) & (R.rect[:, 2] <= py) & (py < R.rect[:, 3]))[0]
    out: List[np.ndarray] = []
    fx, fy = np.float64(px), np.float64(py)

    def branch(value, ambiguous, flips):
        if not ambiguous:
            return [(bool(value), flips)]
        if flips + 1 > MAX_FLIPS:
            raise _LeftOut()
        return [(bool(value), flips + 1), (not bool(value), flips + 1)]

    def go(k, T, e_T, c, flips):
        while k < len(lst):
            i = lst[k]
            k += 1
            power, e_power, alpha, r_alpha = _pair(rules, R, i, fx, fy)
            test, lo, hi, e_next = _stop_test(T, e_T, alpha, r_alpha)
            skip_p, amb_p, skip_a, amb_a, stop, amb_s = _decisions(rules, power, e_power, alpha, r_alpha, test, lo, hi)
            outcomes: Dict[str, int] = {}
            for sp, f1 in branch(skip_p, amb_p, flips):
                if sp:
                    outcomes["skip"] = min(outcomes.get("skip", f1), f1)
                    continue
                for sa, f2 in branch(skip_a, amb_a, f1):
                    if sa:
                        outcomes["skip"] = min(outcomes.get("skip", f2), f2)
                        continue
                    for ss, f3 in branch(stop, amb_s, f2):
                        kind = "stop" if ss else "acc"
                        outcomes[kind] = min(outcomes.get(kind, f3), f3)
            # the float64 path's own outcome first, so that alternative 0 is the walk's colour
            own = "skip" if (skip_p or skip_a) else ("stop" if stop else "acc")
            order = [own] + [o for o in ("skip", "acc", "stop") if o != own and o in outcomes]
            if len(order) == 1:
                flips = outcomes[own]
                if own == "stop":
                    break
                if own == "acc":
                    c, T, e_T = c + float(alpha * T) * R.colors[i], float(test), float(e_next)
                continue
            for o in order:
                if o == "stop":
                    out.append(c + T * bg)
                elif o == "acc":
                    go(k, float(test), float(e_next), c + float(alpha * T) * R.colors[i], outcomes[o])
                else:
                    go(k, T, e_T, c, outcomes[o])
            return
        out.append(c + T * bg)

    try:
        go(0, 1.0, 0.0, np.zeros(3), 0)
    except _LeftOut:
        return None
    return np.stack(out)


class Decision(NamedTuple):
    record: int           # row of the input arrays
    kind: str             # "power", "alpha" or "stop"
    taken: bool           # skipped / stopped on the float64 path
    distance: float       # of the tested quantity from its threshold
    bound: float          # what float32 could have moved it by
    ambiguous: bool


def pixel_decisions(rules: Rules, R: Records, px: int, py: int) -> List[Decision]:
    """Every decision pixel (px, py) takes on the float64 path while it is live, with its margin."""
    lst = np.nonzero((R.rect[:, 0] <= px) & (px < R.rect[:, 1]) & (R.rect[:, 2] <= py) & (py < R.rect[:, 3]))[0]
    fx, fy = np.float64(px), np.float64(py)
    T, e_T, out = 1.0, 0.0, []
    for i in lst:
        power, e_power, alpha, r_alpha = _pair(rules, R, i, fx, fy)
        test, lo, hi, e_next = _stop_test(T, e_T, alpha, r_alpha)
        skip_p, amb_p, skip_a, amb_a, stop, amb_s = _decisions(rules, power, e_power, alpha, r_alpha, test, lo, hi)
        if rules.power_skip:
            out.append(Decision(int(R.index[i]), "power", bool(skip_p), float(abs(power)), float(e_power), bool(amb_p)))
            if skip_p:
                continue
        if rules.skip_threshold is not None:
            out.append(Decision(int(R.index[i]), "alpha", bool(skip_a), float(abs(alpha - rules.skip_threshold)),
                                float(alpha * r_alpha), bool(amb_a)))
            if skip_a:
                continue
        out.append(Decision(int(R.index[i]), "stop", bool(stop), float(abs(test - rules.stop_threshold)),
                            float(max(hi - test, test - lo)), bool(amb_s)))
        if stop:
            break
        T, e_T = float(test), float(e_next)
    return out


class Verdict(NamedTuple):
    worst_decided: float          # largest error of a decided pixel
    worst_ambiguous: float        # largest distance of an ambiguous pixel from its nearest alternative
    unexplained: List[Tuple[int, int, float]]      # (y, x, error) beyond the tolerance
    n_ambiguous: int
    n_left_out: int


def classify(wk: Walk, image_hw3, tol: float) -> Verdict:
    """Every decided pixel within `tol` of the float64 colour, every ambiguous one within `tol` of an alternative."""
    img = np.asarray(image_hw3, np.float64)
    err = np.abs(img - wk.colour).max(axis=-1)
    amb = wk.ambiguous
    worst_decided = float(err[~amb].max()) if (~amb).any() else 0.0
    bad = [(int(y), int(x), float(err[y, x])) for y, x in zip(*np.nonzero(~amb & ~(err <= tol)))]
    worst_amb = 0.0
    for (y, x), alts in wk.alternatives.items():
        e = float(np.abs(alts - img[y, x]).max(axis=-1).min())
        worst_amb = max(worst_amb, e)
        if not e <= tol:
            bad.append((y, x, e))
    return Verdict(worst_decided, worst_amb, bad, int(amb.sum()), len(wk.left_out))


def explain_excursions(wk: Walk, image_hw3, ref_hw3, bar: float, tol: float):
    """For the tests that keep a count-based bar: every pixel on which `image` and `ref` differ by more than `bar` must be
    an ambiguous pixel, and both frames must lie within `tol` of one of its alternatives.  Returns the pixels that are not."""
    img, ref = np.asarray(image_hw3, np.float64), np.asarray(ref_hw3, np.float64)
    d = np.abs(img - ref).max(axis=-1)
    bad = []
    for y, x in zip(*np.nonzero(d > bar)):
        alts = wk.alternatives.get((int(y), int(x)))
        if alts is None:
            bad.append((int(y), int(x), float(d[y, x]), "decided" if not wk.ambiguous[y, x] else "left out"))
            continue
        e_img = float(np.abs(alts - img[y, x]).max(axis=-1).min())
        e_ref = float(np.abs(alts - ref[y, x]).max(axis=-1).min())
        if not (e_img <= tol and e_ref <= tol):
            bad.append((int(y), int(x), float(d[y, x]), "no alternative: %.3g / %.3g" % (e_img, e_ref)))
    return bad
