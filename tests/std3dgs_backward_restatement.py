"""float64 restatement of the gradients of the GSX_SEM_STD_3DGS frame (the CPU pin of gsx_render_backward_std), and a
float32 mirror of it in the kernels' operation order.

TEST INFRASTRUCTURE ONLY.  Plain numpy.  Input: the float32 stage-1 rows and records of
test_rule_sets_host.std_case(name) (rule_set_restatement.Records, walk order) and that module's walk.

Decisions (`decide`).  The walk of rule_set_restatement is repeated with its own functions (_pair, _stop_test, _decisions),
so every (pixel, record) pair gets the walk's three decisions -- skipped by power > 0, skipped by alpha < 1/255, stopped
before it, or composited -- and the one decision the forward never needed: the CLAMP.  A composited pair is clamped where
opacity exp(power) >= 0.99f; the kernel tests the float32 product, so the decision is ambiguous where
opacity exp(power) (1 +- r_alpha) straddles 0.99f, r_alpha = 8 u S + 3 u as defined there.
`gradient_mask` = pixels that are decided in the walk and composite no pair with an ambiguous clamp.  dL/dframe is multiplied
by it: every term of every gradient carries its pixel's dL/dframe as a factor, so a masked pixel drops out whichever way
float32 took its decisions.

Compositing (`composite`), per composited pair k of a pixel with g = dL/dpixel, F the forward's pixel (T_fin background
included), C_k the colour accumulated up to and including k:
    dL/dc_k     = T_k alpha_k g
    dL/dalpha_k = T_k (c_k . g) - (F - C_k) . g / (1 - alpha_k)
    u_k         = dL/dalpha_k alpha_k  where the clamp is inactive, 0 where it is active
    dL/dlogit   = (sum u) (1 - opacity)                       opacity = sigmoid(logit), once
    S           = (sum u d0, sum u d1, sum u d0^2, sum u d0 d1, sum u d1^2),  d = mean - pixel
dtype float64: the formulas above on the float64 values of the rows (or of `values`, a float64 stage 1: what the test
against autograd evaluates both sides at).  dtype float32 (the mirror): the kernel's operations -- the exponent in log2
units from the packed Q'' = fl(q fl(-1/2 log2 e)) as pw = fma(e_y, fma(e_y, Q11, e_x Qs), (e_x e_x) Q00), alpha =
min(0.99f, op exp2(pw)), ta = T alpha, C = fma(ta, c, C), T = T - ta, F = fma(T_fin, bg, C), the sums' terms as
gsx_backward_tile.inc forms them -- with the decisions frozen to the float64 walk's; the sums over pixels are numpy's.

Chain (`stage1_std`, `chain_std`), per Gaussian, the rule set's own stage 1 (oracle/std3dgs_ref.py): quaternion normalised
once; Sigma = (R S)(R S)^T; EWA with the view-space point clamped to 1.3 tan(fov/2) and focal = dim / (2 tan(fov/2));
cov00 += 0.3, cov11 += 0.3 (constants); conic = adj / det, no floor, one off-diagonal entry; p_w = 1 / (w + 1e-7);
pixel = ((ndc + 1) dim - 1) / 2, so dL/d(NDC mean) = dL/dpixel-mean (W/2, H/2).  chain_std is written in the order of
gsx_backward.hip's geometry_chain and runs in the dtype of its input: float64 is the restatement, float32 the mirror.

Error scale: geometry_backward_restatement's norm -- the same chain run on absolute values (its `chain(absolute=True)` on
this module's stage 1) from the absolute moments sum ua |d|.., ua = alpha (|F|_1 + |c|_1) |g|_1 / (1 - alpha); colours:
sum T alpha |g|_1; opacity: (sum ua)(1 - opacity).
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import numpy as np

import geometry_backward_restatement as gbr
import rule_set_restatement as rsr

f32 = np.float32
K_LOG2 = f32(-0.5) * f32(1.44269504088896340736)         # pack_record's k
ARRAYS = ("colors", "opacity", "moments", "points", "scales", "quaternions", "means2d")


class Pair(NamedTuple):
    """One record's decisions over its pixel rectangle `s` (a pair of slices); masks of the rectangle's shape."""
    s: tuple
    acc: np.ndarray           # composited
    clamped: np.ndarray       # composited with alpha = 0.99f
    skip_power: np.ndarray    # live, skipped because power > 0
    skip_alpha: np.ndarray    # live, power <= 0, skipped because alpha < 1/255
    stops: np.ndarray         # the pixel stops before this record


class Decisions(NamedTuple):
    pairs: List[Optional[Pair]]       # per record of R, None where it meets no live pixel
    clamp_ambiguous: np.ndarray       # (H, W) composited pairs whose clamp float32 could have decided otherwise
    composited: np.ndarray            # (H, W)
    stop_position: np.ndarray         # (H, W) position in the pixel's list of the record that stopped it, -1 if none
    T_final: np.ndarray               # (H, W) float64


def decide(R: rsr.Records, width: int, height: int) -> Decisions:
    rules = rsr.STD_3DGS
    H, W = height, width
    T, e_T = np.ones((H, W)), np.zeros((H, W))
    live = np.ones((H, W), bool)
    clamp_amb = np.zeros((H, W), np.int64)
    composited = np.zeros((H, W), np.int64)
    position = np.zeros((H, W), np.int64)
    stop_position = np.full((H, W), -1, np.int64)
    PY, PX = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pairs: List[Optional[Pair]] = []
    for i in range(R.x.shape[0]):
        x0, x1, y0, y1 = R.rect[i]
        if x1 <= x0 or y1 <= y0:
            pairs.append(None)
            continue
        s = (slice(y0, y1), slice(x0, x1))
        lv = live[s]
        if not lv.any():
            pairs.append(None)
            position[s] += 1
            continue
        power, e_power, alpha, r_alpha = rsr._pair(rules, R, i, PX[s], PY[s])
        test, lo, hi, e_next = rsr._stop_test(T[s], e_T[s], alpha, r_alpha)
        skip_p, _, skip_a, _, stop, _ = rsr._decisions(rules, power, e_power, alpha, r_alpha, test, lo, hi)
        took_a = lv & ~skip_p
        used = took_a & ~skip_a
        stops, acc = used & stop, used & ~stop
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            raw = R.opacity[i] * np.exp(power)
        r = e_power + rsr.K_EXP_MUL * rsr.U
        clamped = acc & (raw >= rsr.CLAMP)
        clamp_amb[s] += acc & ((raw * (1.0 - r) < rsr.CLAMP) != (raw * (1.0 + r) < rsr.CLAMP))
        T[s] = np.where(acc, test, T[s])
        e_T[s] = np.where(acc, e_next, e_T[s])
        composited[s] += acc
        stop_position[s] = np.where(stops, position[s], stop_position[s])
        live[s] = lv & ~stops
        position[s] += 1
        pairs.append(Pair(s, acc, clamped, lv & skip_p, took_a & skip_a, stops))
    return Decisions(pairs, clamp_amb, composited, stop_position, T)


def gradient_mask(wk: rsr.Walk, dec: Decisions) -> np.ndarray:
    """(H, W) bool: decided in the walk, and no ambiguous clamp."""
    return ~wk.ambiguous & (dec.clamp_ambiguous == 0)


def _fma(a, b, c, dt):
    if dt == np.float64:
        return a * b + c
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


class Composite(NamedTuple):
    frame: np.ndarray         # (H, W, 3) the forward's frame under the frozen decisions
    colors: np.ndarray        # (n, 3) dL/dcolors, original row order
    opacity: np.ndarray       # (n,) dL/dlogit
    moments: np.ndarray       # (n, 5)
    scale_colors: np.ndarray  # (n,)
    scale_opacity: np.ndarray
    moments_abs: np.ndarray   # (n, 5)


def composite(R: rsr.Records, dec: Decisions, grad_frame_hw3, background, n: int, width: int, height: int, dtype=np.float64,
              values: Optional[dict] = None, frame=None) -> Composite:
    """Forward under the frozen decisions, then the sums of the module doc.  values: float64 (m,) arrays x, y, A, B, C,
    opacity and (m, 3) colors in R's order used in place of the rows' (dtype float64 only).  frame: the F the backward reads
    (default: this function's own forward)."""
    dt = np.dtype(dtype).type
    H, W = height, width
    P = dict(x=R.x, y=R.y, A=R.A, B=R.B, C=R.C, opacity=R.opacity, colors=R.colors)
    if values is not None:
        assert dt == np.float64
        P.update(values)
    P = {k: np.asarray(v, np.float64).astype(dt) for k, v in P.items()}
    if dt == f32:
        Q00, Qs, Q11 = (P["A"] * K_LOG2).astype(f32), ((P["B"] + P["B"]) * K_LOG2).astype(f32), (P["C"] * K_LOG2).astype(f32)
    PY, PX = np.meshgrid(np.arange(H).astype(dt), np.arange(W).astype(dt), indexing="ij")
    clamp = dt(f32(0.99))
    bg = np.asarray(background, np.float64).astype(dt)
    g = np.asarray(grad_frame_hw3, np.float64).astype(dt)
    one = dt(1.0)

    def alpha_of(i, s):
        e0, e1 = P["x"][i] - PX[s], P["y"][i] - PY[s]
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            if dt == f32:
                pw = _fma(e1, _fma(e1, Q11[i], e0 * Qs[i], dt), (e0 * e0) * Q00[i], dt)
                raw = (P["opacity"][i] * np.exp2(pw)).astype(f32)
            else:
                raw = P["opacity"][i] * np.exp(-0.5 * (P["A"][i] * e0 * e0 + P["C"][i] * e1 * e1) - P["B"][i] * e0 * e1)
        return e0, e1, raw

    # forward
    T = np.ones((H, W), dt)
    C = np.zeros((H, W, 3), dt)
    for i, pr in enumerate(dec.pairs):
        if pr is None or not pr.acc.any():
            continue
        _, _, raw = alpha_of(i, pr.s)
        alpha = np.where(pr.clamped, clamp, raw)
        ta = np.where(pr.acc, T[pr.s] * alpha, dt(0.0)).astype(dt)
        for ch in range(3):
            C[pr.s + (ch,)] = _fma(ta, P["colors"][i, ch], C[pr.s + (ch,)], dt)
        T[pr.s] = T[pr.s] - ta
    own = np.stack([_fma(T, bg[ch], C[..., ch], dt) for ch in range(3)], axis=-1)
    F = own if frame is None else np.asarray(frame, np.float64).astype(dt)
    # backward
    gc, go, S = np.zeros((n, 3), dt), np.zeros(n, dt), np.zeros((n, 5), dt)
    sc, so, Sabs = np.zeros(n), np.zeros(n), np.zeros((n, 5))
    T = np.ones((H, W), dt)
    C = np.zeros((H, W, 3), dt)
    g_l1, f_l1 = np.abs(g).sum(-1).astype(np.float64), np.abs(F).sum(-1).astype(np.float64)
    for i, pr in enumerate(dec.pairs):
        if pr is None or not pr.acc.any():
            continue
        s, acc, row = pr.s, pr.acc, int(R.index[i])
        e0, e1, raw = alpha_of(i, s)
        alpha = np.where(acc, np.where(pr.clamped, clamp, raw), dt(0.0)).astype(dt)
        Tk = T[s]
        ta = (Tk * alpha).astype(dt)
        c = P["colors"][i]
        for ch in range(3):
            C[s + (ch,)] = _fma(ta, c[ch], C[s + (ch,)], dt)
        G, Cs, Fs = g[s], C[s], F[s]
        cg = (c[0] * G[..., 0] + c[1] * G[..., 1]) + c[2] * G[..., 2]
        rest = ((Fs[..., 0] - Cs[..., 0]) * G[..., 0] + (Fs[..., 1] - Cs[..., 1]) * G[..., 1]) + (Fs[..., 2] - Cs[..., 2]) * G[..., 2]
        da = Tk * cg - rest / (one - alpha)
        free = acc & ~pr.clamped
        u = np.where(free, da * alpha, dt(0.0)).astype(dt)
        u0, u1 = u * e0, u * e1
        gc[row] += (ta[..., None] * G).reshape(-1, 3).sum(0)
        go[row] += u.sum()
        S[row] += np.stack([u0, u1, u0 * e0, u0 * e1, u1 * e1], -1).reshape(-1, 5).sum(0)
        a64 = alpha.astype(np.float64)
        sc[row] += (ta.astype(np.float64) * g_l1[s]).sum()
        ua = np.where(free, a64 * (f_l1[s] + np.abs(c).sum()) * g_l1[s] / (1.0 - a64), 0.0)
        a0, a1 = np.abs(e0).astype(np.float64), np.abs(e1).astype(np.float64)
        so[row] += ua.sum()
        Sabs[row] += np.stack([ua * a0, ua * a1, ua * a0 * a0, ua * a0 * a1, ua * a1 * a1], -1).reshape(-1, 5).sum(0)
        T[s] = Tk - ta
    # dL/dlogit = (sum u)(1 - op): per original row
    op_row = np.zeros(n, dt)
    op_row[R.index] = P["opacity"]
    return Composite(own, gc, (go * (one - op_row)).astype(dt), S, sc, so * (1.0 - op_row.astype(np.float64)), Sabs)


def stage1_std(points, scales, quats, cam, dtype=np.float64, focal=None, limits=None) -> dict:
    """The rule set's stage 1 of every row given (no culling) in `dtype`, with the keys geometry_backward_restatement.chain
    reads (b = a and n2 = 1: one normalisation; floored nowhere; h_w already holds the + 1e-7).  focal, limits: (fx, fy) and
    (limx, limy) to take in place of the camera's own -- a seam for tests that hand the mirror deliberately wrong ones."""
    dt = np.dtype(dtype).type
    p, s, q = (np.asarray(a, np.float64).astype(dt) for a in (points, scales, quats))
    V, F = np.asarray(cam.world2view, np.float64).astype(dt), np.asarray(cam.full_proj, np.float64).astype(dt)
    W, H = int(cam.width), int(cam.height)
    m = p.shape[0]
    n1 = np.maximum(np.sqrt((q * q).sum(1)), dt(1e-12))
    a = q / n1[:, None]
    w, x, y, z = a.T
    R = np.empty((m, 3, 3), dt)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    M = R * s[:, None, :]
    Sg = M @ M.transpose(0, 2, 1)
    ph = np.concatenate([p, np.ones((m, 1), dt)], 1)
    t = (ph @ V)[:, :3]
    tz = t[:, 2]
    tan_x, tan_y = dt(f32(cam.tan_fovx)), dt(f32(cam.tan_fovy))
    limx, limy = (dt(f32(1.3)) * tan_x, dt(f32(1.3)) * tan_y) if limits is None else (dt(limits[0]), dt(limits[1]))
    with np.errstate(all="ignore"):
        rx, ry = t[:, 0] / tz, t[:, 1] / tz
        kx, ky = np.clip(rx, -limx, limx), np.clip(ry, -limy, limy)
        inx, iny = (rx >= -limx) & (rx <= limx), (ry >= -limy) & (ry <= limy)
        cx, cy = kx * tz, ky * tz
        fx, fy = (dt(W) / (dt(2.0) * tan_x), dt(H) / (dt(2.0) * tan_y)) if focal is None else (dt(focal[0]), dt(focal[1]))
        J = np.zeros((m, 2, 3), dt)
        J[:, 0, 0] = fx / tz; J[:, 0, 2] = -(fx * cx) / (tz * tz)
        J[:, 1, 1] = fy / tz; J[:, 1, 2] = -(fy * cy) / (tz * tz)
        Wm = np.ascontiguousarray(V[:3, :3].T)
        T = J @ Wm
        cov = T @ Sg @ T.transpose(0, 2, 1)
        cov[:, 1, 0] = cov[:, 0, 1]                       # one off-diagonal entry serves for both
        cov[:, 0, 0] += dt(f32(0.3))
        cov[:, 1, 1] += dt(f32(0.3))
        det = cov[:, 0, 0] * cov[:, 1, 1] - cov[:, 0, 1] * cov[:, 0, 1]
        Q = np.empty((m, 2, 2), dt)
        Q[:, 0, 0] = cov[:, 1, 1] / det; Q[:, 1, 1] = cov[:, 0, 0] / det
        Q[:, 0, 1] = Q[:, 1, 0] = -cov[:, 0, 1] / det
        h = ph @ F
        h[:, 3] = h[:, 3] + dt(f32(0.0000001))
        sx, sy = dt(W) * dt(0.5), dt(H) * dt(0.5)
        ndc = np.stack([h[:, 0] / h[:, 3], h[:, 1] / h[:, 3]], 1)
        xy = np.stack([((ndc[:, 0] + 1) * dt(W) - 1) * dt(0.5), ((ndc[:, 1] + 1) * dt(H) - 1) * dt(0.5)], 1)
    return dict(xy=xy, ndc=ndc, Q=Q, cov=cov, det=det, floored=np.zeros(m, bool), T=T, Sg=Sg, M=M, R=R, s=s, a=a, b=a,
                n1=n1, n2=np.ones(m, dt), t=t, kx=kx, ky=ky, inx=inx, iny=iny, cx=cx, cy=cy, h=h, V=V, F=F, Wm=Wm, fx=fx,
                fy=fy, sx=sx, sy=sy, clamped=~(inx & iny))


def chain_std(st: dict, S):
    """(dL/dpoints, dL/dscales, dL/dquaternions, dL/d(NDC mean)) of the rows of `st` from their moments S (m, 5), in the
    order of gsx_backward.hip's geometry_chain (kStd) and in the dtype of `st`."""
    dt = st["xy"].dtype.type
    S = np.asarray(S).astype(dt)
    S1, S2, S3, S4, S5 = S.T
    Q, cov, det = st["Q"], st["cov"], st["det"]
    q00, q01, q11 = Q[:, 0, 0], Q[:, 0, 1], Q[:, 1, 1]
    ca, cb, cd = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
    half = dt(-0.5)
    with np.errstate(all="ignore"):
        gq00, gq01, gq11 = half * S3, half * S4, half * S5
        gmx = half * (2 * q00 * S1 + (q01 + q01) * S2)
        gmy = half * ((q01 + q01) * S1 + 2 * q11 * S2)
        g_ca, g_cd, g_cb, g_cc = gq11 / det, gq00 / det, -gq01 / det, -gq01 / det
        g_det = -(((gq00 * q00 + gq01 * q01) + gq01 * q01) + gq11 * q11) / det
        g_ca = g_ca + g_det * cd
        g_cd = g_cd + g_det * ca
        g_cb = (g_cb - g_det * cb) + (g_cc - g_det * cb)
        G = np.zeros((S.shape[0], 2, 2), dt)
        G[:, 0, 0], G[:, 0, 1], G[:, 1, 1] = g_ca, g_cb, g_cd
        T, Sg, V, F = st["T"], st["Sg"], st["V"], st["F"]
        GT, GtT = G @ T, G.transpose(0, 2, 1) @ T
        dS = T.transpose(0, 2, 1) @ GT
        dT = GT @ Sg.transpose(0, 2, 1) + GtT @ Sg
        dJ = dT @ V[:3, :3]
        fx, fy, t, tz = st["fx"], st["fy"], st["t"], st["t"][:, 2]
        cx, cy, kx, ky = st["cx"], st["cy"], st["kx"], st["ky"]
        z2 = tz * tz
        z3 = z2 * tz
        g_cx, g_cy = -dJ[:, 0, 2] * fx / z2, -dJ[:, 1, 2] * fy / z2
        g_z = (-(dJ[:, 0, 0] * fx) / z2 - (dJ[:, 1, 1] * fy) / z2) + (dJ[:, 0, 2] * (2 * fx * cx) / z3 + dJ[:, 1, 2] * (2 * fy * cy) / z3)
        g_z = g_z + (g_cx * kx + g_cy * ky)
        g_rx, g_ry = np.where(st["inx"], g_cx * tz, dt(0)), np.where(st["iny"], g_cy * tz, dt(0))
        g_t = np.stack([g_rx / tz, g_ry / tz, g_z - (g_rx * t[:, 0] + g_ry * t[:, 1]) / z2], 1)
        M, R, s = st["M"], st["R"], st["s"]
        dM = (dS + dS.transpose(0, 2, 1)) @ M
        gs = (dM * R).sum(1)
        d = dM * s[:, None, :]
        w, x, y, z = st["a"].T
        gb = np.stack([
            2 * ((z * (d[:, 1, 0] - d[:, 0, 1]) + y * (d[:, 0, 2] - d[:, 2, 0])) + x * (d[:, 2, 1] - d[:, 1, 2])),
            2 * (((y * (d[:, 0, 1] + d[:, 1, 0]) + z * (d[:, 0, 2] + d[:, 2, 0])) + w * (d[:, 2, 1] - d[:, 1, 2]))
                 - 2 * x * (d[:, 1, 1] + d[:, 2, 2])),
            2 * (((x * (d[:, 0, 1] + d[:, 1, 0]) + z * (d[:, 1, 2] + d[:, 2, 1])) + w * (d[:, 0, 2] - d[:, 2, 0]))
                 - 2 * y * (d[:, 0, 0] + d[:, 2, 2])),
            2 * (((x * (d[:, 0, 2] + d[:, 2, 0]) + y * (d[:, 1, 2] + d[:, 2, 1])) + w * (d[:, 1, 0] - d[:, 0, 1]))
                 - 2 * z * (d[:, 0, 0] + d[:, 1, 1]))], 1)
        a4 = st["a"]
        ga = gb - a4 * (a4 * gb).sum(1, keepdims=True)
        gq = (ga - a4 * (a4 * ga).sum(1, keepdims=True)) / st["n1"][:, None]
        h = st["h"]
        h3 = h[:, 3]
        gn = np.stack([gmx * st["sx"], gmy * st["sy"]], 1)
        gh = np.zeros((S.shape[0], 4), dt)
        gh[:, 0], gh[:, 1] = gn[:, 0] / h3, gn[:, 1] / h3
        gh[:, 3] = -(gn[:, 0] * h[:, 0] + gn[:, 1] * h[:, 1]) / (h3 * h3)
        gp = gh @ F[:3, :].T + g_t @ V[:3, :3].T
    return gp, gs, gq, gn


class Gradients(NamedTuple):
    frame: np.ndarray
    arrays: dict          # name of ARRAYS -> (n, k) array, original row order, zero rows for what is on no composited pair
    scales: dict          # name of ARRAYS -> (n,) error scale
    clamped_ewa: np.ndarray    # (n,) bool: listed rows whose EWA clamp is active


def backward(R: rsr.Records, dec: Decisions, points, scales, quats, cam, grad_frame_hw3, background, dtype=np.float64,
             frame=None, values: Optional[dict] = None, stage1: Optional[dict] = None) -> Gradients:
    """Everything: `composite`, then `chain_std` for the listed rows.  dtype float32 is the mirror.  stage1: a stage1_std
    dict of R.index's rows to run the chain on (default: computed here in `dtype`)."""
    n = np.asarray(points).shape[0]
    W, H = int(cam.width), int(cam.height)
    cp = composite(R, dec, grad_frame_hw3, background, n, W, H, dtype, values, frame)
    rows = np.asarray(R.index, np.int64)
    st = stage1 if stage1 is not None else stage1_std(np.asarray(points)[rows], np.asarray(scales)[rows],
                                                      np.asarray(quats)[rows], cam, dtype)
    gp, gs, gq, gn = chain_std(st, cp.moments[rows])
    st64 = st if np.dtype(dtype) == np.float64 else stage1_std(np.asarray(points)[rows], np.asarray(scales)[rows],
                                                               np.asarray(quats)[rows], cam, np.float64)
    ap, as_, aq = gbr.chain(st64, np.asarray(st64["Q"], np.float64), cp.moments_abs[rows], absolute=True)
    Q64, Sa = np.abs(np.asarray(st64["Q"], np.float64)), cp.moments_abs[rows]
    an = (Q64[:, 0, 0] * Sa[:, 0] + Q64[:, 0, 1] * Sa[:, 1]) * float(st64["sx"]) + \
         (Q64[:, 0, 1] * Sa[:, 0] + Q64[:, 1, 1] * Sa[:, 1]) * float(st64["sy"])
    dt = np.dtype(dtype).type

    def full(arr, k):
        out = np.zeros((n, k), dt)
        out[rows] = arr
        return out

    def full1(arr):
        out = np.zeros(n)
        out[rows] = arr
        return out

    arrays = dict(colors=cp.colors, opacity=cp.opacity.reshape(-1, 1), moments=cp.moments, points=full(gp, 3),
                  scales=full(gs, 3), quaternions=full(gq, 4), means2d=full(gn, 2))
    # a row on no composited pair has zero moments: its chain is zero as well (0 / det and so on), kept exact here
    listed = np.zeros(n, bool)
    listed[rows] = True
    scl = dict(colors=cp.scale_colors, opacity=cp.scale_opacity, moments=cp.moments_abs,
               points=full1(np.abs(ap).sum(1)), scales=full1(np.abs(as_).sum(1)), quaternions=full1(np.abs(aq).sum(1)),
               means2d=full1(an))
    ewa = np.zeros(n, bool)
    ewa[rows] = np.asarray(st64["clamped"])
    return Gradients(cp.frame, arrays, scl, ewa)


def per_gaussian_error(got, ref, scale) -> float:
    """geometry_backward_restatement.per_gaussian_error; a scale of the array's own shape (the moments: five units) is
    applied per component."""
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    scale = np.asarray(scale, np.float64)
    if scale.ndim == 2:
        return max(gbr.per_gaussian_error(got[:, k:k + 1], ref[:, k:k + 1], scale[:, k]) for k in range(scale.shape[1]))
    return gbr.per_gaussian_error(got, ref, scale)


def driving_gradient(width: int, height: int, mask: np.ndarray, seed: int = 7) -> np.ndarray:
    """dL/dframe (H, W, 3) float32: a fixed seeded random image times the gradient mask."""
    rs = np.random.RandomState(seed)
    return (rs.uniform(-1.0, 1.0, (height, width, 3)).astype(f32) * mask[..., None].astype(f32)).astype(f32)
