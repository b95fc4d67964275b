"""Anti-aliased GSX_SEM_STD_3DGS (GSX_FLAG_ANTIALIASED): the opacity compensation of the 0.3 dilation, forward and backward,
restated on top of rule_set_restatement (the float64 walk that knows its margins) and std3dgs_backward_restatement (the
gradients of the std_3dgs frame).

TEST INFRASTRUCTURE ONLY.  Plain numpy.

Rule.  With c = (ca0, cb, cd0) the EWA covariance BEFORE the dilation and (ca1, cd1) = (ca0 + 0.3, cd0 + 0.3):
    det0 = ca0 cd0 - cb cb      det1 = ca1 cd1 - cb cb      ratio = det0 / det1
    rho = sqrt(max(0.000025, ratio))       op_eff = sigmoid(logit) rho
and where ratio <= 0.000025 (a float32 det0 <= 0 included) rho is the constant 0.005 and carries no gradient.

float32 stage-1 mirror (`covariance32`, `factor`).  The covariance is formed by oracle/std3dgs_ref.py's own steps with
its own helpers (the operation order it shares with the C port and with gsx_project.hip), and the factor by the operations
of gsx_internal.h's std_aa_factor in their order: two rounded products and a difference for each determinant, one quotient,
one comparison, one square root.  `rows_antialiased` puts op_eff = fl(sigmoid32 rho32) into the opacity column of the C
port's stage-1 rows.

Forward.  The float64 walk of rule_set_restatement runs on records built from THOSE rows.  Deliberately: float32 det0
cancels badly for needles (ca cd / det0 reaches 1e5), so a float64 rho differs from any float32 renderer's by far more than
a pixel tolerance; with the mirror's op_eff as the record's opacity the walk's own margins apply unchanged.

Backward.  alpha = op_eff G, so U = sum u (composite()'s fourth sum) is dL/d ln op_eff:
    dL/dlogit = U (1 - sigmoid)
    ln rho = 1/2 (ln det0 - ln det1), unclamped:
        dg_ca = 1/2 U (cd0 / det0 - cd1 / det1)      dg_cd = 1/2 U (ca0 / det0 - ca1 / det1)
        dg_cb = -U cb (1 / det0 - 1 / det1)          (the off-diagonal total)
and nothing where rho is clamped.  Everything behind dL/dcov is std3dgs_backward_restatement.chain_std, which is LINEAR in
dL/dcov; it is reused unchanged through one identity: on a stage-1 dict whose conic is 0 and whose determinant is 1, its
step (1) maps the moments (0, 0, S3, S4, S5) to dL/dcov = (-S5 / 2, S4, -S3 / 2) exactly (halving, x / 1 and + 0 are exact
in any format), so chain_std(fake, (0, 0, -2 dg_cd, dg_cb, -2 dg_ca)) IS the chain's tail applied to (dg_ca, dg_cb, dg_cd),
with a zero dL/d(NDC mean) -- which the factor does not reach.  The gradients of the anti-aliased frame are the sum of that
and chain_std on the moments.  float64: the restatement (held to torch autograd of an independent forward at 1e-9,
tests/test_antialias_host.py).  float32: the mirror -- the three terms in the kernel's operations on the mirror's float32
(ca0, cb, cd0), i.e. with the float32 det0 the kernel has, the tail in float32; the kernel adds the terms to dL/dcov before
one tail where the mirror adds two tails, a difference of a few roundings of the result.
U is recovered from composite()'s dL/dlogit = U (1 - op) by dividing by the same (1 - op) in float64 (float32 mirror: at
most one ulp of U from the two roundings).

Error scale.  The chain's scale gains the matching absolute-value term: the same tail, through
geometry_backward_restatement.chain(absolute=True) and the same identity, of
    |U|_abs (|cd0| / |det0| + |cd1| / |det1|) / 2,   |U|_abs (|ca0| / |det0| + |ca1| / |det1|) / 2,
    |U|_abs |cb| (1 / |det0| + 1 / |det1|)
with |U|_abs = sum ua, the bound composite() keeps for the terms U adds up; opacity: |U|_abs (1 - sigmoid).

Clamp band (`ratio_bound`).  A fixture may hold no Gaussian whose clamp decision float32 could take either way: the
float64 ratio must lie outside 0.000025 (1 +- r), r the mirror's relative error bound for ratio, per Gaussian.  With
u = 2^-24 and E = |T| |Sigma| |T|^T the covariance formed from absolute values: an entry of the covariance is the result of
J (3 roundings an entry), T = J W (2), Sigma (M: 1, three products and two sums: 5), T Sigma (5), .. W^T (3), .. J^T (3),
21 in all, rounded up to dc = 24 u E entrywise.  Then
    d(det0) <= |cd0| dc_a + |ca0| dc_d + 2 |cb| dc_b + 2 u (|ca0 cd0| + cb^2)          (and the same at the dilated entries,
    r = d(det0) / |det0| + d(det1) / |det1| + u                                          whose sums add one rounding each)
A relative bound says nothing where float32 cannot tell the sign of det0 (r >= 1: the thin needles whose float32 det0 comes
out <= 0, which the needle fixture holds on purpose): there the same quantities give the absolute bound
    delta = (d(det0) + |ratio| d(det1)) / |det1| + u |ratio|
and the row is off the band when ratio + delta < 0.000025: every float32 value of the ratio is clamped.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

import geometry_backward_restatement as gbr
import rule_set_restatement as rsr
import std3dgs_backward_restatement as sbr
from oracle.cpu_ref import _mm3, _mm3_single, _row4
from oracle.std3dgs_ref import _rotation

f32 = np.float32
U32 = 2.0 ** -24
FLOOR = f32(0.000025)
RHO_FLOOR = f32(0.005)
DILATION = f32(0.3)
K_COV = 24.0              # roundings behind one entry of the float32 covariance, rounded up (module doc)
KEYS = ("colors", "opacity", "points", "scales", "quaternions", "means2d")


def covariance32(points, scales, quats, cam):
    """(ca0, cb, cd0) float32 of every row, before the dilation: oracle/std3dgs_ref.stage1's steps, in its order."""
    p = np.ascontiguousarray(np.asarray(points, f32).reshape(-1, 3))
    s = np.asarray(scales, f32).reshape(-1, 3)
    q = np.asarray(quats, f32).reshape(-1, 4)
    n = p.shape[0]
    V = cam.world2view
    W, H = int(cam.width), int(cam.height)
    with np.errstate(all="ignore"):
        tz = _row4(p, V, 2)
        n1 = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        n1 = np.maximum(n1, f32(1e-12))
        R = _rotation(q / n1[:, None])
        M = R * s[:, None, :]
        S = np.empty_like(M)
        for i in range(3):
            for j in range(3):
                S[:, i, j] = (M[:, i, 0] * M[:, j, 0] + M[:, i, 1] * M[:, j, 1]) + M[:, i, 2] * M[:, j, 2]
        fx = f32(W) / (f32(2.0) * f32(cam.tan_fovx))
        fy = f32(H) / (f32(2.0) * f32(cam.tan_fovy))
        tx, ty = _row4(p, V, 0), _row4(p, V, 1)
        limx, limy = f32(1.3) * f32(cam.tan_fovx), f32(1.3) * f32(cam.tan_fovy)
        cx = np.minimum(np.maximum(tx / tz, -limx), limx) * tz
        cy = np.minimum(np.maximum(ty / tz, -limy), limy) * tz
        J = np.zeros((n, 3, 3), dtype=f32)
        J[:, 0, 0] = fx / tz
        J[:, 0, 2] = -(fx * cx) / (tz * tz)
        J[:, 1, 1] = fy / tz
        J[:, 1, 2] = -(fy * cy) / (tz * tz)
        Wm = np.ascontiguousarray(V[:3, :3].T)
        D = _mm3(_mm3_single(_mm3(_mm3_single(J, Wm), S), np.ascontiguousarray(Wm.T)),
                 np.ascontiguousarray(np.transpose(J, (0, 2, 1))))
    return D[:, 0, 0].astype(f32), D[:, 0, 1].astype(f32), D[:, 1, 1].astype(f32)


class Factor(NamedTuple):
    ca0: np.ndarray
    cb: np.ndarray
    cd0: np.ndarray
    ca1: np.ndarray
    cd1: np.ndarray
    det0: np.ndarray
    det1: np.ndarray
    ratio: np.ndarray
    clamped: np.ndarray       # rho is the constant 0.005 and carries no gradient
    rho: np.ndarray


def factor(ca0, cb, cd0, clamped=None) -> Factor:
    """std_aa_factor's operations in the dtype of the inputs (float32: the mirror, every operation rounded; float64: the
    rule).  clamped: the decision to take instead of this dtype's own (the float64 side is given the float32 decision)."""
    dt = np.asarray(ca0).dtype.type
    ca0, cb, cd0 = (np.asarray(a, dt) for a in (ca0, cb, cd0))
    with np.errstate(all="ignore"):
        ca1, cd1 = ca0 + dt(DILATION), cd0 + dt(DILATION)
        det1 = ca1 * cd1 - cb * cb
        det0 = ca0 * cd0 - cb * cb
        ratio = det0 / det1
        own = ~(ratio > dt(FLOOR))
        cl = own if clamped is None else np.asarray(clamped, bool)
        rho = np.where(cl, dt(RHO_FLOOR), np.sqrt(np.where(cl, dt(1.0), ratio))).astype(dt)
    return Factor(ca0, cb, cd0, ca1, cd1, det0, det1, ratio, cl, rho)


def factor_of_stage1(st: dict, clamped=None) -> Factor:
    """The factor from a std3dgs_backward_restatement.stage1_std dict.  Its `cov` is the dilated covariance, and taking the
    0.3 off again would cost det0 its last digits: the undilated one is formed again, by the product stage1_std forms."""
    with np.errstate(all="ignore"):
        cov = st["T"] @ st["Sg"] @ st["T"].transpose(0, 2, 1)
    return factor(cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1], clamped)


def rows_antialiased(rows, fac32: Factor) -> np.ndarray:
    """The C port's (n, 8) stage-1 rows with opacity -> op_eff = fl(sigmoid32 * rho32), what pack_record stores."""
    out = np.array(rows, f32, copy=True)
    out[:, 7] = (out[:, 7] * fac32.rho).astype(f32)
    return out


def ratio_bound(st64: dict, fac64: Factor):
    """(r, delta) of the module doc, per row of the float64 stage 1 `st64` (std3dgs_backward_restatement.stage1_std)."""
    T, Sg = np.abs(st64["T"]), np.abs(st64["Sg"])
    E = T @ Sg @ T.transpose(0, 2, 1)
    dca, dcb, dcd = (K_COV * U32 * E[:, i, j] for i, j in ((0, 0), (0, 1), (1, 1)))
    a0, b, d0, a1, d1 = (np.abs(v) for v in (fac64.ca0, fac64.cb, fac64.cd0, fac64.ca1, fac64.cd1))
    with np.errstate(all="ignore"):
        e0 = d0 * dca + a0 * dcd + 2 * b * dcb + 2 * U32 * (a0 * d0 + b * b)
        e1 = d1 * (dca + U32 * a1) + a1 * (dcd + U32 * d1) + 2 * b * dcb + 2 * U32 * (a1 * d1 + b * b)
        r = e0 / np.abs(fac64.det0) + e1 / np.abs(fac64.det1) + U32
        delta = (e0 + np.abs(fac64.ratio) * e1) / np.abs(fac64.det1) + U32 * np.abs(fac64.ratio)
    return r, delta


def on_the_clamp_band(fac64: Factor, r, delta) -> np.ndarray:
    """Rows whose clamp decision float32 could take either way: the float64 ratio inside 0.000025 (1 +- r), or, where
    r >= 1, not below 0.000025 by more than delta."""
    lo, hi = float(FLOOR) * (1.0 - r), float(FLOOR) * (1.0 + r)
    with np.errstate(invalid="ignore"):
        relative = ~((fac64.ratio < lo) | (fac64.ratio > hi))
        absolute = ~(fac64.ratio + delta < float(FLOOR))
    return np.where(r < 1.0, relative, absolute)


def rho_terms(fac: Factor, U, absolute: bool = False):
    """(dg_ca, dg_cb, dg_cd) of the module doc in fac's dtype, zero where rho is clamped, in geometry_chain's operations;
    absolute: the matching absolute-value terms from U = |U|_abs (float64)."""
    dt = fac.ca0.dtype.type
    U = np.asarray(U).astype(dt)
    with np.errstate(all="ignore"):
        if absolute:
            a = np.abs
            g_ca = 0.5 * U * (a(fac.cd0) / a(fac.det0) + a(fac.cd1) / a(fac.det1))
            g_cd = 0.5 * U * (a(fac.ca0) / a(fac.det0) + a(fac.ca1) / a(fac.det1))
            g_cb = U * a(fac.cb) * (1.0 / a(fac.det0) + 1.0 / a(fac.det1))
        else:
            hu = dt(0.5) * U
            g_ca = hu * (fac.cd0 / fac.det0 - fac.cd1 / fac.det1)
            g_cd = hu * (fac.ca0 / fac.det0 - fac.ca1 / fac.det1)
            g_cb = -(U * fac.cb) * (dt(1.0) / fac.det0 - dt(1.0) / fac.det1)
    zero = dt(0.0)
    return tuple(np.where(fac.clamped, zero, g).astype(dt) for g in (g_ca, g_cb, g_cd))


def _tail_moments(g_ca, g_cb, g_cd):
    z = np.zeros_like(g_ca)
    return np.stack([z, z, -2 * g_cd, g_cb, -2 * g_ca], 1)


def _fake(st: dict) -> dict:
    """`st` with a zero conic and a unit determinant: chain_std's step (1) then hands the moments through (module doc)."""
    m = st["xy"].shape[0]
    dt = st["xy"].dtype.type
    return dict(st, Q=np.zeros((m, 2, 2), dt), det=np.ones(m, dt))


def chain_tail(st: dict, g_ca, g_cb, g_cd):
    """(dL/dpoints, dL/dscales, dL/dquaternions) from dL/dcov = (g_ca, g_cb total, g_cd): chain_std's tail, in st's dtype."""
    gp, gs, gq, gn = sbr.chain_std(_fake(st), _tail_moments(g_ca, g_cb, g_cd))
    assert not np.asarray(gn).any()
    return gp, gs, gq


def chain_tail_abs(st64: dict, g_ca, g_cb, g_cd):
    """The error scale's share: the same tail on absolute values (geometry_backward_restatement.chain(absolute=True), whose
    step (1) gives (S5 / 2, S4 / 2 twice, S3 / 2) on the same stage-1 dict)."""
    z = np.zeros_like(g_ca)
    S = np.stack([z, z, 2 * g_cd, g_cb, 2 * g_ca], 1)
    fk = _fake(st64)
    return gbr.chain(fk, np.asarray(fk["Q"], np.float64), S, absolute=True)


class Case(NamedTuple):
    """One anti-aliased frame: what the forward and the backward tests hold the GPU to."""
    rows: np.ndarray          # (n, 8) float32 stage-1 rows, opacity = op_eff (the mirror's)
    sigma: np.ndarray         # (n,) float32 sigmoid(logit), the C port's
    fac32: Factor             # the mirror's factor, every row
    R: rsr.Records
    wk: rsr.Walk


def forward_case(rows, points, scales, quats, cam, colors, tile, background) -> Case:
    """rows: the C port's stage-1 rows of the flag-clear frame (c_oracle.render_std3dgs)."""
    rows = np.asarray(rows, f32).reshape(-1, 8)
    fac32 = factor(*covariance32(points, scales, quats, cam))
    rows_aa = rows_antialiased(rows, fac32)
    W, H = int(cam.width), int(cam.height)
    R = rsr.records_std3dgs(rows_aa, colors, W, H, tile)
    return Case(rows_aa, rows[:, 7].copy(), fac32, R, rsr.walk(rsr.STD_3DGS, R, W, H, background))


def backward(case: Case, dec: sbr.Decisions, points, scales, quats, cam, grad_frame_hw3, background, dtype=np.float64,
             values: Optional[dict] = None, stage1: Optional[dict] = None, sigma=None, fac: Optional[Factor] = None,
             with_rho: bool = True) -> sbr.Gradients:
    """std3dgs_backward_restatement.backward on the anti-aliased records, then the two changes of the module doc.
    dtype float32 is the mirror.  values / stage1: as there (the test against autograd).  sigma: sigmoid(logit) of the rows
    of R (default: the rows' float32 value).  fac: the factor of the rows of R in `dtype` (default: float64 from the float64
    stage 1 with the mirror's clamp decision; float32: the mirror's own).  with_rho=False: U's rho term left out (what the
    clamped rows must equal)."""
    R = case.R
    dt = np.dtype(dtype).type
    rows = np.asarray(R.index, np.int64)
    n = np.asarray(points).shape[0]
    base = sbr.backward(R, dec, points, scales, quats, cam, grad_frame_hw3, background, dtype=dtype, values=values, stage1=stage1)
    pts, scl, qts = (np.asarray(a)[rows] for a in (points, scales, quats))
    st = stage1 if stage1 is not None else sbr.stage1_std(pts, scl, qts, cam, dtype)
    st64 = st if dt == np.float64 else sbr.stage1_std(pts, scl, qts, cam, np.float64)
    clamped = case.fac32.clamped[rows]
    if fac is None:
        if dt == np.float64:
            fac = factor_of_stage1(st64, clamped)
        else:
            fac = factor(case.fac32.ca0[rows], case.fac32.cb[rows], case.fac32.cd0[rows], clamped)
    fac64 = fac if dt == np.float64 else factor_of_stage1(st64, clamped)
    op_eff = (np.asarray(values["opacity"], np.float64) if values is not None else np.asarray(R.opacity, np.float64))
    sg = np.asarray(case.sigma[rows] if sigma is None else sigma, np.float64)
    # U = sum u from dL/dlogit = U (1 - op_eff), per listed row
    with np.errstate(all="ignore"):
        Uall = np.asarray(base.arrays["opacity"], np.float64).reshape(-1)[rows] / (1.0 - op_eff)
        Uabs = np.asarray(base.scales["opacity"], np.float64)[rows] / (1.0 - op_eff)
    Uall = np.where(np.isfinite(Uall), Uall, 0.0).astype(dt)
    Uabs = np.where(np.isfinite(Uabs), Uabs, 0.0)
    arrays, scales_ = dict(base.arrays), dict(base.scales)
    go = np.zeros((n, 1), dt)
    go[rows, 0] = (Uall * (dt(1.0) - sg.astype(dt))).astype(dt)
    so = np.zeros(n)
    so[rows] = Uabs * (1.0 - sg)
    arrays["opacity"], scales_["opacity"] = go, so
    if with_rho:
        gp, gs, gq = chain_tail(st, *rho_terms(fac, Uall))
        ap, as_, aq = chain_tail_abs(st64, *rho_terms(fac64, Uabs, absolute=True))
        for key, add, add_abs in (("points", gp, ap), ("scales", gs, as_), ("quaternions", gq, aq)):
            a = np.array(arrays[key], copy=True)
            a[rows] = (a[rows] + np.asarray(add).astype(dt)).astype(dt)
            arrays[key] = a
            s = np.array(scales_[key], copy=True)
            s[rows] = s[rows] + np.abs(add_abs).sum(1)
            scales_[key] = s
    return sbr.Gradients(base.frame, arrays, scales_, base.clamped_ewa)
