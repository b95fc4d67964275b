"""Anti-aliased std_3dgs (GSX_FLAG_ANTIALIASED) on the CPU: the restatement (tests/antialias_restatement.py) held to an
independent derivation, the conditions on the fixtures, the figures the GPU tests (tests/test_hip_antialias.py) are held to,
and the refusals that need no GPU.

Independent derivation.  `torch_gradients` writes the anti-aliased forward as a differentiable torch float64 function --
test_std3dgs_backward_host's stage 1 with rho = sqrt(det0 / det1) on the opacity (the constant 0.005 where the float32
mirror clamps), soft compositing with the float64 walk's decisions frozen -- and autograd differentiates sum(frame *
dL/dframe).  The hand-derived chain, evaluated at the same float64 stage-1 values, agrees to 1e-9 of each Gaussian's error
scale for every array on every case: the bar std3dgs_backward_restatement is held to.

Fixtures.  No Gaussian of any case lies on the clamp: the float64 ratio is outside 0.000025 (1 +- r), r the float32 mirror's
relative error bound for the ratio, per Gaussian; where r >= 1 -- float32 cannot tell the sign of det0: the thin needles of
needle_48x48 -- the absolute form of the same bound decides (antialias_restatement.ratio_bound).  A condition on the
fixtures, asserted here; nothing is masked at test time.

E_REF_AA per output array: the float32 mirror's largest error / scale against the float64 restatement over the cases below,
MEASURED HERE (test_e_ref_is_the_mirrors_own_error), recorded and asserted as an upper bound with the last printed digit
as slack; the kernels are held to BOUND_AA = 12 E_REF_AA.  Mirror vs float64, max error / scale per case (E_REF of the
flag-clear frame, tests/test_std3dgs_backward_host.py, in the last line for comparison):
  case                      colors     opacity    points     scales     quaternions  means2d
  stack_half_16x16          1.96e-08   9.58e-10   7.43e-11   4.64e-11   0            3.14e-10
  ring_40x24                2.51e-08   5.04e-09   5.29e-09   9.25e-10   0            6.39e-09
  random_64x64_n800_t2      8.65e-08   1.31e-08   4.39e-09   8.71e-10   4.52e-11     1.17e-08
  random_130x70_n1500_t8    1.11e-07   1.04e-08   4.30e-09   1.43e-09   6.78e-11     7.84e-09
  subpixel_32x32            3.90e-07   3.95e-08   2.47e-08   7.00e-09   2.40e-10     3.82e-08
  needle_48x48              1.41e-07   2.64e-08   1.62e-08   3.42e-07   6.86e-10     2.37e-08
  E_REF_AA                  3.901e-07  3.952e-08  2.469e-08  3.424e-07  6.859e-10    3.818e-08
  E_REF, flag clear         6.627e-07  1.593e-08  1.432e-08  6.141e-09  2.835e-10    2.6e-08
scales on the needles is 56 times the flag-clear figure, quaternions 2.4 times: dL/drho divides by the float32 det0, a
difference of products up to 3.8e4 times its size there (test_the_new_scenes_hold_what_they_are_for prints the range), and
the scales are what that determinant is steepest in.  The factor 12 is the project's, unchanged.
"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import antialias_restatement as aar  # noqa: E402
import rule_set_restatement as rsr  # noqa: E402
import std3dgs_backward_restatement as sbr  # noqa: E402
from intro_to_gaussian_splatting_amd import _ffi, synthetic  # noqa: E402
from oracle import c_oracle, cpu_ref  # noqa: E402
from test_rule_sets_host import STD_BG, STD_CASES  # noqa: E402
from test_std3dgs_backward_host import AUTOGRAD_TOL, MAX_MASKED_SHARE  # noqa: E402

f32 = np.float32
IDENTITY = dict(qvec=np.array([1.0, 0, 0, 0]), tvec=np.zeros(3))
E_REF_AA = {"colors": 3.901e-07, "opacity": 3.952e-08, "points": 2.469e-08, "scales": 3.424e-07, "quaternions": 6.859e-10,
            "means2d": 3.818e-08}       # measured by test_e_ref_is_the_mirrors_own_error
BOUND_AA = {k: 12 * v for k, v in E_REF_AA.items()}
E_REF_SLACK = 1.001


# ----------------------------------------------------------------------------- the two new scenes

def _at_pixels(px, py, z, w, h, fx):
    """World points (identity pose) whose std_3dgs pixel position is (px, py): pixel = ((ndc + 1) W - 1) / 2."""
    return np.stack([(px + 0.5 - w / 2) * z / fx, (py + 0.5 - h / 2) * z / fx, z], axis=1)


def _append(sc, points, scales, quats, logits, rgb):
    add = dict(points=points, scales=scales, quaternions=quats, opacity=np.asarray(logits).reshape(-1, 1), colors_0_255=rgb)
    for key, rows in add.items():
        sc[key] = np.concatenate([sc[key], np.asarray(rows, f32)], 0).astype(f32)
    return sc


def subpixel_scene():
    """120 ordinary Gaussians and 200 whose screen footprint is far below a pixel (sigma 0.02 px: 1.3e-3 px^2, ratio 2e-6 <<
    0.000025), centred on pixels and nearly opaque (logit 6), so that alpha = 0.005 sigmoid exp(..) passes 1/255 at the
    pixel they sit on: clamped rows that composite and carry gradient."""
    w = h = 32
    sc = synthetic.make_scene(120, w, h, seed=41, sigma_scale=1.5, **IDENTITY)
    rs = np.random.RandomState(42)
    m, fx = 200, float(sc["fx"])
    cells = rs.permutation(28 * 28)[:m]
    px, py = 2.0 + cells % 28, 2.0 + cells // 28
    z = rs.uniform(3.0, 6.0, m)
    scales = np.tile((0.02 * z / fx)[:, None], (1, 3)) * rs.uniform(0.8, 1.25, (m, 3))
    return _append(sc, _at_pixels(px, py, z, w, h, fx), scales, rs.normal(size=(m, 4)), np.full(m, 6.0),
                   rs.uniform(0.0, 255.0, (m, 3)))


def needle_scene():
    """100 ordinary Gaussians, 60 long needles (axis ratio 100:1 .. 300:1, 3 .. 8 px long: det0 is a difference of products
    1e4 .. 1e5 times its size, rho unclamped) and 60 thin ones centred on pixels (half a pixel long, 3000:1 .. 10000:1:
    float32 det0 is rounding noise of either sign, ratio << 0.000025 on every float32 path)."""
    w = h = 48
    sc = synthetic.make_scene(100, w, h, seed=43, sigma_scale=1.5, **IDENTITY)
    rs = np.random.RandomState(44)
    fx = float(sc["fx"])
    m = 60
    z = rs.uniform(3.0, 7.0, m)
    long_px, ratio = rs.uniform(3.0, 8.0, m), rs.uniform(100.0, 300.0, m)
    s1 = long_px * z / fx
    scales = np.stack([s1, s1 / ratio, s1 / ratio], 1)
    pts = _at_pixels(rs.uniform(4.0, 44.0, m), rs.uniform(4.0, 44.0, m), z, w, h, fx)
    _append(sc, pts, scales, rs.normal(size=(m, 4)), rs.uniform(0.0, 3.0, m), rs.uniform(0.0, 255.0, (m, 3)))
    z = rs.uniform(3.0, 7.0, m)
    cells = rs.permutation(40 * 40)[:m]
    s1, ratio = 0.5 * z / fx, rs.uniform(3000.0, 10000.0, m)
    scales = np.stack([s1, s1 / ratio, s1 / ratio], 1)
    pts = _at_pixels(4.0 + cells % 40, 4.0 + cells // 40, z, w, h, fx)
    return _append(sc, pts, scales, rs.normal(size=(m, 4)), np.full(m, 6.0), rs.uniform(0.0, 255.0, (m, 3)))


def small_scene(size):
    """400 Gaussians around a third of a 64x64 frame's pixel in size, seen at 64x64 or, with the same field of view, at
    16x16 (a quarter of the focal length): what the opacity compensation is for."""
    sc = synthetic.make_scene(400, 64, 64, seed=45, sigma_scale=0.25, **IDENTITY)
    sc["opacity"] = (sc["opacity"] + f32(2.0)).astype(f32)
    k = size / 64.0
    sc.update(fx=np.float64(sc["fx"] * k), fy=np.float64(sc["fy"] * k), cx=np.float64(size / 2), cy=np.float64(size / 2),
              width=np.int64(size), height=np.int64(size))
    return sc


OLD_CASES = ["stack_half_16x16", "ring_40x24", "random_64x64_n800_t2", "random_130x70_n1500_t8"]
CASES = {name: STD_CASES[name] for name in OLD_CASES}
CASES["subpixel_32x32"] = (subpixel_scene, 16, STD_BG)
CASES["needle_48x48"] = (needle_scene, 16, STD_BG)
BACKWARD_CASES = list(CASES)
CASES["small_64x64"] = (lambda: small_scene(64), 16, STD_BG)
CASES["small_16x16"] = (lambda: small_scene(16), 16, STD_BG)


def build_case(sc, tile, bg, cam=None, colors=None):
    """One frame's flag-clear C-port rows and the anti-aliased restatement on them (antialias_restatement.forward_case)."""
    w, h = int(sc["width"]), int(sc["height"])
    cam = cpu_ref.build_camera(sc["qvec"], sc["tvec"], sc["fx"], sc["fy"], w, h) if cam is None else cam
    colors = (sc["colors_0_255"] / f32(256.0)).astype(f32) if colors is None else colors
    _, nvis, inst, rows = c_oracle.render_std3dgs(sc["points"], colors, sc["scales"], sc["quaternions"], sc["opacity"], cam,
                                                  tile=tile, background=bg, nthreads=8)
    fwd = aar.forward_case(rows, sc["points"], sc["scales"], sc["quaternions"], cam, colors, tile, bg)
    return dict(sc=sc, tile=tile, bg=bg, cam=cam, colors=colors, rows0=np.asarray(rows, f32).reshape(-1, 8), nvis=nvis,
                inst=inst, fwd=fwd, W=w, H=h, n=int(sc["points"].shape[0]))


@functools.lru_cache(maxsize=None)
def forward_case(name):
    make, tile, bg = CASES[name]
    return build_case(make(), tile, bg)


@functools.lru_cache(maxsize=None)
def backward_case(name):
    """forward_case(name) and: the decisions, the gradient mask, dL/dframe, `ref` (float64) and `mirror` (float32)."""
    return build_backward(forward_case(name))


def build_backward(case):
    """backward_case's dict of any build_case dict."""
    case = dict(case)
    fwd, sc = case["fwd"], case["sc"]
    dec = sbr.decide(fwd.R, case["W"], case["H"])
    mask = sbr.gradient_mask(fwd.wk, dec)
    g = sbr.driving_gradient(case["W"], case["H"], mask)
    args = (fwd, dec, sc["points"], sc["scales"], sc["quaternions"], case["cam"], g, case["bg"])
    case.update(dec=dec, mask=mask, g=g, ref=aar.backward(*args, dtype=np.float64), mirror=aar.backward(*args, dtype=np.float32))
    return case


# ----------------------------------------------------------------------------- the mirror and the fixtures

@pytest.mark.parametrize("name", list(CASES))
def test_the_mirrors_covariance_is_the_c_ports(name):
    """The dilated conic formed from the mirror's float32 covariance is the C port's stage-1 conic bit for bit: the mirror
    walks the operation order the port shares with gsx_project.hip."""
    covariance_is_the_c_ports(forward_case(name))


def covariance_is_the_c_ports(case):
    fac, rows = case["fwd"].fac32, case["rows0"]
    seen = ~np.isnan(rows[:, 0])
    assert seen.any()
    with np.errstate(all="ignore"):
        inv = f32(1.0) / fac.det1
        conic = np.stack([fac.cd1 * inv, -fac.cb * inv, fac.ca1 * inv], 1).astype(f32)
    assert np.array_equal(conic[seen], rows[seen, 2:5])
    # and op_eff is the rounded product of the port's sigmoid and the mirror's rho
    aa = case["fwd"].rows
    assert np.array_equal(aa[seen, 7], (rows[seen, 7] * fac.rho[seen]).astype(f32))
    assert np.array_equal(aa[seen, :7], rows[seen, :7])
    assert (fac.rho[fac.clamped] == f32(0.005)).all() and (fac.rho[seen] <= f32(1.0)).all()


@pytest.mark.parametrize("name", list(CASES))
def test_no_gaussian_lies_on_the_clamp(name):
    no_gaussian_lies_on_the_clamp(name, forward_case(name))


def no_gaussian_lies_on_the_clamp(name, case):
    """The check on any build_case dict; returns the nearest ratio to the floor, in units of the floor."""
    sc, rows = case["sc"], case["rows0"]
    seen = np.nonzero(~np.isnan(rows[:, 0]))[0]
    st64 = sbr.stage1_std(sc["points"][seen], sc["scales"][seen], sc["quaternions"][seen], case["cam"], np.float64)
    fac64 = aar.factor_of_stage1(st64)
    r, delta = aar.ratio_bound(st64, fac64)
    band = aar.on_the_clamp_band(fac64, r, delta)
    fac32 = case["fwd"].fac32
    nearest = float(np.min(np.maximum(fac64.ratio, 1e-300) / float(aar.FLOOR) + (fac64.ratio < float(aar.FLOOR)) * 1e9))
    print("%s: %d rows, %d clamped (float32), %d with float32 det0 <= 0, %d judged by the absolute bound; nearest ratio to "
          "the floor %.3g x" % (name, seen.size, int(fac32.clamped[seen].sum()), int((fac32.det0[seen] <= 0).sum()),
                                int((r >= 1).sum()), nearest))
    assert not band.any(), (name, seen[band], fac64.ratio[band], r[band])
    # off the band, float32 and float64 take the same decision
    assert np.array_equal(fac32.clamped[seen], fac64.clamped), name
    return nearest


def test_the_new_scenes_hold_what_they_are_for():
    sub, ndl = backward_case("subpixel_32x32"), backward_case("needle_48x48")
    for case, first in ((sub, 120), (ndl, 160)):
        fac, rows = case["fwd"].fac32, case["rows0"]
        tiny = np.arange(case["n"]) >= first
        assert fac.clamped[tiny].all() and not np.isnan(rows[tiny, 0]).any()
        # clamped rows that composite somewhere and carry gradient
        live = tiny & (case["ref"].scales["colors"] > 0) & (case["ref"].scales["opacity"] > 0)
        print("clamped rows with gradient: %d of %d" % (int(live.sum()), int(tiny.sum())))
        assert live.sum() >= 20
        assert np.abs(case["ref"].arrays["points"][live]).max() > 0
    # footprints well under 0.01 px^2: pi sqrt(det0)
    fac = sub["fwd"].fac32
    assert (np.pi * np.sqrt(np.abs(fac.det0[120:].astype(np.float64))) < 0.01).all()
    print("sub-pixel rows: ratio up to %.3g of the floor" % float(fac.ratio[120:].max() / aar.FLOOR))
    assert (fac.ratio[120:] < 0.5 * float(aar.FLOOR)).all()
    # needles: the long ones unclamped with a badly conditioned det0, some thin ones with float32 det0 <= 0
    fac = ndl["fwd"].fac32
    long_ = slice(100, 160)
    cond = (np.abs(fac.ca0 * fac.cd0) + fac.cb * fac.cb)[long_] / np.abs(fac.det0[long_])
    ratio3d = ndl["sc"]["scales"][100:, 0] / ndl["sc"]["scales"][100:, 1]
    print("needles: det0 condition %.3g .. %.3g, %d thin ones with float32 det0 <= 0" % (
        cond.min(), cond.max(), int((fac.det0[160:] <= 0).sum())))
    assert (ratio3d >= 100).all() and not fac.clamped[long_].any() and cond.max() > 1e3
    assert (fac.det0[160:] <= 0).sum() >= 3


# ----------------------------------------------------------------------------- the independent derivation

def torch_gradients(case):
    """test_std3dgs_backward_host.torch_gradients with the opacity compensation: autograd of the float64 forward."""
    sc, cam, fwd, dec = case["sc"], case["cam"], case["fwd"], case["dec"]
    R = fwd.R
    W, H = case["W"], case["H"]
    rows = torch.as_tensor(np.asarray(R.index, np.int64))
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)  # noqa: E731
    P = t64(sc["points"]).requires_grad_(True)
    S = t64(sc["scales"]).requires_grad_(True)
    Q = t64(sc["quaternions"]).requires_grad_(True)
    L = t64(sc["opacity"]).reshape(-1).requires_grad_(True)
    Cc = t64(case["colors"]).requires_grad_(True)
    V, F = t64(cam.world2view), t64(cam.full_proj)
    p, s, q = P[rows], S[rows], Q[rows]
    n1 = torch.clamp(torch.sqrt((q * q).sum(1)), min=1e-12)
    w, x, y, z = (q / n1[:, None]).unbind(1)
    Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                      2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                      2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = Rm * s[:, None, :]
    Sg = M @ M.transpose(1, 2)
    ph = torch.cat([p, torch.ones((p.shape[0], 1), dtype=torch.float64)], 1)
    h = ph @ F
    pw = 1.0 / (h[:, 3] + float(f32(0.0000001)))
    ndc = torch.stack([h[:, 0] * pw, h[:, 1] * pw], 1)
    ndc.retain_grad()
    xy = torch.stack([((ndc[:, 0] + 1.0) * W - 1.0) * 0.5, ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5], 1)
    tan_x, tan_y = float(f32(cam.tan_fovx)), float(f32(cam.tan_fovy))
    fx, fy = W / (2.0 * tan_x), H / (2.0 * tan_y)
    t = ph @ V
    tz = t[:, 2]
    limx, limy = float(f32(1.3)) * tan_x, float(f32(1.3)) * tan_y
    cx = torch.clamp(t[:, 0] / tz, -limx, limx) * tz
    cy = torch.clamp(t[:, 1] / tz, -limy, limy) * tz
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * cx) / (tz * tz), zero, fy / tz, -(fy * cy) / (tz * tz)], 1).reshape(-1, 2, 3)
    Tm = J @ V[:3, :3].t()
    cov = Tm @ Sg @ Tm.transpose(1, 2)
    d = float(f32(0.3))
    ca0, cb, cd0 = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
    ca, cd = ca0 + d, cd0 + d
    det = ca * cd - cb * cb
    conic = torch.stack([cd / det, -cb / det, ca / det], 1)
    # the opacity compensation: the constant where the float32 mirror clamps
    clamped = torch.as_tensor(fwd.fac32.clamped[np.asarray(R.index, np.int64)])
    det0 = ca0 * cd0 - cb * cb
    ratio = torch.where(clamped, torch.ones_like(det0), det0 / det)
    rho = torch.where(clamped, torch.full_like(det0, float(aar.RHO_FLOOR)), torch.sqrt(ratio))
    sigma = torch.sigmoid(L[rows])
    op = sigma * rho
    col = Cc[rows]
    T = torch.ones((H, W), dtype=torch.float64)
    C = torch.zeros((H, W, 3), dtype=torch.float64)
    PY, PX = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    for i, pr in enumerate(dec.pairs):
        if pr is None or not pr.acc.any():
            continue
        sl = pr.s
        dx, dy = xy[i, 0] - PX[sl], xy[i, 1] - PY[sl]
        power = -0.5 * (conic[i, 0] * dx * dx + conic[i, 2] * dy * dy) - conic[i, 1] * dx * dy
        alpha = torch.where(torch.as_tensor(pr.clamped), torch.full_like(power, rsr.CLAMP), op[i] * torch.exp(power))
        Ts = T[sl].clone()
        ta = torch.where(torch.as_tensor(pr.acc), Ts * alpha, torch.zeros_like(alpha))
        C[sl] = C[sl] + ta[..., None] * col[i]
        T[sl] = Ts - ta
    frame = C + T[..., None] * t64(case["bg"])
    (frame * t64(case["g"])).sum().backward()
    z_ = lambda v: np.zeros_like(v.detach().numpy()) if v.grad is None else v.grad.numpy()  # noqa: E731
    values = dict(x=xy[:, 0].detach().numpy(), y=xy[:, 1].detach().numpy(), A=conic[:, 0].detach().numpy(),
                  B=conic[:, 1].detach().numpy(), C=conic[:, 2].detach().numpy(), opacity=op.detach().numpy(),
                  colors=col.detach().numpy())
    return dict(points=z_(P), scales=z_(S), quaternions=z_(Q), opacity=z_(L).reshape(-1, 1), colors=z_(Cc), ndc=z_(ndc),
                frame=frame.detach().numpy()), values, sigma.detach().numpy()


@pytest.mark.parametrize("name", BACKWARD_CASES)
def test_the_restatement_agrees_with_autograd_of_an_independent_forward(name):
    agrees_with_autograd(name, backward_case(name))


def agrees_with_autograd(name, case):
    """The check on any build_backward dict (tests/test_std3dgs_camera_cases_host.py runs it on its own)."""
    fwd, sc = case["fwd"], case["sc"]
    rows = np.asarray(fwd.R.index, np.int64)
    auto, values, sigma = torch_gradients(case)
    st = sbr.stage1_std(sc["points"][rows], sc["scales"][rows], sc["quaternions"][rows], case["cam"], np.float64)
    np.testing.assert_allclose(st["xy"], np.stack([values["x"], values["y"]], 1), rtol=1e-12, atol=1e-9)
    fac = aar.factor_of_stage1(st, fwd.fac32.clamped[rows])
    # (a needle's det0 is a difference of products up to 1e5 times its size: two float64 stage 1 agree on it to 1e-11)
    np.testing.assert_allclose(sigma * fac.rho, values["opacity"], rtol=1e-9)
    got = aar.backward(fwd, case["dec"], sc["points"], sc["scales"], sc["quaternions"], case["cam"], case["g"], case["bg"],
                       dtype=np.float64, values=values, stage1=st, sigma=sigma, fac=fac)
    np.testing.assert_allclose(got.frame, auto["frame"], rtol=0, atol=1e-12)
    worst = {key: sbr.per_gaussian_error(got.arrays[key], auto[key], got.scales[key])
             for key in ("colors", "opacity", "points", "scales", "quaternions")}
    ndc = np.zeros((case["n"], 2))
    ndc[rows] = auto["ndc"]
    worst["means2d"] = sbr.per_gaussian_error(got.arrays["means2d"], ndc, got.scales["means2d"])
    print("%s: restatement vs autograd, max error / scale: %s" % (name, {k: "%.3g" % v for k, v in worst.items()}))
    for key, e in worst.items():
        assert e <= AUTOGRAD_TOL, (name, key, e)
    assert np.abs(auto["points"]).max() > 0 and np.abs(auto["opacity"]).max() > 0
    # the rho term is not a rounding matter: without it the chain is far from autograd wherever a Gaussian is unclamped
    if not fwd.fac32.clamped[rows].all():
        bare = aar.backward(fwd, case["dec"], sc["points"], sc["scales"], sc["quaternions"], case["cam"], case["g"], case["bg"],
                            dtype=np.float64, values=values, stage1=st, sigma=sigma, fac=fac, with_rho=False)
        assert np.abs(bare.arrays["scales"] - auto["scales"]).max() > 1e-6 * np.abs(auto["scales"]).max(), name


def test_e_ref_is_the_mirrors_own_error():
    worst = {k: (0.0, "") for k in aar.KEYS}
    for name in BACKWARD_CASES:
        case = backward_case(name)
        ref, mir = case["ref"], case["mirror"]
        line = {}
        for key in aar.KEYS:
            sc = ref.scales[key]
            assert (np.abs(ref.arrays[key]) <= sc[:, None] * (1 + 1e-9) + 1e-300).all(), (name, key)
            assert np.isfinite(mir.arrays[key]).all() and np.isfinite(ref.arrays[key]).all(), (name, key)
            line[key] = sbr.per_gaussian_error(mir.arrays[key], ref.arrays[key], sc)
            worst[key] = max(worst[key], (line[key], name))
        print("  %-25s %s" % (name, "  ".join("%-10.3g" % line[k] for k in aar.KEYS)))
    print("E_REF_AA = {%s}" % ", ".join('"%s": %.4g' % (k, worst[k][0]) for k in aar.KEYS))
    for key, (val, where) in worst.items():
        print("E_REF_AA %s = %.4g at %s (recorded %.4g, kernels held to %.4g)" % (key, val, where, E_REF_AA[key], BOUND_AA[key]))
    for key, (val, where) in worst.items():
        assert E_REF_AA[key] / 1.5 <= val <= E_REF_AA[key] * E_REF_SLACK, (key, val, where)


@pytest.mark.parametrize("name", BACKWARD_CASES)
def test_the_gradient_mask_leaves_out_at_most_one_percent(name):
    case = backward_case(name)
    wk, mask = case["fwd"].wk, case["mask"]
    assert not wk.left_out, wk.left_out
    assert (~mask).sum() <= MAX_MASKED_SHARE * mask.size, (name, int((~mask).sum()))


def test_clamped_rows_get_the_chain_without_the_rho_term():
    """Rows on the floor: points / scales / quaternions are what the restatement gives with U's rho term absent, bit for bit
    in the mirror and in float64; dL/dlogit is still U (1 - sigmoid)."""
    case = backward_case("subpixel_32x32")
    fwd, sc = case["fwd"], case["sc"]
    args = (fwd, case["dec"], sc["points"], sc["scales"], sc["quaternions"], case["cam"], case["g"], case["bg"])
    clamped = fwd.fac32.clamped
    for dtype, full in ((np.float64, case["ref"]), (np.float32, case["mirror"])):
        bare = aar.backward(*args, dtype=dtype, with_rho=False)
        for key in ("points", "scales", "quaternions"):
            assert np.array_equal(full.arrays[key][clamped], bare.arrays[key][clamped]), key
            assert not np.array_equal(full.arrays[key][~clamped], bare.arrays[key][~clamped]), key
        assert np.array_equal(full.arrays["opacity"], bare.arrays["opacity"])
    # U (1 - sigmoid), not U (1 - op_eff): the flag-clear formula on the same records is off by (1 - op_eff) / (1 - sigmoid)
    rows = np.asarray(fwd.R.index, np.int64)
    plain = sbr.backward(fwd.R, case["dec"], sc["points"], sc["scales"], sc["quaternions"], case["cam"], case["g"], case["bg"])
    live = np.abs(plain.arrays["opacity"][rows, 0]) > 0
    want = plain.arrays["opacity"][rows, 0] / (1.0 - fwd.R.opacity) * (1.0 - fwd.sigma[rows].astype(np.float64))
    np.testing.assert_allclose(case["ref"].arrays["opacity"][rows, 0][live], want[live], rtol=1e-12)


# ----------------------------------------------------------------------------- refusals that need no GPU

def test_the_c_abi_refuses_the_flag_by_name_without_a_gpu():
    lib = _ffi.load()
    assert _ffi.GSX_FLAG_ANTIALIASED == 2048
    cam = _ffi.GsxCamera()
    cam.width, cam.height = 64, 48
    ptr = ctypes.c_void_p(256)      # never dereferenced: every call below is refused before any HIP call

    def params(semantics):
        p = _ffi.default_params()
        p.semantics = semantics
        p.flags |= _ffi.GSX_FLAG_ANTIALIASED
        return p

    def refused(rc):
        msg = lib.gsx_last_error()
        assert rc == _ffi.GSX_ERR_INVALID_ARGUMENT and b"GSX_FLAG_ANTIALIASED" in msg, (rc, msg)

    five = [ptr] * 5
    for sem in (_ffi.GSX_SEM_REF_CPU, _ffi.GSX_SEM_REF_CUDA):
        p = params(sem)
        refused(lib.gsx_render_forward(ctypes.byref(cam), *five, 10, 16, ptr, ctypes.byref(p), None, None, 0, None))
        refused(lib.gsx_render_backward_std(ctypes.byref(cam), *five, 10, 16, ptr, ptr, ptr, ptr, None, None, None, None, None,
                                            ctypes.byref(p), None, 0, None))
        refused(lib.gsx_render_contribution(ctypes.byref(cam), *five, 10, 16, ptr, ptr, ptr, None, 0, ctypes.byref(p), None, 0,
                                            None))
    # the entries that take no std_3dgs frame: with the flag they say so by name, whatever the semantics
    for sem in (_ffi.GSX_SEM_STD_3DGS, _ffi.GSX_SEM_REF_CPU):
        p = params(sem)
        refused(lib.gsx_render_depth(ctypes.byref(cam), *five, 10, 16, ptr, ctypes.byref(p), None, 0, None))
        refused(lib.gsx_render_backward(ctypes.byref(cam), *five, 10, 16, ptr, ptr, ptr, ptr, ctypes.byref(p), None, 0, None))
        refused(lib.gsx_render_backward_geometry(ctypes.byref(cam), *five, 10, 16, ptr, ptr, ptr, ptr, ptr, ptr, ptr,
                                                 ctypes.byref(p), None, 0, None))
        refused(lib.gsx_render_preprocessed(48, 64, 16, *([ptr] * 8), 10, ptr, ctypes.byref(p), None, None, 0, None))
    # under std_3dgs the three entries that honour it go on to their next check
    p = params(_ffi.GSX_SEM_STD_3DGS)
    rc = lib.gsx_render_backward_std(ctypes.byref(cam), *five, 10, 16, ptr, ptr, ptr, ptr, None, None, None, None, None,
                                     ctypes.byref(p), None, 0, None)
    assert rc == _ffi.GSX_ERR_INVALID_ARGUMENT and b"workspace" in lib.gsx_last_error()


def test_the_python_surface_refuses_by_name_without_a_gpu(tmp_path):
    from intro_to_gaussian_splatting_amd import Gaussians, GaussianScene, Trainer
    from intro_to_gaussian_splatting_amd.synthetic import make_scene, write_colmap_text

    sc = make_scene(8, 32, 32, seed=0)
    write_colmap_text(str(tmp_path), sc)
    g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"], device="cpu")
    scene = GaussianScene(str(tmp_path), g)
    for sem in ("ref_cpu", "ref_cuda"):
        with pytest.raises(ValueError, match="antialiased=True needs semantics='std_3dgs'"):
            scene.render_image_hip(1, semantics=sem, antialiased=True)
    with pytest.raises(ValueError, match="antialiased=True needs semantics='std_3dgs'"):
        scene.render_contribution_hip(1, antialiased=True)
    with pytest.raises(ValueError, match="antialiased=True.*camera_gradients"):
        scene.render_image_hip(1, semantics="std_3dgs", antialiased=True, camera_gradients=True)
    with pytest.raises(ValueError, match="antialiased=True.*screen_statistics='abs'"):
        scene.render_image_hip(1, semantics="std_3dgs", antialiased=True, geometry_gradients=True, screen_statistics="abs")
    with pytest.raises(ValueError, match="antialiased=True needs semantics='std_3dgs'"):
        scene.capture_frame(1, antialiased=True)
    targets = {1: torch.zeros((32, 32, 3))}
    with pytest.raises(ValueError, match="antialiased=True needs semantics='std_3dgs'"):
        Trainer(scene, targets, antialiased=True)
    for bad in (dict(refine_poses=dict(lr_rotation=1e-3, lr_translation=1e-3)), dict(depth_targets={1: torch.ones((32, 32))}),
                dict(statistic="screen_abs")):
        with pytest.raises(ValueError, match="std_3dgs"):
            Trainer(scene, targets, semantics="std_3dgs", antialiased=True, **bad)
    assert not g.points.requires_grad          # refused before anything was touched
