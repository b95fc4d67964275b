"""The restatement of the std_3dgs gradients (tests/std3dgs_backward_restatement.py) held to an independent derivation, and
the figures the GPU test (tests/test_hip_std3dgs_backward.py) is held to, measured here on the CPU.

Two derivations that share nothing but the decisions.  `torch_gradients` below writes the GSX_SEM_STD_3DGS forward as a
differentiable torch float64 function -- stage 1 from the steps listed in oracle/std3dgs_ref.py, the compositing with the
float64 walk's decisions frozen as masks (a clamped alpha is the constant 0.99f) -- and lets autograd differentiate
sum(frame * dL/dframe).  The hand-derived restatement, evaluated at the same float64 stage-1 values, must agree to 1e-9 of
each Gaussian's error scale for every array, on every case.

E_REF per output array: the float32 mirror's largest error / scale against the float64 restatement over all cases
(geometry_backward_restatement's norm, per Gaussian).  MEASURED HERE by test_e_ref_is_the_mirrors_own_error, recorded below
and asserted as an upper bound of what is measured, with the last printed digit as slack.  The kernels are held to
BOUND = 12 E_REF, the project's standing margin for a kernel whose summation order differs from the mirror's.

The conditions that make the cases worth running are asserted from the float64 walk: composited clamped pairs, pairs skipped
by each of the two skip rules, pixels stopped on both sides of a 64-record batch seam, a non-zero background reaching F under
a pair that carries gradient, Gaussians with the EWA clamp active, culled rows (zero gradient).  gradient_mask leaves out at
most 1 % of a frame's pixels in every case and nothing is LEFT OUT by the walk.
"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from intro_to_gaussian_splatting_amd import _ffi  # noqa: E402
import rule_set_restatement as rsr  # noqa: E402
import std3dgs_backward_restatement as sbr  # noqa: E402
from intro_to_gaussian_splatting_amd import synthetic  # noqa: E402
from oracle import cpu_ref  # noqa: E402
from test_rule_sets_host import STD_BG, STD_CASES, std_case, std_reference  # noqa: E402

f32 = np.float32
E_REF = {"colors": 6.627e-07, "opacity": 1.593e-08, "moments": 2.874e-08, "points": 1.432e-08, "scales": 6.141e-09,
         "quaternions": 2.835e-10, "means2d": 2.6e-08}      # measured by test_e_ref_is_the_mirrors_own_error
BOUND = {k: 12 * v for k, v in E_REF.items()}
E_REF_SLACK = 1.001
AUTOGRAD_TOL = 1e-9
MAX_MASKED_SHARE = 0.01


def offaxis_scene():
    """Two things no case of STD_CASES has.  (1) Gaussians whose centres lie up to 1.8 frustum half-widths off axis, beyond
    the 1.3 tan(fov/2) clamp of the EWA projection, with footprints large enough to reach into the 48x32 frame: the clamp's
    branch of the chain carries gradient.  (2) One pair-skipping record: a 500 : 0.001 needle at 0.8 rad whose float32
    determinant cancels to a negative number, so its conic is indefinite and the exponent is > 0 on most of the frame --
    the first skip rule, which a positive definite conic can never reach; its opacity (logit -6: 0.0025 < 1/255) makes the
    second rule skip it wherever the first does not, so it composites nowhere, carries no gradient and sits on a tile list
    only under published_rects=True."""
    sc = synthetic.make_scene(150, 48, 32, seed=6, spread=1.8, sigma_scale=3.0, qvec=np.array([1.0, 0, 0, 0]),
                              tvec=np.zeros(3))
    add = dict(points=[[0.1, 0.05, 4.0]], colors_0_255=[[200.0, 100.0, 50.0]], scales=[[500.0, 0.001, 0.001]],
               quaternions=[[np.cos(0.4), 0.0, 0.0, np.sin(0.4)]], opacity=[[-6.0]])
    for key, row in add.items():
        sc[key] = np.concatenate([sc[key], np.asarray(row, f32)], 0).astype(f32)
    return sc


# the issue's cases and one of this file's own
CASES = dict(STD_CASES)
CASES["offaxis_48x32_n151"] = (offaxis_scene, 16, STD_BG)


@functools.lru_cache(maxsize=None)
def case_tuple(name):
    """std_case(name)'s tuple, for this file's own case as well."""
    if name in STD_CASES:
        return std_case(name)
    make, tile, bg = CASES[name]
    return build_tuple(make(), tile, bg)


def build_tuple(sc, tile, bg, cam=None, colors=None):
    """std_case's tuple of any scene dict; cam, colors: the ones to walk in place of cpu_ref.build_camera's and the
    scene's own / 256 (what a scene object hands its kernels, where that rounds differently)."""
    w, h = int(sc["width"]), int(sc["height"])
    cam = cpu_ref.build_camera(sc["qvec"], sc["tvec"], sc["fx"], sc["fy"], w, h) if cam is None else cam
    colors = (sc["colors_0_255"] / f32(256.0)).astype(f32) if colors is None else colors
    return (sc, tile, bg, cam, colors) + std_reference(sc, cam, colors, tile, bg)


@functools.lru_cache(maxsize=None)
def backward_case(name):
    """dict of one case, computed once: the std_case entries by name, the decisions, the gradient mask, dL/dframe (H, W, 3)
    float32, `ref` (float64 restatement at the float32 rows) and `mirror` (float32)."""
    return build_backward(case_tuple(name), c_rows(name))


def build_backward(tup, rows=None):
    """backward_case's dict of any case tuple (rows: its C-port stage-1 rows, where they are at hand)."""
    sc, tile, bg, cam, colors, img, nvis, inst, R, wk = tup
    if rows is None:
        rows = rows_of(tup)
    W, H = int(cam.width), int(cam.height)
    dec = sbr.decide(R, W, H)
    assert (dec.composited == wk.composited).all() and ((dec.stop_position >= 0) == wk.stopped).all()
    mask = sbr.gradient_mask(wk, dec)
    g = sbr.driving_gradient(W, H, mask)
    args = (R, dec, sc["points"], sc["scales"], sc["quaternions"], cam, g, bg)
    ref = sbr.backward(*args, dtype=np.float64)
    mirror = sbr.backward(*args, dtype=np.float32)
    rows = np.asarray(rows, f32)
    return dict(sc=sc, tile=tile, bg=bg, cam=cam, colors=colors, R=R, wk=wk, dec=dec, mask=mask, g=g, ref=ref, mirror=mirror,
                W=W, H=H, n=int(sc["points"].shape[0]), rows=rows, img=img, nvis=nvis, inst=inst)


@functools.lru_cache(maxsize=None)
def c_rows(name):
    """The (n, 8) float32 stage-1 rows of the C port (x, y, A, B, C, radius, depth, opacity; NaN where culled)."""
    return rows_of(case_tuple(name))


def rows_of(tup):
    from oracle import c_oracle
    sc, tile, bg, cam, colors = tup[:5]
    return c_oracle.render_std3dgs(sc["points"], colors, sc["scales"], sc["quaternions"], sc["opacity"], cam, tile=tile,
                                   background=bg, nthreads=8)[3]


# ----------------------------------------------------------------------------- the independent derivation

def torch_gradients(case):
    """autograd of the torch float64 forward: dict of ARRAYS-like entries (moments as dL/dconic and dL/dxy) for the rows of R,
    and the float64 stage-1 values the forward composited with."""
    sc, cam, R, dec = case["sc"], case["cam"], case["R"], case["dec"]
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
    # stage 1, oracle/std3dgs_ref.py's steps
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
    xy.retain_grad()
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
    ca, cb, cd = cov[:, 0, 0] + float(f32(0.3)), cov[:, 0, 1], cov[:, 1, 1] + float(f32(0.3))
    det = ca * cd - cb * cb
    conic = torch.stack([cd / det, -cb / det, ca / det], 1)
    conic.retain_grad()
    op = torch.sigmoid(L[rows])
    col = Cc[rows]
    # stage 2 with the decisions frozen
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
    z = lambda v: np.zeros_like(v.detach().numpy()) if v.grad is None else v.grad.numpy()  # noqa: E731
    values = dict(x=xy[:, 0].detach().numpy(), y=xy[:, 1].detach().numpy(), A=conic[:, 0].detach().numpy(),
                  B=conic[:, 1].detach().numpy(), C=conic[:, 2].detach().numpy(), opacity=op.detach().numpy(),
                  colors=col.detach().numpy())
    return dict(points=z(P), scales=z(S), quaternions=z(Q), opacity=z(L).reshape(-1, 1), colors=z(Cc), ndc=z(ndc), xy=z(xy),
                conic=z(conic), frame=frame.detach().numpy()), values


@pytest.mark.parametrize("name", list(CASES))
def test_the_restatement_agrees_with_autograd_of_an_independent_forward(name):
    agrees_with_autograd(name, backward_case(name))


def agrees_with_autograd(name, case):
    """The check on any case dict of backward_case's shape (tests/test_std3dgs_camera_cases_host.py runs it on its own)."""
    R, rows = case["R"], np.asarray(case["R"].index, np.int64)
    auto, values = torch_gradients(case)
    sc = case["sc"]
    st = sbr.stage1_std(sc["points"][rows], sc["scales"][rows], sc["quaternions"][rows], case["cam"], np.float64)
    # the two stage 1 are one point (so that 1e-9 is about the derivative, not about where it is taken)
    np.testing.assert_allclose(st["xy"], np.stack([values["x"], values["y"]], 1), rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(st["Q"][:, 0, 1], values["B"], rtol=1e-10, atol=1e-14)
    got = sbr.backward(R, case["dec"], sc["points"], sc["scales"], sc["quaternions"], case["cam"], case["g"], case["bg"],
                       dtype=np.float64, values=values, stage1=st)
    np.testing.assert_allclose(got.frame, auto["frame"], rtol=0, atol=1e-12)
    worst = {}
    for key in ("colors", "opacity", "points", "scales", "quaternions"):
        worst[key] = sbr.per_gaussian_error(got.arrays[key], auto[key], got.scales[key])
    n = case["n"]
    ndc = np.zeros((n, 2))
    ndc[rows] = auto["ndc"]
    worst["means2d"] = sbr.per_gaussian_error(got.arrays["means2d"], ndc, got.scales["means2d"])
    # the moments, in the gradients they are the coefficients of: dL/dA = -S3 / 2, dL/dB = -S4, dL/dC = -S5 / 2,
    # dL/dmean = -(A S1 + B S2, B S1 + C S2)
    S, Sa = got.arrays["moments"][rows], got.scales["moments"][rows]
    A, B, C = values["A"], values["B"], values["C"]
    mine = np.stack([-0.5 * S[:, 2], -S[:, 3], -0.5 * S[:, 4], -(A * S[:, 0] + B * S[:, 1]), -(B * S[:, 0] + C * S[:, 1])], 1)
    scale = np.stack([0.5 * Sa[:, 2], Sa[:, 3], 0.5 * Sa[:, 4], np.abs(A) * Sa[:, 0] + np.abs(B) * Sa[:, 1],
                      np.abs(B) * Sa[:, 0] + np.abs(C) * Sa[:, 1]], 1)
    theirs = np.concatenate([auto["conic"], auto["xy"]], 1)
    worst["moments"] = sbr.per_gaussian_error(mine, theirs, scale)
    print("%s: restatement vs autograd, max error / scale: %s" % (name, {k: "%.3g" % v for k, v in worst.items()}))
    for key, e in worst.items():
        assert e <= AUTOGRAD_TOL, (name, key, e)
    # and the gradient is not trivially zero
    assert np.abs(auto["points"]).max() > 0 and np.abs(auto["opacity"]).max() > 0


# ----------------------------------------------------------------------------- E_REF and what the cases must reach

def test_e_ref_is_the_mirrors_own_error():
    worst = {k: (0.0, None) for k in sbr.ARRAYS}
    for name in CASES:
        case = backward_case(name)
        ref, mir = case["ref"], case["mirror"]
        for key in sbr.ARRAYS:
            # the scale bounds the gradient itself
            sc = ref.scales[key]
            sc2 = sc if sc.ndim == 2 else sc[:, None]
            assert (np.abs(ref.arrays[key]) <= sc2 * (1 + 1e-9) + 1e-300).all(), (name, key)
            e = sbr.per_gaussian_error(mir.arrays[key], ref.arrays[key], sc)
            worst[key] = max(worst[key], (e, name))
        print("%s: mirror vs float64, max error / scale: %s" % (
            name, {k: "%.4g" % sbr.per_gaussian_error(mir.arrays[k], ref.arrays[k], ref.scales[k]) for k in sbr.ARRAYS}))
    print("E_REF = {%s}" % ", ".join('"%s": %.4g' % (k, worst[k][0]) for k in sbr.ARRAYS))
    for key, (val, where) in worst.items():
        print("E_REF %s = %.4g at %s (recorded %.4g, kernels held to %.4g)" % (key, val, where, E_REF[key], BOUND[key]))
    for key, (val, where) in worst.items():
        assert E_REF[key] / 1.5 <= val <= E_REF[key] * E_REF_SLACK, (key, val, where)


def test_the_cases_reach_every_branch_of_the_backward():
    clamped = skip_power = skip_alpha = early = late = background = ewa = culled = 0
    for name in CASES:
        case = backward_case(name)
        dec, mask, ref = case["dec"], case["mask"], case["ref"]
        c = p = a = 0
        bg_free = np.zeros(mask.shape, bool)
        for pr in dec.pairs:
            if pr is None:
                continue
            m = mask[pr.s]
            c += int((pr.clamped & m).sum())
            p += int((pr.skip_power & m).sum())
            a += int((pr.skip_alpha & m).sum())
            bg_free[pr.s] |= pr.acc & ~pr.clamped
        stopped = (dec.stop_position >= 0) & mask
        e, l = int((stopped & (dec.stop_position < 64)).sum()), int((stopped & (dec.stop_position >= 64)).sum())
        b = int((bg_free & mask & (dec.T_final * max(case["bg"]) > 1e-3)).sum())
        w = int((ref.clamped_ewa & (ref.scales["points"] > 0)).sum())
        z = int(np.isnan(case["rows"][:, 0]).sum())
        assert not np.abs(ref.arrays["points"][np.isnan(case["rows"][:, 0])]).any()
        print("%s: clamped pairs %d, skipped by power %d / by alpha %d, stops before / after the first seam %d / %d, pixels "
              "whose background reaches a free pair %d, EWA-clamped Gaussians with gradient %d, culled rows %d" % (
                  name, c, p, a, e, l, b, w, z))
        clamped, skip_power, skip_alpha, early, late = clamped + c, skip_power + p, skip_alpha + a, early + e, late + l
        background, ewa, culled = background + b, ewa + w, culled + z
    assert clamped > 0 and skip_power > 0 and skip_alpha > 0 and early > 0 and late > 0
    assert background > 0 and ewa > 0 and culled > 0


@pytest.mark.parametrize("name", list(CASES))
def test_the_gradient_mask_leaves_out_at_most_one_percent(name):
    case = backward_case(name)
    wk, dec, mask = case["wk"], case["dec"], case["mask"]
    clamp_only = int(((dec.clamp_ambiguous > 0) & ~wk.ambiguous).sum())
    print("%s: %d of %d pixels masked (%d by the walk, %d more by the clamp)" % (
        name, int((~mask).sum()), mask.size, int(wk.ambiguous.sum()), clamp_only))
    assert not wk.left_out, wk.left_out
    assert (~mask).sum() <= MAX_MASKED_SHARE * mask.size, (name, int((~mask).sum()))
    assert (case["g"][~mask] == 0).all() and np.abs(case["g"][mask]).min() > 0


# ----------------------------------------------------------------------------- the C ABI's refusals, no GPU

def test_gsx_render_backward_std_refuses_bad_arguments_by_name_without_a_gpu():
    lib = _ffi.load()
    assert lib.gsx_version() == 305
    assert lib.gsx_backward_std_workspace_bytes(-1, 64, 64, 16, 10) == 0
    assert lib.gsx_backward_std_workspace_bytes(1000, 64, 64, 16, 5000) == lib.gsx_backward_geometry_workspace_bytes(1000, 64, 64, 16, 5000) > 0
    cam = _ffi.GsxCamera()
    cam.width, cam.height = 64, 48
    ptr = ctypes.c_void_p(256)      # never dereferenced: every call below is refused before any HIP call

    def call(params, camera=cam, inputs=5, image=ptr, grads=3, geometry=(ptr, ptr, ptr), screen=(None, None), workspace=None):
        return lib.gsx_render_backward_std(None if camera is None else ctypes.byref(camera), *([ptr] * inputs + [None] * (5 - inputs)),
                                           10, 16, image, *([ptr] * grads + [None] * (3 - grads)), *geometry, *screen,
                                           None if params is None else ctypes.byref(params), workspace, 0, None)

    def std():
        p = _ffi.default_params()
        p.semantics = _ffi.GSX_SEM_STD_3DGS
        return p

    def refused(rc, *words):
        msg = lib.gsx_last_error()
        assert rc == _ffi.GSX_ERR_INVALID_ARGUMENT and all(w in msg for w in words), (rc, msg, words)

    refused(call(std(), camera=None), b"camera")
    refused(call(None), b"params")
    refused(call(std(), image=None), b"image")
    refused(call(_ffi.default_params()), b"semantics", b"GSX_SEM_STD_3DGS")
    p = std(); p.semantics = _ffi.GSX_SEM_REF_CUDA
    refused(call(p), b"semantics")
    p = std(); p.sh = 256
    refused(call(p), b"GsxParams.sh")
    p = std(); p.tile_x0, p.tile_x1, p.tile_y0, p.tile_y1 = 1, 2, 0, 1
    refused(call(p), b"tile window")
    p = std(); p.out_x0, p.out_y0, p.out_w, p.out_h = 0, 0, 80, 48
    refused(call(p), b"output window")
    p = std(); p.flags |= _ffi.GSX_FLAG_NO_SYNC
    refused(call(p), b"GSX_FLAG_NO_SYNC")
    p = std(); p.camera_device = 256
    refused(call(p), b"camera_device")
    refused(call(std(), inputs=4), b"input array")
    refused(call(std(), grads=2), b"grad_opacity_logit")
    refused(call(std(), geometry=(ptr, None, ptr)), b"grad_scales", b"all three or none")
    refused(call(std(), screen=(ptr, None)), b"screen_radius", b"both or none")
    refused(call(std(), geometry=(None, None, None), screen=(ptr, ptr)), b"grad_means2d", b"need")
    # everything named is in order: the workspace is looked at last, and still nothing has touched a device
    refused(call(std()), b"workspace")
    refused(call(std(), geometry=(None, None, None)), b"workspace")
    refused(call(std(), screen=(ptr, ptr)), b"workspace")
