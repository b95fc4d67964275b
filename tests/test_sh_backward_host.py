"""gsx_sh_backward, host side: the C ABI; the float64 restatement (tests/sh_backward_restatement.py) against central
differences of its own forward; the float32 reference error E_REF the GPU test's bound is built from; the rule that makes
an SH scene differentiable.

E_REF: the reference has no spherical harmonics, so the float32 "reference" is torch's CPU autograd of the same formula
written in torch float32 (elementwise operations in the forward kernel's order, no reductions).  Its worst scaled error
(sh_backward_restatement.scaled_error: |float32 - float64| over the formula evaluated on absolute values) against the
restatement over the seven cases of the kernel test, per output, measured on the CPU:
    sh      6.921e-07  (n 70001, degree 3)
    points  3.838e-07  (n 70001, degree 3)
(a cubic monomial of a float32 direction carries about eight roundings; the worst of 3.4M entries sits near twelve)
The kernel is held to 12 E_REF (tests/test_hip_sh_backward.py), the margin the geometry chain's tests grant: it normalises
by a reciprocal and factors the polynomials differently from torch, a few roundings per term.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import sh_backward_restatement as shr

E_REF = {"sh": 6.921e-7, "points": 3.838e-7}
E_REF_SLACK = 1.001         # the reference against the restatement is E_REF by definition; the last printed digit is the slack
BOUND = {k: 12 * v for k, v in E_REF.items()}


# ---- C ABI
def test_header_declares_ffi_binds_and_library_exports_gsx_sh_backward():
    from intro_to_gaussian_splatting_amd import _ffi

    hdr = open(os.path.join(ROOT, "include", "gsx.h")).read()
    assert re.search(r"GSX_API\s+int\s+gsx_sh_backward\(", hdr)
    assert "gsx_sh_backward" in _ffi.SIGNATURES
    assert len(_ffi.SIGNATURES["gsx_sh_backward"][1]) == 9
    assert re.search(r"#define\s+GSX_VERSION\s+305\b", hdr)
    if shutil.which("nm") is None:
        pytest.skip("needs binutils nm")
    for path in (_ffi.LIB_PATH, _ffi.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT gsx_sh_backward\b", out), path


# ---- the restatement against central differences of its own float64 forward
FD_H = 1e-5
FD_TOL = 1e-7               # of the row's largest entry: truncation is O(h^2) = 1e-10, rounding eps / h = 2e-11
FD_GAUSSIANS = 6
FD_NEAR_ZERO = 1e-3         # a coordinate is skipped only when a channel's pre-clamp value lies this near to 0 ...
FD_SEEDS = {0: 0, 1: 1, 2: 2, 3: 3}      # ... which these seeds keep to at most 1 coordinate in 20 (asserted)


def _loss(points, sh, degree, g):
    return float((shr.colors(points, sh, degree, shr.CENTER) * g).sum())


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_restatement_matches_central_differences(degree):
    rs = np.random.RandomState(FD_SEEDS[degree])
    k = (degree + 1) ** 2
    pts = rs.normal(size=(FD_GAUSSIANS, 3))
    sh = rs.normal(size=(FD_GAUSSIANS, k, 3))
    g = rs.normal(size=(FD_GAUSSIANS, 3))
    pre, mask = shr.forward(pts, sh, degree, shr.CENTER)[:2]
    assert mask.any() and not mask.all() or degree == 0       # both sides of the clamp
    grad_sh, grad_mean, _, _ = shr.backward(pts, sh, degree, shr.CENTER, g)
    near = (np.abs(pre) < FD_NEAR_ZERO).any(1)
    tried = skipped = 0
    worst = 0.0
    for i in range(FD_GAUSSIANS):
        for arr, grad in ((sh, grad_sh), (pts, grad_mean)):
            row_max = np.abs(grad[i]).max()
            for j in np.ndindex(arr[i].shape):
                tried += 1
                if near[i]:
                    skipped += 1
                    continue
                keep = arr[i][j]
                arr[i][j] = keep + FD_H
                lp = _loss(pts, sh, degree, g)
                arr[i][j] = keep - FD_H
                lm = _loss(pts, sh, degree, g)
                arr[i][j] = keep
                fd = (lp - lm) / (2 * FD_H)
                err = abs(fd - grad[i][j])
                if row_max > 0:
                    worst = max(worst, err / row_max)
                assert err <= FD_TOL * row_max, (degree, i, j, fd, grad[i][j])
    print("degree %d: %d coordinates, %d skipped near the clamp, worst |fd - grad| / max|row| = %.3g" % (
        degree, tried, skipped, worst))
    assert tried == FD_GAUSSIANS * (3 * k + 3) and skipped * 20 <= tried
    if degree == 0:
        assert not grad_mean.any()


# ---- the float32 reference: torch CPU autograd of the same formula
def _torch_colors(points, sh, degree, center):
    """The forward in torch float32, elementwise and in the kernel's order of operations (sh::basis_at, sh::pre_clamp)."""
    v = points - center
    dx, dy, dz = v[:, 0], v[:, 1], v[:, 2]
    norm = torch.sqrt(dx * dx + dy * dy + dz * dz)
    x, y, z = dx / norm, dy / norm, dz / norm
    c1, c2, c3 = shr.C1, shr.C2, shr.C3
    Y = [torch.full_like(x, shr.C0)]
    if degree > 0:
        Y += [-c1 * y, c1 * z, -c1 * x]
    if degree > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        Y += [c2[0] * xy, c2[1] * yz, c2[2] * (2.0 * zz - xx - yy), c2[3] * xz, c2[4] * (xx - yy)]
    if degree > 2:
        Y += [c3[0] * y * (3.0 * xx - yy), c3[1] * xy * z, c3[2] * y * (4.0 * zz - xx - yy),
              c3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), c3[4] * x * (4.0 * zz - xx - yy), c3[5] * z * (xx - yy),
              c3[6] * x * (xx - 3.0 * yy)]
    acc = torch.zeros_like(points)
    for k, yk in enumerate(Y):
        acc = acc + yk[:, None] * sh[:, k, :]
    return torch.clamp_min(acc + 0.5, 0.0)


def test_float32_reference_error_is_e_ref():
    worst = {"sh": (0.0, None), "points": (0.0, None)}
    for n, degree, skip in shr.CASES:
        pts, sh, gc = [a[skip:] for a in shr.case_inputs(n, degree, skip)]
        tp = torch.from_numpy(pts).requires_grad_(True)
        ts = torch.from_numpy(sh).requires_grad_(True)
        cols = _torch_colors(tp, ts, degree, torch.from_numpy(shr.CENTER))
        assert cols.dtype == torch.float32
        (cols * torch.from_numpy(gc)).sum().backward()
        pre = shr.forward(pts, sh, degree, shr.CENTER)[0]
        sure = np.abs(pre) >= shr.NEAR_ZERO
        assert np.array_equal((cols.detach().numpy() > 0)[sure], (pre > 0)[sure])
        ref_sh, ref_mean, scale_sh, scale_mean = shr.backward(pts, sh, degree, shr.CENTER, gc)
        got_mean = np.zeros_like(pts) if tp.grad is None else tp.grad.numpy()      # (degree 0: no path to the mean at all)
        e = {"sh": shr.scaled_error(ts.grad.numpy(), ref_sh, scale_sh, keep=sure[:, None, :]),
             "points": shr.scaled_error(got_mean, ref_mean, scale_mean, keep=sure.all(1)[:, None])}
        for key, val in e.items():
            print("n %d degree %d: float32 autograd vs restatement, %s: max error / scale %.4g" % (n, degree, key, val))
            if val > worst[key][0]:
                worst[key] = (val, (n, degree))
    for key, (val, where) in worst.items():
        print("E_REF %s = %.4g at %s" % (key, val, where))
        assert val <= E_REF[key] * E_REF_SLACK, (key, val)
        assert val >= E_REF[key] / E_REF_SLACK, (key, val)        # the recorded figure IS the measured one


def test_case_inputs_clamp_a_fair_share_and_few_sit_on_the_edge():
    for n, degree, skip in shr.CASES:
        if n < 200:
            continue
        pts, sh, gc = [a[skip:] for a in shr.case_inputs(n, degree, skip)]
        pre = shr.forward(pts, sh, degree, shr.CENTER)[0]
        clamped = float((pre <= 0).mean())
        print("n %d degree %d: %.1f %% of channels clamped, %.3f %% within 1e-4 of zero" % (
            n, degree, 100 * clamped, 100 * float((np.abs(pre) < 1e-4).mean())))
        assert 0.03 <= clamped <= 0.5, (n, degree, clamped)
        assert (np.abs(pre) < 1e-4).mean() <= 0.003 and (np.abs(pre) < shr.NEAR_ZERO).mean() <= 0.01


# ---- the rule that makes an SH scene differentiable
def test_sh_scene_is_differentiable_exactly_when_its_coefficients_require_grad():
    from intro_to_gaussian_splatting_amd import Gaussians
    from intro_to_gaussian_splatting_amd.gaussian_scene import _refusals, _wants_grad

    def refused(g, **kw):
        return [what for what, bad in _refusals(g, **kw) if bad]

    g = Gaussians(torch.zeros((4, 3)), torch.zeros((4, 3)), device="cpu")
    g.sh, g.sh_degree = torch.zeros((4, 4, 3)), 1
    assert not _wants_grad(g) and not _wants_grad(g, True)
    g.sh.requires_grad_(True)
    assert _wants_grad(g) and _wants_grad(g, True) and refused(g) == []
    with torch.no_grad():
        assert not _wants_grad(g)
    # every other refusal applies to it unchanged
    assert [w.split("=")[0] for w in refused(g, semantics="std_3dgs", tile_window=(0, 1, 0, 1), out=g.sh, substrips=[0, 1],
                                              no_sync=True, camera_buffer=g.sh)] == \
        ["semantics", "tile_window", "out", "substrips", "no_sync", "camera_buffer"]
    g.sh.requires_grad_(False)
    # colours, opacity or (with geometry gradients) the geometry of an SH scene whose coefficients do not: the call raises
    for name, geometry in (("colors", False), ("opacity", False), ("points", True), ("scales", True), ("quaternions", True)):
        getattr(g, name).requires_grad_(True)
        assert _wants_grad(g, geometry), name
        what = refused(g)
        assert len(what) == 1 and "SH" in what[0] and "gaussians.sh.requires_grad_(True)" in what[0], name
        getattr(g, name).requires_grad_(False)
    g.points.requires_grad_(True)
    assert not _wants_grad(g)           # the geometry alone, without geometry_gradients: the plain path, as always
    g.points.requires_grad_(False)
    # an RGB scene is refused nothing on that account
    g.sh = None
    g.colors.requires_grad_(True)
    assert _wants_grad(g) and refused(g) == []
