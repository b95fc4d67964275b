"""gsx_photometric_loss_weighted, host side: the closed-form gradients dL/dx and dL/dE of include/gsx.h
(tests/photometric_loss_weighted_restatement.py) against torch's float64 autograd of the forward formula and against
central differences; the C ABI's refusals and its workspace arithmetic (also under AddressSanitizer + UBSan:
tests/host/plan_loss_weighted_sanitize.cpp); the argument checks of the Python surface; ``ExposureRefiner`` on CPU tensors;
the float32 reference error E_REF_W the GPU test's bound is built from.

E_REF_W: torch's own float32 CPU evaluation of the weighted forward formula (x' elementwise in the header's order, F.conv2d
with padding 5 and groups 3, the weighted means) and its autograd, against the float64 restatement, worst over the cases with
a non-zero mask x lambda in {0, 0.2, 1}.  Units: |dloss| / loss for the value, max|d| / max|ref| for dL/dx and for dL/dE.
Measured on the CPU:
    value          9.203e-07  (unaligned_base_none_general, lambda 1)
    grad           2.282e-06  (cropped_45x50_of_48x64_random_offset, lambda 1)
    grad_exposure  3.126e-06  (tile_minus_1_by_tile_plus_1_binary_identity, lambda 1)
The kernels are held to BOUND_W = 12 E_REF_W (tests/test_hip_photometric_loss_weighted.py), the project's multiple.  torch's
convolution sums in an order that depends on the CPU it runs on: the test accepts a factor of 1.5 either way, as
tests/test_photometric_loss_host.py does, and BOUND_W is built from the RECORDED figures.  The all-zero masks are left out
here (every output is an exact zero: asserted as such).

wr.LARGE_CASES (9 .. 289 tiles) do not feed E_REF_W.  The same reference measured on them on the CPU: value at most 1.178e-06
(tiles_289_vector_cropped_random_general, lambda 1), grad 2.403e-06 (tiles_289_scalar_random_general, lambda 1),
grad_exposure 3.399e-07 (tiles_4x4_scalar_binary_general, lambda 1) -- each case is held to E_REF_W x 1.5.
"""
import ctypes
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

import photometric_loss_weighted_restatement as wr
from test_photometric_loss_host import E_REF_WINDOW, FD_ELEMENTS, FD_H, FD_TOL

E_REF_W = {"value": 9.203e-7, "grad": 2.282e-6, "grad_exposure": 3.126e-6}
BOUND_W = {k: 12 * v for k, v in E_REF_W.items()}


def _t(a, dtype):
    return None if a is None else torch.from_numpy(np.asarray(a).astype(dtype))


# ---- the closed form
@pytest.mark.parametrize("name", wr.NONZERO_CASE_IDS)
def test_closed_form_is_float64_autograd_of_the_weighted_forward_formula(name):
    x, y, m, E = wr.cropped_inputs(name)
    for lam in wr.LAMBDAS:
        tx = _t(x, np.float64).requires_grad_(True)
        tE = None if E is None else _t(E, np.float64).requires_grad_(True)
        delta = None
        if E is not None:       # the restatement's x' is the float32 one: hand the difference over as a constant
            affine = x.astype(np.float64) @ E.astype(np.float64)[:, :3].T + E.astype(np.float64)[:, 3]
            delta = torch.from_numpy(wr.apply_exposure(x, E).astype(np.float64) - affine)
            assert float(delta.abs().max()) <= 1e-6
        loss, l1, ssim = wr.torch_loss(tx, _t(y, np.float64), lam, _t(m, np.float64), tE, delta)
        loss.backward()
        ref = wr.forward(x, y, lam, m, E)
        for got, want in zip((loss, l1, ssim), ref):
            assert abs(float(got.detach()) - want) <= 1e-13 * max(1.0, abs(want)), (name, lam)
        g, gE = wr.gradient(x, y, lam, m, E)
        err = wr.rel_max(tx.grad.numpy(), g)
        assert err <= 1e-13, (name, lam, err)
        if E is not None:
            err_e = wr.rel_max(tE.grad.numpy(), gE)
            print("%s lambda %.1f: closed form vs float64 autograd: dL/dx %.3g, dL/dE %.3g" % (name, lam, err, err_e))
            assert err_e <= 1e-13, (name, lam, err_e)


def _forward64(xp, y, lam, m):
    """The weighted value of an x' given in float64 (exactly affine in x and E): what the central differences difference.
    Evaluated in numpy's long double: with a weight the gradient entries are of order 1 / (3 W), and FD_TOL of the largest is
    then no more than what float64 rounding of the two values leaves of their difference at FD_H."""
    import photometric_loss_restatement as plr

    xp, y = np.asarray(xp, np.longdouble), np.asarray(y, np.longdouble)
    m = np.ones(xp.shape[:2], np.longdouble) if m is None else np.asarray(m, np.longdouble)
    lam = plr.lam64(lam)
    _, _, A1, A2, B1, B2 = plr._parts(xp, y)
    n = 3 * m.sum()
    ssim = (m[..., None] * (A1 * A2 / (B1 * B2))).sum() / n
    l1 = (m[..., None] * np.abs(xp - y)).sum() / n
    return (1 - lam) * l1 + lam * (1 - ssim)


@pytest.mark.parametrize("name", wr.NONZERO_CASE_IDS)
def test_closed_form_matches_central_differences(name):
    x32, y32, m, E32 = wr.cropped_inputs(name)
    x, y = x32.astype(np.float64), y32.astype(np.float64)
    E = None if E32 is None else E32.astype(np.float64)
    rs = np.random.RandomState(7)
    xp32 = x32 if E32 is None else wr.apply_exposure(x32, E32)
    # the restatement's x' is the float32 one: the differences are taken around it, x' exactly affine in the step
    delta = 0.0 if E is None else xp32.astype(np.float64) - (x @ E[:, :3].T + E[:, 3])
    for lam in (0.2, 1.0):          # (lambda 0 is |x' - y| alone: piecewise linear, nothing to difference)
        g, gE = wr.gradient(x32, y32, lam, m, E32)
        # a step in x or E moves x' by at most (1.4 + 0.2 + 1) h: skip when any element is that close to the L1 kink
        near_kink = np.abs(xp32.astype(np.float64) - y) <= 6 * FD_H
        for _ in range(min(FD_ELEMENTS, x.size)):
            j = tuple(int(rs.randint(s)) for s in x.shape)
            if near_kink[j[0], j[1]].any():
                continue
            keep = x[j]
            x[j] = keep + FD_H
            lp = _forward64(x if E is None else x @ E[:, :3].T + E[:, 3] + delta, y, lam, m)
            x[j] = keep - FD_H
            lm = _forward64(x if E is None else x @ E[:, :3].T + E[:, 3] + delta, y, lam, m)
            x[j] = keep
            fd = float((lp - lm) / (2 * FD_H))
            assert abs(fd - g[j]) <= FD_TOL * np.abs(g).max(), (name, lam, j, fd, g[j])
        if E is None or near_kink.any():
            continue                # an entry of E moves every pixel: difference it only with no element at the kink
        for i in range(3):
            for k in range(4):
                keep = E[i, k]
                E[i, k] = keep + FD_H
                lp = _forward64(x @ E[:, :3].T + E[:, 3] + delta, y, lam, m)
                E[i, k] = keep - FD_H
                lm = _forward64(x @ E[:, :3].T + E[:, 3] + delta, y, lam, m)
                E[i, k] = keep
                fd = float((lp - lm) / (2 * FD_H))
                assert abs(fd - gE[i, k]) <= FD_TOL * np.abs(gE).max(), (name, lam, (i, k), fd, gE[i, k])


def test_all_ones_weight_and_identity_exposure_are_the_unweighted_loss():
    import photometric_loss_restatement as plr

    x, y = plr.case_inputs("halo_across_a_neighbour")
    ones, eye = np.ones(x.shape[:2], np.float32), np.eye(3, 4, dtype=np.float32)
    for lam in wr.LAMBDAS:
        want, want_g = plr.forward(x, y, lam), plr.gradient(x, y, lam)
        got, (got_g, _) = wr.forward(x, y, lam, ones, eye), wr.gradient(x, y, lam, ones, eye)
        assert np.allclose(got[:3], want, rtol=1e-14, atol=0) and got[3] == x.shape[0] * x.shape[1]
        assert np.abs(got_g - want_g).max() <= 1e-14 * np.abs(want_g).max()


@pytest.mark.parametrize("name", wr.ZERO_CASE_IDS)
def test_all_zero_weight_is_exactly_zero_in_the_restatement(name):
    x, y, m, E = wr.cropped_inputs(name)
    assert not m.any()
    for lam in wr.LAMBDAS:
        g, gE = wr.gradient(x, y, lam, m, E)
        assert wr.forward(x, y, lam, m, E) == (0.0, 0.0, 0.0, 0.0) and not g.any() and (gE is None or not gE.any())


# ---- the float32 reference: torch CPU, forward + autograd
def test_float32_reference_error_is_e_ref_w():
    worst = {k: (0.0, None) for k in E_REF_W}
    for name in wr.NONZERO_CASE_IDS:
        x, y, m, E = wr.cropped_inputs(name)
        for lam in wr.LAMBDAS:
            tx = torch.from_numpy(x).requires_grad_(True)
            tE = None if E is None else torch.from_numpy(E.copy()).requires_grad_(True)
            loss = wr.torch_loss(tx, torch.from_numpy(y), lam, None if m is None else torch.from_numpy(m), tE)[0]
            assert loss.dtype == torch.float32
            loss.backward()
            ref, (ref_g, ref_gE) = wr.forward(x, y, lam, m, E), wr.gradient(x, y, lam, m, E)
            e = wr.errors(loss.detach(), tx.grad.numpy(), None if tE is None else tE.grad.numpy(), ref[0], ref_g, ref_gE)
            print("%s lambda %.1f: float32 torch vs restatement: %s" % (
                name, lam, ", ".join("%s %.4g" % kv for kv in sorted(e.items()))))
            for key, val in e.items():
                if val > worst[key][0]:
                    worst[key] = (val, (name, lam))
    for key, (val, where) in worst.items():
        print("E_REF_W %s = %.4g at %s (recorded %.4g)" % (key, val, where, E_REF_W[key]))
        assert E_REF_W[key] / E_REF_WINDOW <= val <= E_REF_W[key] * E_REF_WINDOW, (key, val)


@pytest.mark.parametrize("name", wr.LARGE_NONZERO_CASE_IDS)
def test_float32_reference_stays_within_the_window_of_e_ref_w_at_the_large_cases(name):
    """wr.LARGE_CASES do not feed E_REF_W; the kernels are held to the same 12 E_REF_W there, so the reference itself has
    to meet E_REF_W x E_REF_WINDOW at them."""
    x, y, m, E = wr.cropped_inputs(name)
    for lam in wr.LAMBDAS:
        tx = torch.from_numpy(x).requires_grad_(True)
        tE = None if E is None else torch.from_numpy(E.copy()).requires_grad_(True)
        loss = wr.torch_loss(tx, torch.from_numpy(y), lam, None if m is None else torch.from_numpy(m), tE)[0]
        assert loss.dtype == torch.float32
        loss.backward()
        ref, (ref_g, ref_gE) = wr.forward(x, y, lam, m, E), wr.gradient(x, y, lam, m, E)
        e = wr.errors(loss.detach(), tx.grad.numpy(), None if tE is None else tE.grad.numpy(), ref[0], ref_g, ref_gE)
        print("%s lambda %.1f: float32 torch vs restatement: %s" % (
            name, lam, ", ".join("%s %.4g" % kv for kv in sorted(e.items()))))
        for key, val in e.items():
            assert val <= E_REF_W[key] * E_REF_WINDOW, (name, lam, key, val, E_REF_W[key])


@pytest.mark.parametrize("name", wr.LARGE_ZERO_CASE_IDS)
def test_all_zero_weight_over_289_tiles_is_exactly_zero_in_the_restatement(name):
    x, y, m, E = wr.cropped_inputs(name)
    assert not m.any()
    g, gE = wr.gradient(x, y, 0.2, m, E)
    assert wr.forward(x, y, 0.2, m, E) == (0.0, 0.0, 0.0, 0.0) and not g.any() and not gE.any()


# ---- C ABI
def test_header_declares_ffi_binds_and_library_exports_the_weighted_loss():
    from intro_to_gaussian_splatting_amd import _ffi

    hdr = open(os.path.join(ROOT, "include", "gsx.h")).read()
    assert re.search(r"GSX_API\s+int\s+gsx_photometric_loss_weighted\(", hdr)
    assert re.search(r"GSX_API\s+size_t\s+gsx_photometric_loss_weighted_workspace_bytes\(", hdr)
    assert len(_ffi.SIGNATURES["gsx_photometric_loss_weighted"][1]) == 17
    assert len(_ffi.SIGNATURES["gsx_photometric_loss_weighted_workspace_bytes"][1]) == 3
    assert len(_ffi.SIGNATURES["gsx_photometric_loss"][1]) == 13 and _ffi.load().gsx_version() == 305
    if shutil.which("nm") is None:
        pytest.skip("needs binutils nm")
    for path in (_ffi.LIB_PATH, _ffi.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT gsx_photometric_loss_weighted\b", out), path
        assert re.search(r"\bT gsx_photometric_loss_weighted_workspace_bytes\b", out), path


def test_refusals_name_the_argument_and_need_no_gpu():
    from intro_to_gaussian_splatting_amd import _ffi

    lib = _ffi.load()
    P = ctypes.c_void_p
    ok = dict(image=P(256), s_image=30, target=P(512), s_target=30, weight=P(1280), s_weight=10, exposure=P(1536), rows=4,
              cols=10, lam=0.2, out=P(768), grad=P(1024), s_grad=30, grad_e=P(1792), ws=P(4096), ws_bytes=1 << 20,
              stream=None)       # the pointers are never dereferenced

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gsx_photometric_loss_weighted(a["image"], a["s_image"], a["target"], a["s_target"], a["weight"],
                                                 a["s_weight"], a["exposure"], a["rows"], a["cols"], a["lam"], a["out"],
                                                 a["grad"], a["s_grad"], a["grad_e"], a["ws"], a["ws_bytes"], a["stream"])

    bad = [(dict(image=None), b"image"), (dict(target=None), b"target"), (dict(out=None), b"loss_out"),
           (dict(ws=None), b"workspace"), (dict(rows=0), b"rows"), (dict(rows=-3), b"rows"), (dict(cols=0), b"cols"),
           (dict(s_image=29), b"image_row_stride"), (dict(s_target=29), b"target_row_stride"),
           (dict(s_grad=29), b"grad_row_stride"), (dict(lam=-0.01), b"lambda_dssim"), (dict(lam=1.01), b"lambda_dssim"),
           (dict(lam=float("nan")), b"lambda_dssim"), (dict(lam=float("inf")), b"lambda_dssim"),
           (dict(ws=P(4097)), b"256-byte aligned"),
           (dict(s_weight=9), b"weight_row_stride"), (dict(s_weight=-1), b"weight_row_stride"),
           (dict(exposure=None), b"grad_exposure"), (dict(grad=None, s_grad=0), b"grad_exposure")]
    for kw, word in bad:
        assert call(**kw) == _ffi.GSX_ERR_INVALID_ARGUMENT, kw
        assert word in lib.gsx_last_error(), (kw, lib.gsx_last_error())
    assert b"without exposure" in (call(exposure=None), lib.gsx_last_error())[1]
    assert b"without grad_image" in (call(grad=None), lib.gsx_last_error())[1]
    # a weight stride counts only when there is a weight, a gradient stride only when there is a gradient: such calls get
    # past the argument checks and are stopped by the workspace size
    f = lib.gsx_photometric_loss_weighted_workspace_bytes
    need_v, need_g = f(4, 10, 0), f(4, 10, 1)
    assert call(weight=None, s_weight=0, ws_bytes=need_g - 1) == _ffi.GSX_ERR_WORKSPACE_TOO_SMALL
    assert b"workspace" in lib.gsx_last_error()
    assert call(grad=None, s_grad=0, grad_e=None, ws_bytes=need_v - 1) == _ffi.GSX_ERR_WORKSPACE_TOO_SMALL
    assert call(ws_bytes=need_v) == _ffi.GSX_ERR_WORKSPACE_TOO_SMALL
    with pytest.raises(_ffi.GsxError):
        _ffi.check(call(rows=0))


def test_workspace_bytes_are_zero_on_invalid_sizes_monotone_and_contain_the_plain_carve():
    from intro_to_gaussian_splatting_amd import _ffi

    lib = _ffi.load()
    f, plain = lib.gsx_photometric_loss_weighted_workspace_bytes, lib.gsx_photometric_loss_workspace_bytes
    for rows, cols in ((0, 5), (5, 0), (-1, 5), (5, -1), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 1 << 20)):
        assert f(rows, cols, 0) == 0 and f(rows, cols, 1) == 0, (rows, cols)
    # one tile: the plain carve, 12 bytes of sums and 16 of scale in 256 each; with a gradient 48 bytes of dL/dE partials
    assert f(1, 1, 0) == plain(1, 1, 0) + 512 and f(1, 1, 1) == plain(1, 1, 1) + 768
    # 1080p: 2040 tiles; 2040 x 12 = 24480 -> 24576, 256, and 2040 x 48 = 97920 -> 98048
    assert f(1904, 1072, 0) == plain(1904, 1072, 0) + 24576 + 256
    assert f(1904, 1072, 1) == plain(1904, 1072, 1) + 24576 + 256 + 98048
    prev = (0, 0)
    for k in (1, 2, 31, 32, 33, 64, 65, 500, 1080, 1920, 4000, 30000):
        v, g = f(k, 2 * k, 0), f(k, 2 * k, 1)
        assert v % 256 == 0 and g % 256 == 0 and 0 < v <= g and v >= prev[0] and g >= prev[1], k
        assert v > plain(k, 2 * k, 0) and g > plain(k, 2 * k, 1)
        prev = (v, g)
    assert f(2 ** 31 - 1, 1, 1) > plain(2 ** 31 - 1, 1, 1)          # a very long strip is a valid region


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_weighted_workspace_arithmetic_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "plan_loss_weighted_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "intro_to_gaussian_splatting_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "plan_loss_weighted_sanitize.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.startswith("ok:")


# ---- Python surface, as far as it goes without a GPU
def test_python_surface_refuses_a_bad_weight_or_exposure_before_anything_else():
    from intro_to_gaussian_splatting_amd import photometric_loss

    x, y = torch.zeros((8, 6, 3)), torch.zeros((8, 6, 3))
    w, e = torch.ones((8, 6)), torch.eye(3, 4)
    with pytest.raises(ValueError, match=r"weight must have shape \(8, 6\)"):
        photometric_loss(x, y, weight=torch.ones((6, 8)))
    with pytest.raises(ValueError, match=r"weight must have shape \(8, 6\)"):
        photometric_loss(x, y, weight=torch.ones((8, 6, 1)))
    with pytest.raises(TypeError, match="weight must be float32"):
        photometric_loss(x, y, weight=w.double())
    with pytest.raises(TypeError, match="weight must be float32"):
        photometric_loss(x, y, weight=w > 0)
    with pytest.raises(TypeError, match="weight must be a torch.Tensor"):
        photometric_loss(x, y, weight=np.ones((8, 6), np.float32))
    with pytest.raises(ValueError, match="weight is on meta, expected cpu"):
        photometric_loss(x, y, weight=torch.ones((8, 6), device="meta"))
    with pytest.raises(ValueError, match="weight must be contiguous"):
        photometric_loss(x, y, weight=torch.ones((6, 8)).t())
    with pytest.raises(ValueError, match="weight requires grad"):
        photometric_loss(x, y, weight=w.clone().requires_grad_(True))
    with pytest.raises(ValueError, match=r"exposure must have shape \(3, 4\)"):
        photometric_loss(x, y, exposure=torch.eye(4, 4))
    with pytest.raises(TypeError, match="exposure must be float32"):
        photometric_loss(x, y, exposure=e.double())
    with pytest.raises(TypeError, match="exposure must be a torch.Tensor"):
        photometric_loss(x, y, exposure=np.eye(3, 4, dtype=np.float32))
    with pytest.raises(ValueError, match="exposure is on meta, expected cpu"):
        photometric_loss(x, y, exposure=torch.eye(3, 4, device="meta"))
    # good ones get as far as the device check: there is no CPU path for the weighted loss either
    with pytest.raises(ValueError, match="frame is on cpu.*no CPU fallback"):
        photometric_loss(x, y, weight=w, exposure=e.requires_grad_(True))


# ---- ExposureRefiner, on CPU tensors
def _cpu_scene(indices):
    return types.SimpleNamespace(images={i: object() for i in indices},
                                 gaussians=types.SimpleNamespace(points=torch.zeros((1, 3))))


def test_exposure_refiner_steps_only_views_with_a_gradient():
    from intro_to_gaussian_splatting_amd import ExposureRefiner

    rates = []

    def lr(step):
        rates.append(step)
        return 0.01 / step

    ref = ExposureRefiner(_cpu_scene([3, 5, 9]), lr=lr)
    assert ref.indices == [3, 5, 9]
    for idx in ref.indices:
        e = ref.exposure(idx)
        assert e.shape == (3, 4) and e.dtype == torch.float32 and e.requires_grad and e.is_leaf
        assert torch.equal(e.detach(), torch.eye(3, 4))
    assert ref.step() == 0
    (ref.exposure(5) * torch.arange(12.0).view(3, 4)).sum().backward()
    before = {i: ref.exposure(i).detach().clone() for i in ref.indices}
    assert ref.step() == 1
    assert ref.exposure(5).grad is None and ref.steps == {3: 0, 5: 1, 9: 0}
    assert torch.equal(ref.exposure(3).detach(), before[3]) and torch.equal(ref.exposure(9).detach(), before[9])
    moved = before[5] - ref.exposure(5).detach()
    assert moved[0, 0] == 0 and torch.allclose(moved.flatten()[1:], torch.full((11,), 0.01), rtol=1e-4)   # Adam's first step: lr sign(g)
    # the second step of view 5 runs at lr(2); the first step of view 9 at lr(1)
    for idx in (5, 9):
        ref.exposure(idx).sum().backward()
    before = {i: ref.exposure(i).detach().clone() for i in ref.indices}
    assert ref.step() == 2 and ref.steps == {3: 0, 5: 2, 9: 1}
    assert torch.allclose(before[9] - ref.exposure(9).detach(), torch.full((3, 4), 0.01), rtol=1e-4)
    assert float((before[5] - ref.exposure(5).detach()).abs().max()) < 0.01
    with pytest.raises(ValueError, match="indices names image 4"):
        ExposureRefiner(_cpu_scene([3]), [4], lr=0.01)
    with pytest.raises(TypeError):
        ExposureRefiner(_cpu_scene([3]))            # lr has no default


def test_exposure_refiner_state_dict_round_trips():
    from intro_to_gaussian_splatting_amd import ExposureRefiner

    def run(ref, rounds):
        for k in range(rounds):
            for idx in ref.indices[:1 + k % 2]:
                (ref.exposure(idx) * torch.arange(1.0, 13.0).view(3, 4) * (k + 1)).sum().backward()
            ref.step()

    a = ExposureRefiner(_cpu_scene([1, 2]), lr=0.02, betas=(0.8, 0.99), eps=1e-6)
    run(a, 3)
    state = a.state_dict()
    kept = {i: state["views"][i]["exposure"].clone() for i in (1, 2)}
    b = ExposureRefiner(_cpu_scene([1, 2]), lr=0.5)
    b.load_state_dict(state)
    assert b.lr == 0.02 and b.betas == (0.8, 0.99) and b.eps == 1e-6 and b.steps == a.steps
    run(a, 4)
    run(b, 4)
    for idx in (1, 2):
        assert torch.equal(a.exposure(idx).detach(), b.exposure(idx).detach())
        assert torch.equal(state["views"][idx]["exposure"], kept[idx])          # the state is a copy, not a view
        assert b.exposure(idx).requires_grad and b.exposure(idx).is_leaf
    with pytest.raises(ValueError, match="the state holds views"):
        ExposureRefiner(_cpu_scene([1]), lr=0.02).load_state_dict(state)


# ---- Trainer and GaussianScene arguments
def test_trainer_and_scene_take_masks_and_exposure_and_refuse_bad_ones(tmp_path):
    import inspect

    from intro_to_gaussian_splatting_amd import Gaussians, GaussianScene, Trainer, photometric_loss
    from intro_to_gaussian_splatting_amd.synthetic import make_scene, write_colmap_text

    for fn in (photometric_loss, GaussianScene.photometric_loss):
        p = inspect.signature(fn).parameters
        assert p["weight"].default is None and p["exposure"].default is None
    t = inspect.signature(Trainer.__init__).parameters
    assert t["masks"].default is None and t["exposure"].default is None

    sc = make_scene(8, 32, 32, seed=0)
    write_colmap_text(str(tmp_path), sc)
    g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"], device="cpu")
    scene = GaussianScene(str(tmp_path), g)
    targets = {1: torch.zeros((32, 32, 3))}
    for kw, match in ((dict(masks={2: torch.ones((32, 32))}), "masks names image 2"),
                      (dict(masks={1: torch.ones((32, 31))}), r"float32 tensor of shape \(32, 32\)"),
                      (dict(masks={1: torch.ones((32, 32), dtype=torch.float64)}), "float32 tensor"),
                      (dict(masks={1: [1.0]}), "got list"),
                      (dict(masks={1: torch.ones((32, 32), device="meta")}), "is on meta, the scene's Gaussians on cpu"),
                      (dict(exposure=dict(betas=(0.9, 0.99))), "exposure needs an lr")):
        with pytest.raises(ValueError, match=match):
            Trainer(scene, targets, **kw)
    assert not g.points.requires_grad          # refused before anything was touched
    with pytest.raises(ValueError, match="frame is on cpu"):      # the scene passes both through to the loss
        scene.photometric_loss(1, targets[1], targets[1], weight=torch.ones((32, 32)), exposure=torch.eye(3, 4))
    with pytest.raises(ValueError, match=r"weight must have shape \(32, 32\)"):
        scene.photometric_loss(1, targets[1], targets[1], weight=torch.ones((16, 16)))
    with pytest.raises(ValueError, match="points is on cpu.*no CPU fallback"):      # good ones get as far as the optimiser
        Trainer(scene, targets, masks={1: torch.ones((32, 32))}, exposure=dict(lr=lambda step: 0.01 / step))
