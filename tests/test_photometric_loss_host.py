"""gsx_photometric_loss, host side: the closed-form gradient of include/gsx.h (tests/photometric_loss_restatement.py)
against torch's float64 autograd of the forward formula and against central differences; the C ABI's refusals and its
workspace arithmetic (also under AddressSanitizer + UBSan: tests/host/plan_loss_sanitize.cpp); the float32 reference error
E_REF the GPU test's bound is built from.

E_REF: torch's own float32 CPU evaluation of the forward formula (F.conv2d, padding 5, groups 3) and its autograd, against
the float64 restatement, worst over the ten cases of the kernel test x lambda in {0, 0.2, 1}.  Units: |dloss| / loss for
the value, max|dgrad| / max|grad| for the gradient.  Measured on the CPU:
    value  1.110e-06  (cropped_32x48_of_48x64, lambda 1)
    grad   2.228e-06  (cropped_45x50_of_48x64, lambda 1)
The kernels are held to BOUND = 12 E_REF (tests/test_hip_photometric_loss.py), the multiple the SH and geometry tests use:
they filter separably (22 roundings of a pixel's sum where the 121-tap sum has 121 in another order) and form the
quotients in another order than autograd does.  torch's convolution sums in an order that depends on the CPU it runs on, so
the figure a run measures may differ from the recorded one by a few tens of per cent; the test accepts a factor of 1.5
either way and BOUND is built from the RECORDED figure.

plr.LARGE_CASES (9 .. 289 tiles) do not feed E_REF.  The same reference measured on them on the CPU: value at most 5.648e-07
(tiles_3x3_vector, lambda 1), grad at most 2.051e-06 (tiles_289_scalar, lambda 1) -- each case is held to E_REF x 1.5, so
that the kernels' 12 E_REF there is a bound the reference itself keeps with a factor of 8 to spare.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import photometric_loss_restatement as plr

E_REF = {"value": 1.110e-6, "grad": 2.228e-6}
E_REF_WINDOW = 1.5          # measured / recorded and recorded / measured stay below this (docstring)
BOUND = {k: 12 * v for k, v in E_REF.items()}


def _cropped(name):
    _, _, (a, b), _ = plr.case_of(name)
    x, y = plr.case_inputs(name)
    return np.ascontiguousarray(x[:a, :b]), np.ascontiguousarray(y[:a, :b])


# ---- the closed form
@pytest.mark.parametrize("name", plr.CASE_IDS)
def test_closed_form_is_float64_autograd_of_the_forward_formula(name):
    x, y = _cropped(name)
    for lam in plr.LAMBDAS:
        tx = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
        loss, l1, ssim = plr.torch_loss(tx, torch.from_numpy(y.astype(np.float64)), lam)
        loss.backward()
        ref = plr.forward(x, y, lam)
        for got, want in zip((loss, l1, ssim), ref):
            assert abs(float(got.detach()) - want) <= 1e-13 * max(1.0, abs(want)), (name, lam)
        g = plr.gradient(x, y, lam)
        err = np.abs(g - tx.grad.numpy()).max() / np.abs(g).max()
        print("%s lambda %.1f: closed form vs float64 autograd, max|d| / max|grad| = %.3g" % (name, lam, err))
        assert err <= 1e-13, (name, lam, err)


FD_H = 1e-6
FD_TOL = 1e-7       # of the largest gradient entry: truncation O(h^2) = 1e-12 of the third derivative, rounding eps / h = 1e-10
FD_ELEMENTS = 6


@pytest.mark.parametrize("name", plr.CASE_IDS)
def test_closed_form_matches_central_differences(name):
    x, y = [a.astype(np.float64) for a in _cropped(name)]
    rs = np.random.RandomState(7)
    for lam in (0.2, 1.0):          # (lambda 0 is |x - y| alone: piecewise linear, nothing to difference)
        g = plr.gradient(x, y, lam)
        for _ in range(min(FD_ELEMENTS, x.size)):
            j = tuple(int(rs.randint(s)) for s in x.shape)
            if abs(x[j] - y[j]) <= 2 * FD_H:
                continue            # the kink of |x - y|
            keep = x[j]
            x[j] = keep + FD_H
            lp = plr.forward(x, y, lam)[0]
            x[j] = keep - FD_H
            lm = plr.forward(x, y, lam)[0]
            x[j] = keep
            fd = (lp - lm) / (2 * FD_H)
            assert abs(fd - g[j]) <= FD_TOL * np.abs(g).max(), (name, lam, j, fd, g[j])


def test_filter_is_its_own_adjoint_and_sums_to_one_inside():
    rs = np.random.RandomState(3)
    u, v = rs.normal(size=(13, 9, 3)), rs.normal(size=(13, 9, 3))
    assert abs((plr.blur(u) * v).sum() - (u * plr.blur(v)).sum()) <= 1e-12
    assert abs(plr.window().sum() - 1) <= 1e-15
    assert np.allclose(plr.blur(np.ones((30, 30, 3)))[5:-5, 5:-5], 1.0, atol=1e-14)


# ---- the float32 reference: torch CPU, forward + autograd
def test_float32_reference_error_is_e_ref():
    worst = {"value": (0.0, None), "grad": (0.0, None)}
    for name in plr.CASE_IDS:
        x, y = _cropped(name)
        for lam in plr.LAMBDAS:
            tx = torch.from_numpy(x).requires_grad_(True)
            loss = plr.torch_loss(tx, torch.from_numpy(y), lam)[0]
            assert loss.dtype == torch.float32
            loss.backward()
            e = dict(zip(("value", "grad"), plr.errors(loss.detach(), tx.grad.numpy(), plr.forward(x, y, lam)[0],
                                                       plr.gradient(x, y, lam))))
            print("%s lambda %.1f: float32 torch vs restatement: value %.4g, grad %.4g" % (name, lam, e["value"], e["grad"]))
            for key, val in e.items():
                if val > worst[key][0]:
                    worst[key] = (val, (name, lam))
    for key, (val, where) in worst.items():
        print("E_REF %s = %.4g at %s (recorded %.4g)" % (key, val, where, E_REF[key]))
        assert E_REF[key] / E_REF_WINDOW <= val <= E_REF[key] * E_REF_WINDOW, (key, val)


@pytest.mark.parametrize("name", plr.LARGE_CASE_IDS)
def test_float32_reference_stays_within_the_window_of_e_ref_at_the_large_cases(name):
    """plr.LARGE_CASES do not feed E_REF; the kernels are held to the same 12 E_REF there, so the reference itself has to
    meet E_REF x E_REF_WINDOW at them: the bound then is one the reference keeps with a factor of 8 to spare."""
    x, y = _cropped(name)
    worst = {"value": 0.0, "grad": 0.0}
    for lam in plr.LAMBDAS:
        tx = torch.from_numpy(x).requires_grad_(True)
        loss = plr.torch_loss(tx, torch.from_numpy(y), lam)[0]
        assert loss.dtype == torch.float32
        loss.backward()
        e = plr.errors(loss.detach(), tx.grad.numpy(), plr.forward(x, y, lam)[0], plr.gradient(x, y, lam))
        print("%s lambda %.1f: float32 torch vs restatement: value %.4g, grad %.4g" % (name, lam, e[0], e[1]))
        worst = {"value": max(worst["value"], e[0]), "grad": max(worst["grad"], e[1])}
    for key, val in worst.items():
        assert val <= E_REF[key] * E_REF_WINDOW, (name, key, val, E_REF[key])


# ---- C ABI
def test_header_declares_ffi_binds_and_library_exports_the_loss():
    from intro_to_gaussian_splatting_amd import _ffi

    hdr = open(os.path.join(ROOT, "include", "gsx.h")).read()
    assert re.search(r"GSX_API\s+int\s+gsx_photometric_loss\(", hdr)
    assert re.search(r"GSX_API\s+size_t\s+gsx_photometric_loss_workspace_bytes\(", hdr)
    assert len(_ffi.SIGNATURES["gsx_photometric_loss"][1]) == 13
    assert len(_ffi.SIGNATURES["gsx_photometric_loss_workspace_bytes"][1]) == 3
    assert re.search(r"#define\s+GSX_VERSION\s+305\b", hdr) and _ffi.load().gsx_version() == 305
    if shutil.which("nm") is None:
        pytest.skip("needs binutils nm")
    for path in (_ffi.LIB_PATH, _ffi.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT gsx_photometric_loss\b", out) and re.search(r"\bT gsx_photometric_loss_workspace_bytes\b", out), path


def test_refusals_name_the_argument_and_need_no_gpu():
    from intro_to_gaussian_splatting_amd import _ffi

    lib = _ffi.load()
    P = ctypes.c_void_p
    ok = dict(image=P(256), s_image=30, target=P(512), s_target=30, rows=4, cols=10, lam=0.2, out=P(768), grad=P(1024),
              s_grad=30, ws=P(4096), ws_bytes=1 << 20, stream=None)       # the pointers are never dereferenced

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gsx_photometric_loss(a["image"], a["s_image"], a["target"], a["s_target"], a["rows"], a["cols"], a["lam"],
                                        a["out"], a["grad"], a["s_grad"], a["ws"], a["ws_bytes"], a["stream"])

    bad = [(dict(image=None), b"image"), (dict(target=None), b"target"), (dict(out=None), b"loss_out"),
           (dict(ws=None), b"workspace"), (dict(rows=0), b"rows"), (dict(rows=-3), b"rows"), (dict(cols=0), b"cols"),
           (dict(s_image=29), b"image_row_stride"), (dict(s_target=29), b"target_row_stride"),
           (dict(s_grad=29), b"grad_row_stride"), (dict(lam=-0.01), b"lambda_dssim"), (dict(lam=1.01), b"lambda_dssim"),
           (dict(lam=float("nan")), b"lambda_dssim"), (dict(lam=float("inf")), b"lambda_dssim"),
           (dict(ws=P(4097)), b"256-byte aligned")]
    for kw, word in bad:
        assert call(**kw) == _ffi.GSX_ERR_INVALID_ARGUMENT, kw
        assert word in lib.gsx_last_error(), (kw, lib.gsx_last_error())
    # a gradient stride counts only when there is a gradient
    need_v, need_g = lib.gsx_photometric_loss_workspace_bytes(4, 10, 0), lib.gsx_photometric_loss_workspace_bytes(4, 10, 1)
    assert call(grad=None, s_grad=0, ws_bytes=need_v - 1) == _ffi.GSX_ERR_WORKSPACE_TOO_SMALL
    assert b"workspace" in lib.gsx_last_error()
    # the workspace with a gradient is larger: what suffices for the value is refused for both
    assert call(ws_bytes=need_v) == _ffi.GSX_ERR_WORKSPACE_TOO_SMALL and call(ws_bytes=need_g - 1) == _ffi.GSX_ERR_WORKSPACE_TOO_SMALL
    with pytest.raises(_ffi.GsxError):
        _ffi.check(call(rows=0))


def test_workspace_bytes_are_zero_on_invalid_sizes_monotone_and_256_byte_multiples():
    from intro_to_gaussian_splatting_amd import _ffi

    f = _ffi.load().gsx_photometric_loss_workspace_bytes
    for rows, cols in ((0, 5), (5, 0), (-1, 5), (5, -1), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 1 << 20)):
        assert f(rows, cols, 0) == 0 and f(rows, cols, 1) == 0, (rows, cols)
    assert f(1, 1, 0) == 256 and f(1, 1, 1) == 256 + 3 * 256
    # 1080p, the rendered region of a tile-16 wh3 frame: 60 x 34 tiles of 32 x 32; 3 maps of 1904 x (3 x 1072) floats
    assert f(1904, 1072, 0) == 60 * 34 * 8 + 64 and f(1904, 1072, 1) == f(1904, 1072, 0) + 3 * 1904 * 3216 * 4
    prev = (0, 0)
    for k in (1, 2, 31, 32, 33, 64, 65, 500, 1080, 1920, 4000, 30000):
        v, g = f(k, 2 * k, 0), f(k, 2 * k, 1)
        assert v % 256 == 0 and g % 256 == 0 and 0 < v <= g and v >= prev[0] and g >= prev[1], k
        assert g >= v + 3 * k * 6 * k * 4
        prev = (v, g)
    assert f(2 ** 31 - 1, 1, 1) > 3 * 4 * 3 * (2 ** 31 - 1)         # a very long strip is a valid region


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_workspace_arithmetic_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "plan_loss_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "intro_to_gaussian_splatting_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "plan_loss_sanitize.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.startswith("ok:")


# ---- Python surface, as far as it goes without a GPU
def test_python_surface_refuses_cpu_tensors_dtype_shape_target_grad_and_region():
    from intro_to_gaussian_splatting_amd import photometric_loss

    x, y = torch.zeros((8, 6, 3)), torch.zeros((8, 6, 3))
    with pytest.raises(ValueError, match="frame is on cpu.*no CPU fallback"):
        photometric_loss(x, y)
    with pytest.raises(TypeError, match="frame must be float32"):
        photometric_loss(x.double(), y)
    with pytest.raises(ValueError, match=r"frame must have shape \(A, B, 3\)"):
        photometric_loss(torch.zeros((8, 6, 4)), y)
    with pytest.raises(ValueError, match="frame must be contiguous"):
        photometric_loss(torch.zeros((6, 8, 3)).transpose(0, 1), y)
    with pytest.raises(TypeError, match="frame must be a torch.Tensor"):
        photometric_loss(np.zeros((8, 6, 3), np.float32), y)
