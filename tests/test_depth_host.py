"""Depth and coverage, host side: the float64 restatement (tests/depth_restatement.py) against central finite differences
of its own float64 forward and against the reference's own autograd (tests/golden/depthgrad_*.npz); the reference's D and
A; the C ABI by name; the depth carve under ASan / UBSan; depth_loss and the Trainer's arguments.

E_REF: the worst per-Gaussian scaled error (geometry_backward_restatement.per_gaussian_error) of the REFERENCE'S OWN
float32 autograd of L = sum frame W + sum D W_D + sum A W_A against the float64 restatement over all depthgrad_ fixtures,
per output, measured on the CPU:
    points       1.537e-08  (tiny_48x48_n600)
    scales       3.607e-08  (tiny_48x48_n600)
    quaternions  4.223e-09  (tiny_48x48_n600)
    colors       1.942e-07  (tiny_48x48_n600)
    opacity      4.861e-08  (tiny_48x48_n600)
All five are set by tiny_48x48_n600, whose 551 floored footprints of ~0.1 px put most of a Gaussian's weight on one or two
pixels.  The max-normalised errors of the same data are 2e-8 .. 6e-6.
The unit is the Gaussian's own error scale (the sums run on absolute values: depth_restatement's module doc), which
over-counts what float32 loses, so the geometry outputs sit below float32's unit roundoff.  The kernel is held to
12 E_REF against the restatement and 13 E_REF against the fixtures (tests/test_hip_depth.py), the project's ratio.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_preprocessed, load_golden, oracle_camera

import depth_restatement as dr
import geometry_backward_restatement as gbr
from test_geometry_backward_host import fixture_inputs, forward_fixture

DEPTH_SCENES = ["tile2_40x32_n80", "tiny_48x48_n600", "small_64x48_n300", "cull_96x80_n400", "rows1_48x48_n1",
                "rows3_48x48_n3", "tile20_64x64_n300",
                # beyond the required set: one and three visible rows among 500 (culled rows around a small row class)
                "rows1_48x48_n500", "rows3_48x48_n500"]
E_REF = {"points": 1.537e-8, "scales": 3.607e-8, "quaternions": 4.223e-9, "colors": 1.942e-7, "opacity": 4.861e-8}
BOUND_RESTATEMENT = {k: 12 * v for k, v in E_REF.items()}
BOUND_FIXTURE = {k: 13 * v for k, v in E_REF.items()}
E_REF_SLACK = 1.001         # the reference against the restatement is E_REF by definition; the last printed digit is the slack
_CACHE = {}


def depth_fixture(name):
    """(depthgrad_ fixture, the arrays with the scene's inputs, W and image, the arrays with the reference's stage 1)."""
    gg, base = fixture_inputs(name)
    return load_golden("depthgrad_" + name), base, forward_fixture(name)


def fixture_images(dg, base):
    """(frame, dL/dframe, depth image (W,H,2), dL/d(depth image)) of a fixture, float32 as the reference left them."""
    return (base["image"], base["W"], np.stack([dg["D"], dg["A"]], -1).astype(np.float32),
            np.stack([dg["W_D"], dg["W_A"]], -1).astype(np.float32))


def restate(name):
    """The restatement's five gradients and five scales for a fixture's scene and weights (computed once per session)."""
    if name not in _CACHE:
        dg, base, fwd = depth_fixture(name)
        frame, gf, depth, gd = fixture_images(dg, base)
        _CACHE[name] = dr.depth_backward(golden_preprocessed(fwd), base["points"], base["scales"], base["quaternions"],
                                         oracle_camera(fwd), frame, gf, depth, gd, int(base["width"]), int(base["height"]),
                                         int(base["tile"]), with_scale=True)
    return _CACHE[name]


@pytest.mark.parametrize("name", DEPTH_SCENES)
def test_restatement_matches_reference_autograd_per_gaussian(name):
    dg, base, fwd = depth_fixture(name)
    out = restate(name)
    n = base["points"].shape[0]
    refs = [dg["grad_" + k].reshape(n, -1) for k in dr.OUTPUTS]
    errs = dr.per_output_errors(refs, out[:5], out[5:])
    rels = {key: np.abs(refs[k] - out[k]).max() / np.abs(refs[k]).max() for k, key in enumerate(dr.OUTPUTS)}
    for key in dr.OUTPUTS:
        print("%s: %s: reference autograd vs restatement, max error / scale %.4g, max-normalised %.3g" % (name, key, errs[key], rels[key]))
    for k, key in enumerate(dr.OUTPUTS):
        assert np.abs(refs[k]).max() > 0
        assert (np.abs(out[k]) <= out[5 + k][:, None] * (1 + 1e-9)).all(), key      # the scale bounds the gradient itself
        assert errs[key] <= E_REF[key] * E_REF_SLACK, (name, key, errs[key])
    assert np.abs(dg["depth_grad_points"]).max() > 0 and np.abs(dg["depth_grad_opacity"]).max() > 0      # depth's share is in there


@pytest.mark.parametrize("name", DEPTH_SCENES)
def test_restated_depth_and_coverage_match_the_reference_s(name):
    """D and A of the float64 walk against the reference's float32 frame over the colours (z, 1, 0): within float32's
    rounding of a sum of at most a few hundred terms, 1e-5 of A <= 1 and of z_max for D."""
    dg, base, fwd = depth_fixture(name)
    pre = golden_preprocessed(fwd)
    frame, D, A, info = dr.forward(pre, int(base["width"]), int(base["height"]), int(base["tile"]))
    z_listed = info["z_listed"]
    assert np.abs(frame - base["image"]).max() <= 1e-5
    assert 0 < z_listed <= float(dg["z_max"]) and A.max() > 0
    assert np.abs(A - dg["A"]).max() <= 1e-5 and np.abs(D - dg["D"]).max() <= 1e-5 * z_listed
    assert (A <= 1 + 1e-12).all() and (D <= A * z_listed * (1 + 1e-12)).all() and (D >= 0.2 * A * (1 - 1e-12)).all()


def test_fixtures_are_data_of_the_stated_shape_and_size():
    for name in DEPTH_SCENES:
        path = os.path.join(ROOT, "tests", "golden", "depthgrad_%s.npz" % name)
        assert os.path.getsize(path) <= 200 * 1024, path
        dg, base, fwd = depth_fixture(name)
        n, w, h = base["points"].shape[0], int(base["width"]), int(base["height"])
        for key in ("D", "A", "W_D", "W_A"):
            assert dg[key].shape == (w, h) and dg[key].dtype == np.float32, key
        for key, k in (("points", 3), ("scales", 3), ("quaternions", 4), ("colors", 3), ("opacity", 1)):
            assert dg["grad_" + key].reshape(n, -1).shape == (n, k), key
        # the frame's share is the committed geometry fixture's: the total minus depth's share, to the rounding of one add
        gg = load_golden("geomgrad_" + name)
        for key in ("points", "scales", "quaternions"):
            assert np.array_equal(dg["grad_" + key], gg["grad_" + key] + dg["depth_grad_" + key]), key
        assert np.array_equal(dg["grad_colors"], base["grad_colors"])
        # the unrendered last tile row and column hold zeros
        tile = int(base["tile"])
        a, b = len(range(0, w - tile, tile)) * tile, len(range(0, h - tile, tile)) * tile
        assert not dg["D"][a:].any() and not dg["D"][:, b:].any() and not dg["A"][a:].any() and not dg["A"][:, b:].any()


# ---- finite differences of the restatement's own float64 forward
FD_H = 5e-5                 # relative to the coordinate's natural size (below)
FD_TOL = 1e-7               # of the row's largest entry
FD_GAUSSIANS = 6


def _theta_forward(pre, theta, cam, w, h, tile, tiles=None):
    """(frame, D, A) in float64 from a float64 stage 1 of `theta` (points, scales, quaternions, opacity logits, original
    row order) over pre's FIXED tile lists, depth order and float32 stop decisions: the function depth_restatement
    differentiates, smooth in theta."""
    order = np.asarray(pre.order, np.int64)
    st = gbr.stage1(theta["points"][order], theta["scales"][order], theta["quaternions"][order], cam)
    s = 1.0 / (1.0 + np.exp(-theta["opacity"][order].reshape(-1)))
    ops = 1.0 / (1.0 + np.exp(-s))
    frame, D, A, _ = dr.forward(pre, w, h, tile, z=st["t"][:, 2], tiles=tiles, means=st["xy"], conics=st["Q"], ops=ops)
    return st, s, ops, frame, D, A


def test_restatement_matches_central_differences_of_its_float64_forward():
    central_differences("tile2_40x32_n80")


def central_differences(name):
    """Every coordinate of FD_GAUSSIANS Gaussians -- 3 of the point, 3 scales, 4 of the quaternion, the opacity logit --
    perturbed by +-h: the central difference of L = <W, frame> + <W_D, D> + <W_A, A> against the restatement's gradient,
    to FD_TOL of the row's largest entry.  Lists, order and stop decisions are held at the unperturbed float32 values, so
    nothing can flip and no coordinate is dropped.  The difference is taken over the tiles that list the Gaussian (the
    others cancel exactly), which keeps the rounding of L itself out of it."""
    from oracle import cpu_ref

    dg, base, fwd = depth_fixture(name)
    pre, cam = golden_preprocessed(fwd), oracle_camera(fwd)
    w, h, tile = int(base["width"]), int(base["height"]), int(base["tile"])
    n = base["points"].shape[0]
    _, gf, _, gd = fixture_images(dg, base)
    gf, gd = gf.astype(np.float64), gd.astype(np.float64)
    theta = {"points": base["points"].astype(np.float64), "scales": base["scales"].astype(np.float64),
             "quaternions": base["quaternions"].astype(np.float64), "opacity": base["opacity"].astype(np.float64).reshape(n, 1)}

    origins = [(x0, y0) for x0 in cpu_ref.tile_origins(w, tile) for y0 in cpu_ref.tile_origins(h, tile)]
    lists = {o: cpu_ref.tile_list(pre, o[0], o[1], tile) for o in origins}
    rank = {int(r): k for k, r in enumerate(np.asarray(pre.order))}

    def loss(t, tiles):
        _, _, _, frame, D, A = _theta_forward(pre, t, cam, w, h, tile, tiles)
        return float((frame * gf).sum() + (D * gd[..., 0]).sum() + (A * gd[..., 1]).sum())

    st, s, ops, frame, D, A = _theta_forward(pre, theta, cam, w, h, tile)
    sm = dr.sums(pre, frame, gf, np.stack([D, A], -1), gd, w, h, tile, z=st["t"][:, 2], means=st["xy"], conics=st["Q"], ops=ops)
    grads = dict(zip(dr.OUTPUTS, dr.finish(pre, sm, st, st["Q"], n, sig=s, ops=ops)))
    assert np.abs(sm["Sz"]).max() > 0.1
    rows = np.asarray(pre.order)[np.argsort(-(np.abs(sm["S"]).sum(1) + np.abs(sm["Sz"])))[:FD_GAUSSIANS]]
    tried, worst = 0, 0.0
    for key in ("points", "scales", "quaternions", "opacity"):
        for row in rows:
            tiles = [o for o in origins if rank[int(row)] in lists[o]]
            for j in range(theta[key].shape[1]):
                hh = FD_H * (abs(theta[key][row, j]) if key == "scales" else 1.0)
                Ls = []
                for sign in (1, -1):
                    t = {k: v.copy() for k, v in theta.items()}
                    t[key][row, j] += sign * hh
                    Ls.append(loss(t, tiles))
                fd = (Ls[0] - Ls[1]) / (2 * hh)
                g = grads[key][row, j]
                scale = np.abs(grads[key][row]).max()
                tried += 1
                worst = max(worst, abs(fd - g) / scale)
                assert abs(fd - g) <= FD_TOL * scale, (key, int(row), j, fd, g)
    print("%s: finite differences: %d coordinates, none dropped, worst |fd - grad| / max|grad row| = %.3g" % (name, tried, worst))
    assert tried == FD_GAUSSIANS * 11


# ---- C ABI and host arithmetic
def test_header_declares_and_ffi_binds_the_depth_entries():
    from intro_to_gaussian_splatting_amd import _ffi
    import test_cabi

    hdr = open(os.path.join(ROOT, "include", "gsx.h")).read()
    declared = test_cabi._declared_functions()
    for name in ("gsx_render_depth", "gsx_render_backward_depth", "gsx_depth_workspace_bytes", "gsx_backward_depth_workspace_bytes"):
        assert re.search(r"GSX_API\s+\w+\s+%s\(" % name, hdr) and name in declared, name
        assert name in _ffi.SIGNATURES, name
    sig = _ffi.SIGNATURES
    # the screen entry's arguments plus the depth image and dL/ddepth; the forward: the frame entry's without the stats
    assert len(sig["gsx_render_backward_depth"][1]) == len(sig["gsx_render_backward_screen"][1]) + 2 == 23
    assert len(sig["gsx_render_depth"][1]) == len(sig["gsx_render_forward"][1]) - 1 == 13
    assert sig["gsx_depth_workspace_bytes"] == sig["gsx_backward_depth_workspace_bytes"] == sig["gsx_backward_geometry_workspace_bytes"]
    # the existing signatures are as they were
    assert [len(sig[k][1]) for k in ("gsx_render_backward", "gsx_render_backward_geometry", "gsx_render_backward_screen",
                                     "gsx_render_backward_camera")] == [16, 19, 21, 23]
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    assert "D is not divided by A" in flat and "grad_means3d += Sz world2view[0:3][2]" in flat


def test_depth_workspace_is_the_geometry_workspace_plus_a_float_per_row():
    from intro_to_gaussian_splatting_amd import _ffi

    lib = _ffi.load()
    for n, cap in ((0, 1), (1, 100), (63, 5000), (64, 5000), (65, 5000), (100000, 3000000)):
        geo = lib.gsx_backward_geometry_workspace_bytes(n, 640, 480, 16, cap)
        for fn in (lib.gsx_depth_workspace_bytes, lib.gsx_backward_depth_workspace_bytes):
            assert geo > 0 and fn(n, 640, 480, 16, cap) == geo + (max(n, 1) * 4 + 255) // 256 * 256, (n, cap)
    for fn in (lib.gsx_depth_workspace_bytes, lib.gsx_backward_depth_workspace_bytes):
        assert fn(-1, 640, 480, 16, 1) == 0 and fn(10, 0, 480, 16, 1) == 0 and fn(10, 640, 480, 0, 1) == 0
        assert fn(10, 640, 480, 16, -1) == 0 and fn(2 ** 31, 640, 480, 16, 1) == 0


def test_refusals_name_the_argument_and_need_no_gpu():
    """Every refusal returns before any HIP call: these run on a machine without a GPU, on pointers that are never read."""
    import ctypes

    from intro_to_gaussian_splatting_amd import _ffi
    from test_density_host import PTR, WS

    lib = _ffi.load()

    def camera(w=64, h=48):
        cam = _ffi.GsxCamera()
        cam.width, cam.height = w, h
        return cam

    def params(**kw):
        p = _ffi.default_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def forward(cam=None, no_camera=False, ins=(PTR,) * 5, n=10, tile=16, out=PTR, p=None, ws=WS, ws_bytes=1 << 20):
        cam = camera() if cam is None else cam
        return lib.gsx_render_depth(None if no_camera else ctypes.byref(cam), *ins, n, tile, out,
                                    None if p is None else ctypes.byref(p), ws, ws_bytes, None)

    def backward(cam=None, no_camera=False, ins=(PTR,) * 5, n=10, tile=16, image=PTR, grad_image=PTR, outs=(PTR,) * 7, depth=PTR,
                 grad_depth=PTR, p=None, ws=WS, ws_bytes=1 << 20):
        cam = camera() if cam is None else cam
        return lib.gsx_render_backward_depth(None if no_camera else ctypes.byref(cam), *ins, n, tile, image, grad_image, *outs,
                                             depth, grad_depth, None if p is None else ctypes.byref(p), ws, ws_bytes, None)

    shared = ((dict(no_camera=True), b"camera is NULL"), (dict(cam=camera(0, 48)), b"is not positive"), (dict(tile=0), b"tile size 0"),
              (dict(n=-1), b"n = -1"), (dict(n=2 ** 31), b"n = "), (dict(ins=(PTR, None, PTR, PTR, PTR)), b"an input array is NULL"),
              (dict(ins=(PTR,) * 4 + (None,)), b"an input array is NULL"), (dict(ws=None), b"workspace is NULL"),
              (dict(ws=WS + 128), b"256-byte aligned"),
              (dict(p=params(semantics=_ffi.GSX_SEM_STD_3DGS)), b"GSX_SEM_REF_CPU only"),
              (dict(p=params(semantics=_ffi.GSX_SEM_REF_CUDA)), b"GSX_SEM_REF_CPU only"),
              (dict(p=params(sh=PTR, sh_degree=1)), b"not GsxParams.sh"),
              (dict(p=params(tile_x0=1)), b"no tile window"), (dict(p=params(out_w=128, out_h=48)), b"no output window"),
              (dict(p=params(flags=_ffi.GSX_FLAG_NO_SYNC)), b"no GSX_FLAG_NO_SYNC"),
              (dict(p=params(camera_device=PTR)), b"no camera_device"))
    for fn, entry in ((forward, b"gsx_render_depth"), (backward, b"gsx_render_backward")):
        for kw, word in shared:
            assert fn(**kw) == _ffi.GSX_ERR_INVALID_ARGUMENT, (entry, kw)
            assert word in lib.gsx_last_error(), (entry, kw, lib.gsx_last_error())
        assert fn(ws_bytes=256) == _ffi.GSX_ERR_WORKSPACE_TOO_SMALL
        assert fn(p=params(flags=_ffi.GSX_FLAG_NO_SYNC)) and entry in lib.gsx_last_error()
    assert forward(out=None) == _ffi.GSX_ERR_INVALID_ARGUMENT and b"depth_out is NULL" in lib.gsx_last_error()
    for kw, word in ((dict(depth=None), b"depth / grad_depth is NULL"), (dict(grad_depth=None), b"depth / grad_depth is NULL"),
                     (dict(outs=(PTR, PTR, None) + (PTR,) * 4), b"grad_means3d"), (dict(outs=(PTR,) * 4 + (None, PTR, PTR)), b"grad_quats"),
                     (dict(outs=(None,) + (PTR,) * 6), b"grad_colors"), (dict(grad_image=None), b"grad_image"),
                     (dict(image=None), b"out_image is NULL")):
        assert backward(**kw) == _ffi.GSX_ERR_INVALID_ARGUMENT, kw
        assert word in lib.gsx_last_error(), (kw, lib.gsx_last_error())
    # the two screen outputs may be NULL: the next check, the workspace, speaks
    assert backward(outs=(PTR,) * 5 + (None, None), ws_bytes=256) == _ffi.GSX_ERR_WORKSPACE_TOO_SMALL


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_depth_carve_under_asan_and_ubsan(tmp_path):
    """A stand-alone host program (its own main) over csrc/gsx_plan.h: the fifth carve mode's invariants."""
    exe = str(tmp_path / "plan_depth_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "intro_to_gaussian_splatting_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "plan_depth_sanitize.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.startswith("ok:")


# ---- depth_loss and the Python surface, as far as they go without a GPU
def test_depth_loss_is_the_masked_mean_and_stays_connected():
    import torch

    from intro_to_gaussian_splatting_amd import depth_loss

    gen = torch.Generator().manual_seed(3)
    depth = torch.rand((7, 5, 2), generator=gen, dtype=torch.float64).requires_grad_(True)
    target = torch.rand((7, 5), generator=gen, dtype=torch.float64) * 4
    target[2] = 0.0
    target[0, 1], target[6, 4] = -1.0, float("nan")
    for region in (None, (6, 4), (1, 1)):
        a, b = (7, 5) if region is None else region
        valid = [(x, y) for x in range(a) for y in range(b) if target[x, y] > 0]
        d = depth.detach()
        want = sum(abs(float(d[x, y, 0]) - float(d[x, y, 1]) * float(target[x, y])) for x, y in valid) / max(len(valid), 1)
        got = depth_loss(depth, target, region)
        assert got.dim() == 0 and abs(float(got) - want) <= 1e-14 * max(want, 1)
    # linear in both maps: dL/dD = sign / count, dL/dA = -sign t / count on the valid pixels, exact zeros elsewhere
    depth.grad = None
    depth_loss(depth, target).backward()
    valid = target > 0
    count = int(valid.sum())
    sign = torch.sign(depth[..., 0] - depth[..., 1] * torch.where(valid, target, torch.zeros_like(target))).detach()
    assert torch.equal(depth.grad[..., 0], torch.where(valid, sign / count, torch.zeros_like(sign)))
    assert torch.allclose(depth.grad[..., 1], torch.where(valid, -sign * target / count, torch.zeros_like(sign)), rtol=1e-15, atol=0)
    assert not depth.grad[2].any() and not depth.grad[6, 4].any() and torch.isfinite(depth.grad).all()
    # no valid pixel: a zero that is still connected to depth, with zero gradient
    depth.grad = None
    zero = depth_loss(depth, torch.zeros((7, 5), dtype=torch.float64))
    assert float(zero) == 0.0 and zero.grad_fn is not None
    zero.backward()
    assert depth.grad is not None and not depth.grad.any()
    for bad, match in (((depth[..., 0], target), "must be an .A, B, 2. tensor"), ((depth, target[:6]), "target must be an"),
                       ((depth, target, (8, 5)), "does not fit"), ((depth, target, (0, 5)), "does not fit"),
                       ((depth, target.clone().requires_grad_(True)), "target requires grad")):
        with pytest.raises(ValueError, match=match):
            depth_loss(*bad)


def test_python_surface_and_trainer_arguments(tmp_path):
    import inspect

    import torch

    from intro_to_gaussian_splatting_amd import Gaussians, GaussianScene, Trainer
    from intro_to_gaussian_splatting_amd.synthetic import make_scene, write_colmap_text

    p = inspect.signature(GaussianScene.render_image_depth_hip).parameters
    assert list(p) == ["self", "image_idx", "tile_size", "layout", "screen_statistics", "stats"]
    assert p["tile_size"].default == 16 and p["layout"].default == "wh3" and p["screen_statistics"].default is False
    t = inspect.signature(Trainer.__init__).parameters
    assert t["depth_targets"].default is None and t["lambda_depth"].default == 0.0

    sc = make_scene(8, 32, 32, seed=0)
    write_colmap_text(str(tmp_path), sc)
    g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"], device="cpu")
    scene = GaussianScene(str(tmp_path), g)
    with pytest.raises(ValueError, match="layout must be"):
        scene.render_image_depth_hip(1, layout="chw")
    scene.images[1].world2view.requires_grad_(True)
    with pytest.raises(ValueError, match="no pose gradient.*world2view of image 1 requires grad"):
        scene.render_image_depth_hip(1)
    scene.images[1].world2view.requires_grad_(False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):         # past the new checks: the old one
        scene.render_image_depth_hip(1)

    targets = {1: torch.zeros((32, 32, 3))}
    depth = {1: torch.ones((32, 32))}
    for kw, match in ((dict(lambda_depth=0.5), "lambda_depth = 0.5 without depth_targets"),
                      (dict(depth_targets=depth, lambda_depth=-1.0), "lambda_depth = -1.0 is not"),
                      (dict(depth_targets=depth, lambda_depth=float("nan")), "lambda_depth = nan is not"),
                      (dict(depth_targets={2: depth[1]}, lambda_depth=1.0), "depth_targets names image 2"),
                      (dict(depth_targets={1: torch.ones((32, 31))}, lambda_depth=1.0), r"float32 tensor of shape \(32, 32\)"),
                      (dict(depth_targets={1: torch.ones((32, 32), dtype=torch.float64)}, lambda_depth=1.0), "float32 tensor"),
                      (dict(depth_targets={1: [1.0]}, lambda_depth=1.0), "got list"),
                      (dict(depth_targets={1: torch.ones((32, 32), device="meta")}, lambda_depth=1.0), "is on meta, the scene's Gaussians on cpu"),
                      (dict(depth_targets=depth, lambda_depth=1.0, refine_poses=dict(lr_rotation=1e-3, lr_translation=1e-3)),
                       "cannot be combined with refine_poses")):
        with pytest.raises(ValueError, match=match):
            Trainer(scene, targets, **kw)
    assert not g.points.requires_grad          # refused before anything was touched
