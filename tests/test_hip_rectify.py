"""gsx_rectify_photo on the GPU: the kernel against the float64 restatement (tests/rectify_restatement.py) within 12 x the
float32 mirror's own error; the exact identity resampling; stride, NULL weight, margins, determinism; the convention closure
per rule set (a frame of that rule set draws a view-space point on the output pixel whose rectified value is what COLMAP's
camera sees along that point); load_capture end to end into one Trainer step."""
import ctypes
import math
import os
import shutil

import numpy as np
import pytest
import torch

import rectify_restatement as R
from conftest import GOLDEN_DIR
from test_capture_host import BOUND_IMAGE, BOUND_WEIGHT, DELTA

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 4096, -12345.0


def _structs(case):
    from intro_to_gaussian_splatting_amd import _ffi

    lens = _ffi.GsxLens()
    lens.model, (lens.width, lens.height) = R.MODELS[case["model"]], case["size"]
    for k, v in enumerate(case["params"]):
        lens.params[k] = v
    target = _ffi.GsxPinhole()
    target.width, target.height, target.fx, target.fy, target.cx, target.cy = case["target"]
    return lens, target


def _run(case, photo, pad=0, with_weight=True):
    """The C ABI called directly, both outputs carved out of guarded buffers: (image (W', H', 3), weight (W', H') or None)
    as numpy, after asserting that the margins kept the sentinel and that every element inside was written."""
    from intro_to_gaussian_splatting_amd import _ffi

    lib = _ffi.load()
    lens, target = _structs(case)
    h, w = photo.shape[:2]
    stride = 3 * w + pad
    rows = torch.full((h, stride), 0xEE, dtype=torch.uint8, device=DEV)
    rows[:, :3 * w] = torch.from_numpy(photo.reshape(h, 3 * w)).to(DEV)
    tw, th = case["target"][:2]
    wholes = [torch.full((GUARD + tw * th * k + GUARD,), SENTINEL, dtype=torch.float32, device=DEV) for k in (3, 1)]
    image, weight = (whole[GUARD:GUARD + tw * th * k] for whole, k in zip(wholes, (3, 1)))
    with torch.cuda.device(DEV):
        rc = lib.gsx_rectify_photo(ctypes.c_void_p(rows.data_ptr()), stride, ctypes.byref(lens), ctypes.byref(target),
                                   case["samples"], ctypes.c_void_p(image.data_ptr()),
                                   ctypes.c_void_p(weight.data_ptr()) if with_weight else None,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _ffi.check(rc)
    torch.cuda.synchronize()
    for whole, out, written in zip(wholes, (image, weight), (True, with_weight)):
        host = whole.cpu().numpy()
        assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + out.numel():] == SENTINEL).all(), "wrote outside its buffer"
        assert bool((out == SENTINEL).any()) != written, "an output element was not written" if written else "weight_out NULL was written"
    return image.cpu().numpy().reshape(tw, th, 3), weight.cpu().numpy().reshape(tw, th) if with_weight else None


@pytest.fixture(scope="module")
def references():
    """Each case's photo and float64 restatement, computed once and left unchanged."""
    out = {}
    for name, case in R.CASES.items():
        photo = R.photo_of(case)
        out[name] = (photo, R.restate64(case, photo))
    return out


@pytest.mark.parametrize("name", list(R.CASES))
def test_kernel_against_the_restatement(name, references):
    """Every case of the restatement -- each lens model, samples 1, 2, 3 and 8, partial blocks on both axes, an invalid border
    under an off-centre principal point, a barrel lens that folds -- within BOUND = 12 x E_REF of the float64 restatement;
    pixels with a sample within DELTA of a validity edge are left out (at most 2 %) and their weight may differ by those
    samples' share.  The margins around both outputs keep their sentinel (_run)."""
    case = R.CASES[name]
    photo, ref = references[name]
    image, weight = _run(case, photo)
    R.compare(case, image, weight, BOUND_IMAGE, BOUND_WEIGHT, DELTA, ref=ref)
    assert np.all(image[ref["count"] == 0] == 0.0) and not np.signbit(image[ref["count"] == 0]).any()    # exact +0
    assert image.min() >= 0.0 and image.max() <= 1.0 and weight.min() >= 0.0 and weight.max() <= 1.0


def test_identity_resampling_returns_the_photo_bit_for_bit():
    """A pinhole with a power-of-two focal length and a dyadic principal point, one sample per pixel, the target the photo's
    own pinhole in index coordinates (cx - 1/2): every coordinate is exact, so u = i, v = j, the bilinear weights are 0 and
    image_out x 255 is the photo, transposed -- the edge pixels u = 0 and u = W - 1 included, which are valid."""
    case = dict(size=(97, 61), model="PINHOLE", params=(64.0, 128.0, 48.25, 30.75),
                target=(97, 61, 64.0, 128.0, 47.75, 30.25), samples=1, seed=11)
    photo = R.photo_of(case)
    image, weight = _run(case, photo)
    assert np.all(weight == 1.0)
    want = photo.transpose(1, 0, 2).astype(np.float32)
    assert np.array_equal((want / np.float32(255.0)).view(np.uint32), image.view(np.uint32))
    assert np.array_equal(image * np.float32(255.0), want)


def test_padded_stride_null_weight_and_a_second_call_give_the_same_bits(references):
    case = R.CASES["opencv_s2"]
    photo, _ = references["opencv_s2"]
    image, weight = _run(case, photo)
    padded, padded_w = _run(case, photo, pad=37)                    # rows 3 W + 37 bytes apart, junk between them
    alone, none = _run(case, photo, with_weight=False)              # weight_out = NULL: its guarded buffer stays untouched
    again, again_w = _run(case, photo)
    assert none is None
    for other in (padded, alone, again):
        assert np.array_equal(other.view(np.uint32), image.view(np.uint32))
    for other in (padded_w, again_w):
        assert np.array_equal(other.view(np.uint32), weight.view(np.uint32))


def test_python_surface_is_the_same_call(references):
    """capture.rectify: the same bits as the direct call, for a contiguous photo and for a view with a padded row stride."""
    from intro_to_gaussian_splatting_amd import capture, colmap

    case = R.CASES["offcentre_border"]
    photo, _ = references["offcentre_border"]
    want_image, want_weight = _run(case, photo)
    camera = colmap.Camera(1, case["model"], case["size"][0], case["size"][1], np.array(case["params"]))
    _, target = _structs(case)
    dev_photo = torch.from_numpy(photo).to(DEV)
    wide = torch.zeros((photo.shape[0], photo.shape[1] + 5, 3), dtype=torch.uint8, device=DEV)
    wide[:, :photo.shape[1]] = dev_photo
    for p in (dev_photo, wide[:, :photo.shape[1]]):
        image, weight = capture.rectify(p, camera, target, samples=case["samples"])
        assert image.shape == (48, 32, 3) and weight.shape == (48, 32) and image.dtype == weight.dtype == torch.float32
        assert np.array_equal(image.cpu().numpy().view(np.uint32), want_image.view(np.uint32))
        assert np.array_equal(weight.cpu().numpy().view(np.uint32), want_weight.view(np.uint32))
    with pytest.raises(ValueError, match="camera"):
        capture.rectify(dev_photo[:-1], camera, target)


# ---------------------------------------------------------------------------------------------- convention closure
PATTERN = ((0.11, 0.07, 0.3), (0.05, 0.12, 1.1), (0.09, 0.09, 2.0))     # per channel: a, b, phase
AMPLITUDE = 110.0


def _pattern(X, Y):
    """(..., 3) in 0..255 at COLMAP image coordinates (X, Y): 127.5 + A sin(a X + phase) cos(b Y)."""
    return np.stack([127.5 + AMPLITUDE * np.sin(a * X + ph) * np.cos(b * Y) for a, b, ph in PATTERN], axis=-1)


def _colmap_project(camera, x, y):
    """float64 COLMAP projection of the view-space directions (x, y, 1): image coordinates (X, Y)."""
    fxs, fys, cxs, cys, k1, k2, p1, p2 = R.lens_coefficients(camera.model, camera.params)
    r2 = x * x + y * y
    rho = k1 * r2 + k2 * r2 * r2
    xd = x + x * rho + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y + y * rho + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return fxs * xd + cxs, fys * yd + cys


@pytest.mark.parametrize("semantics", ["ref_cpu", "std_3dgs"])
def test_convention_closure(semantics):
    """For every output index (i, j) of a 40 x 24 target the view-space point P = ((i - cx)/fx, (j - cy)/fy, 1):
    (1) a frame of the rule set draws P on (i, j) to 1e-3 pixel -- ref_cpu: gsx_project_points on the GPU; std_3dgs: stage 1
        of oracle/std3dgs_ref.py on the CPU -- through the GaussianImage of rectified_camera's pinhole;
    (2) rectify, samples = 1, of a photo that holds a smooth analytic pattern returns the pattern at P's float64 COLMAP
        projection.  Tolerance, derived: bilinear interpolation of f on a unit cell errs by at most (max|f_xx| + max|f_yy|)/8
        = A (a^2 + b^2)/8; the photo's bytes are f rounded, 1/2 each, and a convex combination keeps that; the float32
        coordinates (|u| < 256: an ulp of 1.6e-5, a handful of operations) are allowed 1e-4 pixel times the gradient bound
        A (a + b).  All in 0..255 units, divided by 255.
    A resampler that ignored the rule set would miss by (W' - 1)/W' in focal length -- half an output pixel, 2.5 photo pixels,
    at the frame's edge -- and one that dropped COLMAP's 1/2 by half a photo pixel: up to A a / 2 = 6, against 0.9."""
    from intro_to_gaussian_splatting_amd import GaussianImage, capture, colmap
    from oracle import cpu_ref, std3dgs_ref

    camera = colmap.Camera(1, "OPENCV", 200, 120, np.array([151.3, 149.1, 103.7, 57.2, 0.06, -0.01, 0.002, -0.003]))
    pinhole, target = capture.rectified_camera(camera, semantics, width=40, zoom=1.35)
    assert (target.width, target.height) == (40, 24)
    i, j = np.meshgrid(np.arange(40.0), np.arange(24.0), indexing="ij")
    x, y = (i - float(target.cx)) / float(target.fx), (j - float(target.cy)) / float(target.fy)
    points = np.stack([x, y, np.ones_like(x)], axis=-1).reshape(-1, 3).astype(np.float32)
    image = colmap.Image(1, np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3), 1, "a")         # world = view
    gi = GaussianImage(pinhole, image, device=DEV)
    if semantics == "ref_cpu":
        pts = torch.from_numpy(points).to(DEV)
        out, kept = gi.project_point_to_camera_perspective_projection(pts, pts)
        assert out.shape[0] == points.shape[0]
        xy = out[:, :2].cpu().numpy()
    else:
        cam = cpu_ref.Camera(gi.world2view.detach().cpu().numpy(), gi.full_proj_transform.cpu().numpy(),
                             np.float32(gi.tan_fovX.item()), np.float32(gi.tan_fovY.item()), np.float32(gi.f_x.item()),
                             np.float32(gi.f_y.item()), 40, 24)
        n = points.shape[0]
        st = std3dgs_ref.stage1(points, np.full((n, 3), 0.01, np.float32), np.tile(np.float32([1, 0, 0, 0]), (n, 1)),
                                np.zeros(n, np.float32), cam)
        xy = st.xy
    miss = np.abs(xy - np.stack([i.reshape(-1), j.reshape(-1)], axis=1)).max()
    print("%s: the frame draws P within %.2g pixel of its index" % (semantics, miss))
    assert miss <= 1e-3

    yy, xx = np.meshgrid(np.arange(120) + 0.5, np.arange(200) + 0.5, indexing="ij")     # COLMAP: pixel 0's centre is at 1/2
    photo = np.clip(np.rint(_pattern(xx, yy)), 0, 255).astype(np.uint8)
    got, weight = capture.rectify(torch.from_numpy(photo).to(DEV), camera, target, samples=1)
    assert bool((weight == 1.0).all())          # zoom 1.35: the whole frame lies inside the photo
    want = _pattern(*_colmap_project(camera, x, y)) / 255.0
    second = max(AMPLITUDE * (a * a + b * b) / 8.0 for a, b, _ in PATTERN)
    gradient = max(AMPLITUDE * (a + b) for a, b, _ in PATTERN)
    tol = (second + 0.5 + 1e-4 * gradient) / 255.0
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    print("%s: pattern error %.3g, tolerance %.3g" % (semantics, err, tol))
    assert err <= tol
    # the other rule set's target is a different resampling: it misses this tolerance
    other = capture.rectified_camera(camera, "std_3dgs" if semantics == "ref_cpu" else "ref_cpu", width=40, zoom=1.35)[1]
    wrong, _ = capture.rectify(torch.from_numpy(photo).to(DEV), camera, other, samples=1)
    assert np.abs(wrong.cpu().numpy().astype(np.float64) - want).max() > tol


# ---------------------------------------------------------------------------------------------- end to end
def _write_capture(root):
    """The colmap_points model under three views -- PINHOLE (centred, dyadic: every pixel valid under std_3dgs), SIMPLE_RADIAL
    and a pincushion OPENCV whose corners leave the photo -- looking down +z from 4 units back, with .npy photos."""
    model, photos = os.path.join(root, "sparse"), os.path.join(root, "images")
    os.makedirs(model)
    os.makedirs(photos)
    shutil.copy(os.path.join(GOLDEN_DIR, "colmap_points", "bin", "points3D.bin"), os.path.join(model, "points3D.bin"))
    with open(os.path.join(model, "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n")
        f.write("1 PINHOLE 64 48 64.0 64.0 32.0 24.0\n")
        f.write("2 SIMPLE_RADIAL 80 60 71.3 41.2 29.4 -0.08\n")
        f.write("3 OPENCV 96 72 88.1 87.3 47.1 36.8 0.15 0.02 0.001 -0.002\n")
    with open(os.path.join(model, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n")
        for idx, (cam, tx, name) in enumerate(((1, 0.0, "a.npy"), (2, 0.3, "b.npy"), (3, -0.3, "sub/c.npy")), start=1):
            f.write("%d 1.0 0.0 0.0 0.0 %r 0.0 4.0 %d %s\n1.0 2.0 -1\n" % (10 * idx, tx, cam, name))
    os.makedirs(os.path.join(photos, "sub"))
    rs = np.random.default_rng(5)
    for name, (w, h) in (("a.npy", (64, 48)), ("b.npy", (80, 60)), ("sub/c.npy", (96, 72))):
        smooth = rs.uniform(40, 215, (h // 12 + 2, w // 12 + 2, 3)).repeat(12, axis=0).repeat(12, axis=1)[:h, :w]
        np.save(os.path.join(photos, name), smooth.astype(np.uint8))
    return model, photos


@pytest.mark.parametrize("semantics", ["std_3dgs", "ref_cpu"])
def test_load_capture_feeds_a_trainer_step(tmp_path, semantics):
    from intro_to_gaussian_splatting_amd import Trainer, load_capture

    model, photos = _write_capture(str(tmp_path))
    scene, targets, masks = load_capture(model, photos, semantics=semantics, device=DEV)
    assert len(scene.gaussians) == 32 and scene.gaussians.points.device.type == "cuda"
    assert list(scene.images) == list(targets) == [10, 20, 30] and set(masks) <= set(targets)
    for idx, (w, h) in ((10, (64, 48)), (20, (80, 60)), (30, (96, 72))):
        cam = scene.images[idx].gsx_camera()
        assert (cam.width, cam.height) == (w, h) and targets[idx].shape == (w, h, 3) and targets[idx].dtype == torch.float32
        assert bool(torch.isfinite(targets[idx]).all()) and 0.0 <= float(targets[idx].min()) and float(targets[idx].max()) <= 1.0
    assert 30 in masks and masks[30].shape == (96, 72) and float(masks[30].min()) == 0.0 and float(masks[30].max()) == 1.0
    assert float(masks[30][48, 36]) == 1.0 and float(masks[30][0, 0]) == 0.0         # the pincushion's corners leave the photo
    if semantics == "std_3dgs":
        assert 10 not in masks      # the centred pinhole at its own size: every pixel valid, no entry
    else:
        assert 10 in masks          # the reference's frame is wider than the photo by half a pixel a side (W' - 1 steps)
    trainer = Trainer(scene, targets, masks=masks or None, semantics=semantics)
    terms, idx = trainer.step()             # (loss, l1, ssim) on the device
    assert idx in targets and terms.shape == (3,) and all(math.isfinite(v) for v in terms.tolist()) and float(terms[0]) > 0.0
    os.remove(os.path.join(photos, "b.npy"))
    with pytest.raises(FileNotFoundError, match="b.npy"):
        load_capture(model, photos, semantics=semantics, device=DEV)
