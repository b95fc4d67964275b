"""From a COLMAP capture to ``Trainer(scene, targets, masks=...)``: points, rectified cameras, rectified photos.

BUILD EXTENSION -- the reference never reads a photograph.  A capture's cameras are whatever lens model COLMAP estimated
(``SIMPLE_RADIAL`` by default), with a principal point that is not the centre; the renderer draws a centred, undistorted
pinhole (``GaussianImage`` reads ``fx, fy`` and the size, nothing else).  So every photo is resampled once, on the GPU
(gsx_rectify_photo, include/gsx.h), into exactly the pinhole the chosen rule set draws, anti-aliased, with a validity weight
that is the loss's per-pixel mask on the undistortion border.  ``GaussianImage`` itself does not change: it is given the
rectified ``PINHOLE`` camera.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _ffi
from .colmap import Camera, read_camera_file, read_image_file, read_points3D_file
from .gaussians import Gaussians

# COLMAP model name -> (GSX_LENS_* id, number of params); the models gsx_rectify_photo resamples
_LENS = {"SIMPLE_PINHOLE": (_ffi.GSX_LENS_SIMPLE_PINHOLE, 3), "PINHOLE": (_ffi.GSX_LENS_PINHOLE, 4),
         "SIMPLE_RADIAL": (_ffi.GSX_LENS_SIMPLE_RADIAL, 4), "RADIAL": (_ffi.GSX_LENS_RADIAL, 5),
         "OPENCV": (_ffi.GSX_LENS_OPENCV, 8)}


def _focal(camera: Camera) -> Tuple[float, float]:
    """(fx_s, fy_s) of a supported camera; any other model is refused by name."""
    if camera.model not in _LENS:
        raise ValueError("camera %r has model %s: rectification supports %s (fisheye models, FOV and FULL_OPENCV are out of "
                         "scope)" % (camera.id, camera.model, ", ".join(_LENS)))
    params = np.asarray(camera.params, dtype=np.float64).reshape(-1)
    if params.size != _LENS[camera.model][1]:
        raise ValueError("camera %r: %s has %d params, got %d" % (camera.id, camera.model, _LENS[camera.model][1], params.size))
    return (float(params[0]), float(params[0])) if camera.model.startswith("SIMPLE") or camera.model == "RADIAL" \
        else (float(params[0]), float(params[1]))


def gsx_lens(camera: Camera) -> "_ffi.GsxLens":
    """The C-ABI view of a ``colmap.Camera`` (include/gsx.h: GsxLens): COLMAP's params in COLMAP's order, float32."""
    _focal(camera)
    lens = _ffi.GsxLens()
    lens.model, lens.width, lens.height = _LENS[camera.model][0], int(camera.width), int(camera.height)
    for k, v in enumerate(np.asarray(camera.params, dtype=np.float64).reshape(-1)):
        lens.params[k] = float(v)
    return lens


def rectified_camera(camera: Camera, semantics: str = "std_3dgs", width: Optional[int] = None,
                     zoom: float = 1.0) -> Tuple[Camera, "_ffi.GsxPinhole"]:
    """The pinhole a capture's ``camera`` is fitted as, and where its pixels sit in a frame of ``semantics``.

    Returns ``(pinhole, target)``.  ``pinhole`` is a ``colmap.Camera`` of model ``PINHOLE`` and size ``W' x H'`` (``W'`` =
    ``width``, the camera's own by default; ``H' = round(H_s W'/W_s)``), params ``(f'_x, f'_y, W'/2, H'/2)`` with
    ``f' = f_s W'/W_s zoom`` per axis: what ``GaussianImage`` is built from.  ``zoom > 1`` crops (use it to push an
    undistortion border out of the frame), ``zoom < 1`` widens.  ``target`` is the ``GsxPinhole`` of gsx_rectify_photo: that
    SAME camera in output pixel-index coordinates, as the rule set draws it.

    The derivation.  ``GaussianImage`` builds ``tan(fov/2) = W'/(2 f')`` and a symmetric frustum, so a view-space point has
    ``ndc_x = (x/z) / tan(fovX/2) = 2 f'_x (x/z) / W'`` -- the principal point is not read.  From there

      ``std_3dgs`` (oracle/std3dgs_ref.py:91-95)  ``pixel = ((ndc + 1) W' - 1) / 2 = f'_x (x/z) + (W' - 1)/2``:
                   ``fx = f'_x``, ``cx = (W' - 1)/2`` -- a pinhole whose principal point W'/2 is the frame's centre in
                   COLMAP's coordinates (pixel-centre index = coordinate - 1/2);
      ``ref_cpu``  (oracle/cpu_ref.py:349-353)    ``pixel = (ndc + 1)(W' - 1)/2 = f'_x (W' - 1)/W' (x/z) + (W' - 1)/2``:
                   ``fx = f'_x (W' - 1)/W'``, ``cx = (W' - 1)/2`` -- the reference stretches NDC over W' - 1 index steps, so
                   its frame is a slightly shorter focal length around the same centre.

    ``y`` likewise with ``H'`` and ``f'_y``.  Resampling a photo to ``target`` therefore puts every photo pixel where a frame
    of that rule set draws the point it shows.  ``ref_cuda`` is refused: nothing trains under it."""
    if semantics == "ref_cuda":
        raise ValueError("semantics 'ref_cuda' is not supported by rectified_camera: nothing trains under it "
                         "(use 'std_3dgs' or 'ref_cpu')")
    if semantics not in ("std_3dgs", "ref_cpu"):
        raise ValueError("unknown semantics %r (use 'std_3dgs' or 'ref_cpu')" % (semantics,))
    fxs, fys = _focal(camera)
    ws, hs = int(camera.width), int(camera.height)
    if ws < 1 or hs < 1:
        raise ValueError("camera %r has size %d x %d" % (camera.id, ws, hs))
    if not (math.isfinite(zoom) and zoom > 0):
        raise ValueError("zoom = %r is not a positive finite number" % (zoom,))
    w = ws if width is None else int(width)
    if isinstance(width, bool) or w < 1 or (width is not None and w != width):
        raise ValueError("width = %r is not a positive integer" % (width,))
    h = max(1, int(round(hs * w / ws)))
    fx, fy = fxs * w / ws * zoom, fys * w / ws * zoom
    pinhole = Camera(camera.id, "PINHOLE", w, h, np.array([fx, fy, w / 2.0, h / 2.0], dtype=np.float64))
    target = _ffi.GsxPinhole()
    target.width, target.height = w, h
    if semantics == "std_3dgs":
        target.fx, target.fy = fx, fy
    else:
        target.fx, target.fy = fx * (w - 1) / w, fy * (h - 1) / h
    target.cx, target.cy = (w - 1) / 2.0, (h - 1) / 2.0
    if not (target.fx > 0 and target.fy > 0):
        raise ValueError("a %d x %d frame has no extent under %s" % (w, h, semantics))
    return pinhole, target


def pick_samples(camera: Camera, target: "_ffi.GsxPinhole") -> int:
    """``min(8, max(1, ceil(max(fx_s/fx, fy_s/fy))))``: photo pixels per output pixel along the denser axis.  (The target's
    focal lengths are float32: a ratio within 1e-6 above a whole number is that number, not the next.)"""
    fxs, fys = _focal(camera)
    return min(8, max(1, int(math.ceil(max(fxs / float(target.fx), fys / float(target.fy)) - 1e-6))))


def rectify(photo: torch.Tensor, camera: Camera, target: "_ffi.GsxPinhole",
            samples: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``photo`` (uint8 ``(H, W, 3)`` on the GPU, rows contiguous; the row stride may be padded) taken by ``camera``,
    resampled to ``target``: ``(image (W', H', 3), weight (W', H'))`` float32 on the photo's device, in one library call
    (gsx_rectify_photo).  ``image`` is the box-filtered bilinear resampling in 0..1, ``weight`` the fraction of a pixel's
    ``samples x samples`` sub-samples that fell inside the photo and the lens model's field -- 1 inside, 0 on the
    undistortion border, in between on its edge.  ``samples=None`` picks ``pick_samples(camera, target)``."""
    lib = _ffi.load()
    if not torch.is_tensor(photo) or photo.dtype != torch.uint8 or photo.dim() != 3 or photo.shape[2] != 3:
        raise ValueError("photo must be a uint8 tensor of shape (H, W, 3)")
    if photo.device.type != "cuda":
        raise ValueError("photo is on %s: rectify runs only as a HIP kernel on an AMD GPU (torch device 'cuda'); there is no "
                         "CPU fallback" % photo.device)
    if tuple(photo.shape[:2]) != (int(camera.height), int(camera.width)):
        raise ValueError("photo is %d x %d (W x H), camera %r is %d x %d" % (photo.shape[1], photo.shape[0], camera.id,
                                                                             camera.width, camera.height))
    if photo.stride(2) != 1 or photo.stride(1) != 3 or photo.stride(0) < 3 * photo.shape[1]:
        photo = photo.contiguous()
    lens = gsx_lens(camera)
    s = pick_samples(camera, target) if samples is None else int(samples)
    dev = photo.device
    image = torch.empty((int(target.width), int(target.height), 3), dtype=torch.float32, device=dev)
    weight = torch.empty((int(target.width), int(target.height)), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.gsx_rectify_photo(ctypes.c_void_p(photo.data_ptr()), int(photo.stride(0)), ctypes.byref(lens),
                                   ctypes.byref(target), s, ctypes.c_void_p(image.data_ptr()),
                                   ctypes.c_void_p(weight.data_ptr()),
                                   ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _ffi.check(rc)
    return image, weight


def read_photo(path: str) -> np.ndarray:
    """A photo as a uint8 ``(H, W, 3)`` array: ``.npy`` directly, anything else through PIL (imported here; its absence is
    an ImportError that names it)."""
    if path.lower().endswith(".npy"):
        a = np.load(path)
    else:
        try:
            from PIL import Image as _PILImage
        except ImportError as e:
            raise ImportError("read_photo(%r) needs the module PIL (the Pillow package) to decode anything but .npy; it is "
                              "not installed" % (path,)) from e
        with _PILImage.open(path) as im:
            a = np.asarray(im.convert("RGB"))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("%s holds %s of shape %s, not uint8 (H, W, 3)" % (path, a.dtype, a.shape))
    return np.ascontiguousarray(a)


def load_capture(colmap_path: str, images_dir: str, semantics: str = "std_3dgs", width: Optional[int] = None,
                 min_track_length: int = 2, device=None):
    """A COLMAP capture as ``(scene, targets, masks)`` for ``Trainer(scene, targets, masks=masks, semantics=semantics)``.

    ``colmap_path`` holds ``cameras``, ``images`` and ``points3D`` (``.bin`` preferred over ``.txt``), ``images_dir`` the
    photos, found by ``Image.name`` (a missing one is refused by name).  The Gaussians are
    ``Gaussians.from_colmap_points(points, min_track_length)``; every camera becomes its ``rectified_camera(camera,
    semantics, width)`` pinhole, the scene is ``GaussianScene.from_views`` of those, and every photo is ``rectify``-ed to its
    camera's target: ``targets[idx]`` is the ``(W', H', 3)`` image, ``masks[idx]`` its ``(W', H')`` weight -- left out for a
    view whose weight is 1 everywhere (``masks`` may come back empty; pass ``masks or None``).

    What it does NOT do: no ``initialize_scale``, no ``init_sh``, no ``normalize()``.  Those stay the caller's three lines::

        scene, targets, masks = load_capture(model, photos, width=1600)
        scene.gaussians.initialize_scale("published")
        scene.gaussians.init_sh(3)
        scene.normalize()
        trainer = Trainer(scene, targets, masks=masks or None, semantics="std_3dgs")
    """
    from .gaussian_scene import GaussianScene

    cameras, images = read_camera_file(colmap_path), read_image_file(colmap_path)
    gaussians = Gaussians.from_colmap_points(read_points3D_file(colmap_path), min_track_length, device=device)
    if gaussians.device.type != "cuda":
        raise ValueError("load_capture needs a GPU: the photos are rectified by a HIP kernel (device %s)" % gaussians.device)
    paths = {}
    for idx, image in images.items():
        if image.camera_id not in cameras:
            raise ValueError("image %r (%s) names camera %r, which the model does not have" % (idx, image.name, image.camera_id))
        paths[idx] = os.path.join(images_dir, image.name)
        if not os.path.isfile(paths[idx]):
            raise FileNotFoundError("image %r: no photo %s under %s" % (idx, image.name, images_dir))
    rectified = {cid: rectified_camera(cam, semantics, width) for cid, cam in cameras.items()
                 if any(im.camera_id == cid for im in images.values())}
    scene = GaussianScene.from_views({cid: r[0] for cid, r in rectified.items()}, images, gaussians)
    targets: Dict[int, torch.Tensor] = {}
    masks: Dict[int, torch.Tensor] = {}
    for idx, image in images.items():
        photo = torch.from_numpy(read_photo(paths[idx])).to(gaussians.device)
        targets[idx], weight = rectify(photo, cameras[image.camera_id], rectified[image.camera_id][1])
        if not bool((weight == 1.0).all()):
            masks[idx] = weight
    return scene, targets, masks
