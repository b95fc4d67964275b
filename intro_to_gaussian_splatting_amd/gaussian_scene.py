"""``GaussianScene``: the reference's render surface (splat/gaussian_scene.py:25-285) on MI355X.

Host code stays Python and PyTorch-ROCm tensors hold the Gaussian parameters; every stage of
the hot path -- projection, depth ordering, tile binning, compositing -- runs in libgsx.so (HIP,
gfx950) through the C ABI of include/gsx.h.  There is no CPU path in this module: without the
library or without a GPU the render methods raise.

Surface kept from the reference:
  ``GaussianScene(colmap_path, gaussians)``, ``.images[idx]``, ``.gaussians``,
  ``.preprocess(idx) -> PreprocessedScene``            (gaussian_scene.py:70-144)
  ``.render_image(idx, tile_size=16) -> (W,H,3)``      (gaussian_scene.py:200-238, CPU semantics; host tensor)
  ``.render_points_image(idx)``                        (gaussian_scene.py:44-51)
Added: ``.render_image_hip`` (explicit layout / tile window / stats), ``.render_preprocessed``
(the argument list of the reference's native ``render_image``, splat/c/render.cu:90-101).
"""
from __future__ import annotations

import ctypes
from collections import namedtuple
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _ffi, _hip
from ._device import _WORKSPACE, _Lru, _Workspace, _check_f32, _ptr, _require_gpu, _stream_handle  # noqa: F401
from .colmap import read_camera_file, read_image_file
from .gaussians import Gaussians
from .image import GaussianImage
from .loss import photometric_loss
from .schema import PreprocessedScene
from .strips import tiles_along

_PINNED_SLOTS = 256
_PLAIN_MIN_TILES = 16384  # windows from this many tiles take GSX_FLAG_PLAIN_FOOTPRINTS when the view allows it (render_image_hip)
_HINT_VIEWS = 64          # GsxParams.hints buffers a scene keeps (83 KB each at 1080p, 300 KB at 4K): the most recent views
_SEMANTICS = {"ref_cpu": _ffi.GSX_SEM_REF_CPU, "ref_cuda": _ffi.GSX_SEM_REF_CUDA,
              "std_3dgs": _ffi.GSX_SEM_STD_3DGS}


def _frame_stats(pinned: torch.Tensor) -> _ffi.GsxFrameStats:
    """The GsxFrameStats a frame's counts arrive in, as a view of its pinned slot (no copy: read it after a synchronise)."""
    return ctypes.cast(ctypes.c_void_p(pinned.data_ptr()), ctypes.POINTER(_ffi.GsxFrameStats)).contents


@dataclass
class _OwnedFrame:
    """``render_image_hip(_private=...)``: what ONE frame owns instead of taking it from the scene (capture_frame: its graph
    bakes the addresses in, so they must not be shared with or recycled by any other frame).  Such a call neither reads nor
    updates the scene's hints and pending list; a field left at its default comes from the scene as in any other call."""
    cap: Optional[int] = None                   # pair capacity; fixed: a frame that needs more is an error, not a retry
    workspace: Optional[torch.Tensor] = None
    kept: Optional[int] = None                  # GsxParams.kept_hint
    rows_flag: int = 0                          # GSX_FLAG_SMALL_BATCH / _ONE_VISIBLE: an owned call is not issued again
    plain: Optional[bool] = None                # GSX_FLAG_PLAIN_FOOTPRINTS where the call allows it
    pinned: Optional[torch.Tensor] = None       # GsxFrameStats slot of a no_sync frame
    inputs: Optional[list] = None               # receives the tensors whose addresses the call handed to the library
    hints: Optional[list] = None                # [GsxParams.hints buffer, a frame has run with it?]

    @classmethod
    def of(cls, private) -> Optional["_OwnedFrame"]:
        """None and the empty dict: not owned.  A dict: its record (an unknown key is a TypeError).  A record: itself."""
        if private is None or isinstance(private, cls):
            return private
        return cls(**private) if private else None


_UNOWNED = _OwnedFrame()        # every field at its default: all of it from the scene
# a ``no_sync`` frame whose counts are still in flight (GaussianScene._settle).  pinned: the slot its GsxFrameStats arrive
# in; ran_plain: issued with GSX_FLAG_PLAIN_FOOTPRINTS; call: render_image_hip(**call) renders it again, synchronously
_PendingFrame = namedtuple("_PendingFrame", "pinned cap_key ran_plain call")
# one gsx_render_forward call, all but the per-view state (GaussianScene._plan_frame).  tensors: the five parameter tensors
# (colours: None on an SH scene); owned_inputs: every tensor the call hands over besides out; keep_alive: host arrays
_FramePlan = namedtuple("_FramePlan", "dev n cam tensors params out cap_key owned_inputs keep_alive")


def _next_attempt(rc: int, n_visible: int, n_instances: int, n_redo: int, flags: int, n: int, speculative: bool,
                  owned: bool, fixed_cap: bool, semantics: str) -> Tuple[str, Optional[int]]:
    """What follows a gsx_render_forward over ``n`` Gaussians, issued with ``flags``, that returned ``rc`` and these counts:
    ("done", None) -- ``rc`` is the outcome --, or once more with ("flags", other flags) or ("cap", another pair capacity):
    1. the plain compositing instance ran and the view does hold ill-conditioned footprints: the one that evaluates them;
    2. at most three Gaussians pass the cull, fewer than the call assumed: the reference's BLAS then sums its products over
       the visible ones in another order (GSX_FLAG_SMALL_BATCH / _ONE_VISIBLE, include/gsx.h) -- in that order; an owned
       call is told its row class, std_3dgs has none;
    3. the workspace was too small: room for 1.25 x the pairs counted, unless the capacity is fixed.
    A speculative (no_sync) call has no counts yet: 1 and 2 are left to ``confirm_frames``."""
    if rc == _ffi.GSX_OK and not speculative:
        if flags & _ffi.GSX_FLAG_PLAIN_FOOTPRINTS and n_redo > 0:
            return "flags", flags & ~_ffi.GSX_FLAG_PLAIN_FOOTPRINTS
        again = 0 if owned or semantics == "std_3dgs" else _ffi.visible_rows_flag(n, n_visible, flags)
        if again:
            return "flags", _ffi.with_rows_flag(flags, again)
    if rc == _ffi.GSX_ERR_WORKSPACE_TOO_SMALL and not fixed_cap:
        return "cap", int(n_instances * 1.25) + 4096
    return "done", None


def _report(stats: dict, st: _ffi.GsxFrameStats, ran_plain: bool, owned: bool, speculative: bool, timing: bool) -> None:
    """``render_image_hip(stats=...)``; plain_footprints: the frame ran the compositing instance of GSX_FLAG_PLAIN_FOOTPRINTS."""
    if speculative:
        if not owned:
            stats.update(n_visible=None, n_instances=None, n_tiles=st.n_tiles, speculative=True, plain_footprints=ran_plain)
        return
    stats.update(n_visible=st.n_visible, n_instances=st.n_instances, n_tiles=st.n_tiles, n_kept=st.n_kept,
                 n_redo=int(st.n_redo))
    if not owned:
        stats["plain_footprints"] = ran_plain
        if timing:
            stats["stage_ms"] = {k: float(st.stage_ms[i]) for i, k in enumerate(_ffi.STAGE_NAMES)}


def _window_tiles(width: int, height: int, tile_size: int, semantics: str, tile_window) -> Tuple[int, int]:
    """Tiles along x and y of what a frame renders: ``tile_window`` with its upper bounds clamped (negative: "to the end")."""
    ntx, nty = tiles_along(width, tile_size, semantics), tiles_along(height, tile_size, semantics)
    wx0, wx1, wy0, wy1 = (0, ntx, 0, nty) if tile_window is None else [int(v) for v in tile_window]
    wx1, wy1 = (ntx if wx1 < 0 else min(wx1, ntx)), (nty if wy1 < 0 else min(wy1, nty))
    return max(0, wx1 - wx0), max(0, wy1 - wy0)


def render_preprocessed(height: int, width: int, tile_size: int, point_means: torch.Tensor,
                        point_colors: torch.Tensor, inverse_covariance_2d: torch.Tensor, min_x: torch.Tensor,
                        max_x: torch.Tensor, min_y: torch.Tensor, max_y: torch.Tensor, opacity: torch.Tensor,
                        layout: str = "wh3", instances_hint: int = 0,
                        stats: Optional[dict] = None, semantics: str = "ref_cpu", flags: int = 0) -> torch.Tensor:
    """Stage 2 on depth-sorted stage-1 arrays: the reference's native entry point
    ``render_image(image_height, image_width, tile_size, point_means, point_colors,
    inverse_covariance_2d, min_x, max_x, min_y, max_y, opacity)`` (splat/c/render.cu:90-101) with the
    CPU path's compositing semantics (``semantics="ref_cuda"``: the CUDA kernel's own semantics,
    SURVEY.md Appendix B).  Returns (W,H,3) for layout "wh3", (H,W,3) for "hw3".  ``flags``: GSX_FLAG_* of
    include/gsx.h, as they are (a caller that sets GSX_FLAG_PLAIN_FOOTPRINTS reads ``stats["n_redo"]``)."""
    lib = _ffi.load()
    dev = point_means.device
    _require_gpu(dev)
    n = int(point_means.shape[0])
    args = [_check_f32(k, v, dev) for k, v in (
        ("point_means", point_means), ("point_colors", point_colors),
        ("inverse_covariance_2d", inverse_covariance_2d), ("min_x", min_x), ("max_x", max_x),
        ("min_y", min_y), ("max_y", max_y), ("opacity", opacity))]
    params = _ffi.default_params()
    params.layout = _ffi.GSX_LAYOUT_WH3 if layout == "wh3" else _ffi.GSX_LAYOUT_HW3
    params.semantics = _SEMANTICS[semantics]
    params.flags |= int(flags)
    shape = (width, height, 3) if layout == "wh3" else (height, width, 3)
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    st = _ffi.GsxFrameStats()
    cap = max(int(instances_hint), 8 * n + 4096)
    with torch.cuda.device(dev):
        for _ in range(3):
            nbytes = lib.gsx_workspace_bytes(n, width, height, tile_size, cap)
            if nbytes == 0:
                raise _ffi.GsxError(_ffi.GSX_ERR_INVALID_ARGUMENT, "gsx_workspace_bytes rejected the sizes")
            ws = _WORKSPACE.get(dev, nbytes)
            rc = lib.gsx_render_preprocessed(height, width, tile_size, *[_ptr(a) for a in args], n, _ptr(out),
                                             ctypes.byref(params), ctypes.byref(st), _ptr(ws), ws.numel(),
                                             _stream_handle(dev))
            if rc != _ffi.GSX_ERR_WORKSPACE_TOO_SMALL:
                break
            cap = int(st.n_instances * 1.25) + 4096
    _ffi.check(rc)
    if stats is not None:
        stats.update(n_visible=st.n_visible, n_instances=st.n_instances, n_tiles=st.n_tiles, n_redo=int(st.n_redo))
    return out


class NativeExtension:
    """What ``GaussianScene.compile_cuda_ext()`` returns: the object the reference gets from ``load_inline``
    (splat/gaussian_scene.py:240-261, splat/utils.py:426-434) -- ONE function, ``render_image``, with the argument
    list and return value of splat/c/render.cu:90-101.  Here nothing is compiled at run time: the function is
    ``gsx_render_preprocessed`` of the prebuilt libgsx.so under the CUDA kernel's own rules (GSX_SEM_REF_CUDA,
    (H,W,3) output), so a caller that does ``ext = scene.compile_cuda_ext(); ext.render_image(H, W, tile, ...)``
    keeps working unchanged."""

    def __init__(self) -> None:
        _ffi.load()          # fails loudly, like a failed JIT build would, when the library is absent

    @staticmethod
    def render_image(image_height: int, image_width: int, tile_size: int, point_means: torch.Tensor,
                     point_colors: torch.Tensor, inverse_covariance_2d: torch.Tensor, min_x: torch.Tensor,
                     max_x: torch.Tensor, min_y: torch.Tensor, max_y: torch.Tensor, opacity: torch.Tensor) -> torch.Tensor:
        return render_preprocessed(int(image_height), int(image_width), int(tile_size), point_means, point_colors,
                                   inverse_covariance_2d, min_x, max_x, min_y, max_y, opacity, layout="hw3",
                                   semantics="ref_cuda")


class CapturedFrame:
    """A frame recorded by ``GaussianScene.capture_frame``: ``replay()`` launches the graph,
    ``out`` is the frame buffer it writes, ``confirm()`` (synchronises) checks that the last replay
    did not exceed the pair capacity recorded in the graph and returns the frame."""

    def __init__(self, scene: "GaussianScene", graph, out: torch.Tensor, pinned: torch.Tensor, call: dict,
                 camera_buffer: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                 capacity: int = 0, inputs: Optional[list] = None) -> None:
        self.scene, self.graph, self.out, self._pinned, self._call = scene, graph, out, pinned, call
        self._camera_buffer = camera_buffer      # device copy of the GsxCamera the recorded kernels read
        self._workspace = workspace              # scratch whose address the graph holds: lives as long as the frame
        self.capacity = int(capacity)            # (Gaussian, tile) pairs the recorded launches have room for
        # the exact parameter tensors handed to the library while recording (a non-contiguous attribute of the
        # scene is a COPY made for the call): the graph reads these addresses on every replay
        self._inputs = inputs

    def set_camera(self, image_idx: int) -> None:
        """Points the captured frame at another camera of the scene (same frame size): the next
        ``replay()`` enqueued on this stream renders that view.  Only for frames captured with
        ``movable_camera=True``.  The constants are copied on the current stream; do not call this
        while a replay of this frame is still in flight on another stream."""
        if self._camera_buffer is None:
            raise RuntimeError("this frame was captured with its camera baked in: capture it with movable_camera=True")
        cam = self.scene.images[image_idx].gsx_camera()
        first = self.scene.images[self._call["image_idx"]].gsx_camera()
        if (cam.width, cam.height) != (first.width, first.height):
            raise ValueError("a captured frame keeps its size: %dx%d, the new camera is %dx%d"
                             % (first.width, first.height, cam.width, cam.height))
        self._camera_buffer.copy_(torch.frombuffer(bytearray(bytes(cam)), dtype=torch.uint8))

    def replay(self) -> torch.Tensor:
        # (spatially ordered rows: the boxes a strip's projection trusts follow points / scales -- refreshed IN PLACE, at the
        # address the graph holds, when those were modified since; a comparison of six integers otherwise)
        g = self.scene.gaussians
        if getattr(g, "sh", None) is not None and self.scene._sh_truncated():
            raise ValueError("gaussians.active_sh_degree = %d is below sh_degree = %d: the captured frame evaluates every "
                             "stored band" % (self.scene._active_sh_degree(), int(g.sh_degree)))
        if getattr(g, "original_index", None) is not None:
            g.current_block_bounds()
        self.graph.replay()
        return self.out

    def counts(self) -> Tuple[int, int, int]:
        """(visible Gaussians, (Gaussian, tile) pairs, pairs the recorded launches have room for) of the last replay;
        synchronises.  More pairs than room: pairs were dropped, the frame has to be rendered again (``confirm()``
        raises for exactly that)."""
        torch.cuda.synchronize(self.out.device)
        st = _frame_stats(self._pinned)
        return int(st.n_visible), int(st.n_instances), int(st.reserved)

    def confirm(self) -> torch.Tensor:
        torch.cuda.synchronize(self.out.device)
        st = _frame_stats(self._pinned)
        if st.n_instances > st.reserved:
            raise _ffi.GsxError(_ffi.GSX_ERR_WORKSPACE_TOO_SMALL,
                                "the captured frame holds %d pairs but the scene now produces %d: capture it again"
                                % (st.reserved, st.n_instances))
        if getattr(self, "_plain_footprints", False) and st.n_redo > 0:
            raise _ffi.GsxError(_ffi.GSX_ERR_UNSUPPORTED,
                                "the frame was captured with GSX_FLAG_PLAIN_FOOTPRINTS and %d tiles now hold ill-conditioned "
                                "footprints: capture it again" % st.n_redo)
        return self.out


# What every Gaussian adds to the frames of one or more views (gsx_render_contribution), one row per row of the container,
# device tensors: weight_max float32 (N,) the largest blend weight T alpha in any pixel of any of the views, weight_sum
# float32 (N,) the sum of the weights, pixels int32 (N,) the (pixel, view) pairs that composited the row (the library's
# uint32), views int32 (N,) the views that listed the row on a tile.
Contribution = namedtuple("Contribution", "weight_max weight_sum pixels views")


def _screen_mode(screen_statistics):
    """``screen_statistics`` as the render calls take it: False, True (gsx_render_backward_screen) or ``"abs"``
    (gsx_render_backward_screen_abs).  Any other string is refused; any other value counts as a bool, as it always has."""
    if isinstance(screen_statistics, str):
        if screen_statistics != "abs":
            raise ValueError("screen_statistics = %r is neither a bool nor 'abs'" % (screen_statistics,))
        return "abs"
    return bool(screen_statistics)


def _camera_wants_grad(image, camera: bool) -> bool:
    """``camera_gradients=True`` and the view's ``world2view`` requires grad (grad mode on): the frame is differentiable for
    the pose alone."""
    return bool(camera) and torch.is_grad_enabled() and bool(getattr(image.world2view, "requires_grad", False))


def _wants_grad(g, geometry: bool = False) -> bool:
    """Gradients are recorded for this render: grad mode is on and the colours or the opacity logits require grad --
    or, with ``geometry`` (``geometry_gradients=True``), the points, scales or quaternions -- or, on an SH scene, the
    coefficients ``gaussians.sh`` (what makes an SH scene differentiable: ``_sh_wants_grad``)."""
    names = ("colors", "opacity", "sh") + (("points", "scales", "quaternions") if geometry else ())
    return torch.is_grad_enabled() and any(getattr(getattr(g, name, None), "requires_grad", False) for name in names)


def _sh_wants_grad(g) -> bool:
    """An SH scene is differentiable when its coefficients require grad (gsx_sh_backward carries dL/dcolour on to them)."""
    return bool(getattr(getattr(g, "sh", None), "requires_grad", False))


def _refusals(g, semantics="ref_cpu", tile_window=None, out=None, substrips=None, no_sync=False, camera_buffer=None):
    """What ``render_image_hip`` was asked for that has no gradient: (what, asked for it) in the order it is refused."""
    return [("semantics=%r" % semantics, semantics != "ref_cpu"),
            ("an SH scene (gaussians.sh) whose coefficients do not require grad (call gaussians.sh.requires_grad_(True) to "
             "differentiate it)", getattr(g, "sh", None) is not None and not _sh_wants_grad(g)),
            ("tile_window", tile_window is not None), ("out", out is not None),
            ("substrips", substrips is not None), ("no_sync", bool(no_sync)),
            ("camera_buffer", camera_buffer is not None)]


def _refuse_with_grad(what: str) -> None:
    raise ValueError("gradients of the frame (gaussians.colors / gaussians.opacity / gaussians.sh require grad) are not "
                     "available with %s: only the whole ref_cpu frame is differentiable, of RGB colours or of SH "
                     "coefficients that require grad (gsx_render_backward, with geometry_gradients=True "
                     "gsx_render_backward_geometry, gsx_sh_backward); call it under torch.no_grad() or without "
                     "requires_grad" % what)


def _check_antialiased(antialiased, semantics: str, camera_gradients=False, screen_statistics=False) -> None:
    """``antialiased=True`` belongs to the std_3dgs rule set and to what that rule set computes: refused by name otherwise,
    with or without gradients."""
    if not antialiased:
        return
    if semantics != "std_3dgs":
        raise ValueError("antialiased=True needs semantics='std_3dgs', got semantics=%r: the opacity compensation "
                         "(GSX_FLAG_ANTIALIASED) is a variant of the published rule set, ref_cpu and ref_cuda have none"
                         % (semantics,))
    if camera_gradients:
        raise ValueError("antialiased=True cannot be combined with camera_gradients=True: the std_3dgs frame has no pose "
                         "gradient (gsx_render_backward_std)")
    if _screen_mode(screen_statistics) == "abs":
        raise ValueError("antialiased=True cannot be combined with screen_statistics='abs': the std_3dgs frame has no "
                         "absolute statistic (gsx_render_backward_std); pass screen_statistics=True")


def _refuse_std_with_grad(what: str) -> None:
    raise ValueError("gradients of the std_3dgs frame (gsx_render_backward_std) are not available with %s: they reach "
                     "colors / sh, opacity and, with geometry_gradients=True, points, scales and quaternions, with "
                     "screen_statistics=True the signed screen statistic -- no pose, no absolute statistic, no "
                     "dL/dbackground; call it under torch.no_grad() or without requires_grad" % what)


_ROW_ARRAYS = ("points", "scales", "quaternions", "opacity")
# what a differentiable frame's forward saw of the state its backward reads again (_pending_snapshot / _check_pending)
_PendingState = namedtuple("_PendingState", "scene image_idx image pose_version gaussians bands arrays original_index "
                                            "row_of_index")


def _raw_active_sh_degree(g) -> int:
    return int(getattr(g, "active_sh_degree", int(g.sh_degree)))


def _pending_snapshot(scene, image_idx, points, scales, quaternions, opacity, colors, sh) -> _PendingState:
    """What the backward of a differentiable frame of view ``image_idx`` will read again from the live scene and cannot
    otherwise verify, as the forward saw it: the view's ``GaussianImage`` and its ``pose_version``; on an SH scene
    (``sh`` given) ``sh_degree`` and the checked active degree; the storage address and shape of the five arrays the
    forward was given (``colors``, or ``sh`` on an SH scene); the ``original_index`` / ``row_of_index`` tensors; the
    container itself.  Host values only: nothing is read from the device.  The arrays are kept alive by the caller
    (``save_for_backward``), so an address cannot be handed out again while the frame is pending."""
    g = scene.gaussians
    image = scene.images[image_idx]
    bands = None if sh is None else (int(g.sh_degree), scene._active_sh_degree())
    given = dict(zip(_ROW_ARRAYS, (points, scales, quaternions, opacity)))
    given["colors" if sh is None else "sh"] = colors if sh is None else sh
    arrays = tuple((name, int(t.data_ptr()), tuple(t.shape)) for name, t in given.items())
    return _PendingState(scene, image_idx, image, int(getattr(image, "pose_version", 0)), g, bands, arrays,
                         getattr(g, "original_index", None), getattr(g, "row_of_index", None))


def _check_pending(state: _PendingState) -> None:
    """The comparison to ``_pending_snapshot``, before a backward launches anything: RuntimeError naming the view and what
    changed -- ``pose`` (the view's image was replaced, or ``set_world2view`` was called, with whatever matrix),
    ``active_sh_degree`` / ``sh_degree``, or the array that was REPLACED (another storage or another shape).  An edit in
    place is not looked for here: autograd's version counters report it.  No device read, no synchronisation."""
    scene, idx = state.scene, state.image_idx

    def refuse(what: str) -> None:
        raise RuntimeError("the backward of the frame of view %r was refused: %s changed between its forward and its "
                           "backward, and the backward reads the live scene again (projection, depth order and binning "
                           "are recomputed): render the frame again and call backward on the new one" % (idx, what))

    image = scene.images.get(idx) if hasattr(scene.images, "get") else scene.images[idx]
    if image is not state.image or int(getattr(image, "pose_version", 0)) != state.pose_version:
        refuse("the pose (GaussianImage.set_world2view)")
    g = scene.gaussians
    if g is not state.gaussians:
        refuse("scene.gaussians (the container was replaced)")
    if state.bands is not None:
        if getattr(g, "sh", None) is None or int(g.sh_degree) != state.bands[0]:
            refuse("gaussians.sh_degree")
        if _raw_active_sh_degree(g) != state.bands[1]:
            refuse("gaussians.active_sh_degree (%d at the forward, %d now)" % (state.bands[1], _raw_active_sh_degree(g)))
    elif getattr(g, "sh", None) is not None:
        refuse("gaussians.sh (an RGB scene at the forward)")
    for name, address, shape in state.arrays:
        t = getattr(g, name, None)
        if not torch.is_tensor(t) or int(t.data_ptr()) != address or tuple(t.shape) != shape:
            refuse("gaussians.%s (the array was replaced: %s at the forward, %s now)"
                   % (name, shape, tuple(t.shape) if torch.is_tensor(t) else None))
    for name, seen in (("original_index", state.original_index), ("row_of_index", state.row_of_index)):
        if getattr(g, name, None) is not seen:
            refuse("gaussians.%s (the row order)" % name)


class _RenderImageFunction(torch.autograd.Function):
    """The ref_cpu frame as a function of (points, scales, quaternions, opacity, colors, sh); ``sh`` is None for an RGB
    scene.  Forward: the frame ``render_image_hip`` returns without gradients, bit for bit.  Backward:
    gsx_render_backward -- dL/dcolors and dL/dopacity (logits); points, scales and quaternions get None, as in the
    reference.  With ``geometry_gradients=True``: gsx_render_backward_geometry -- also dL/dpoints, dL/dscales (linear
    scales) and dL/dquaternions, each for the tensors that require grad; the colour and opacity gradients are the same
    bits.  With ``screen_statistics=True`` besides: gsx_render_backward_screen, the same five gradients, and
    ``scene.screen_statistics`` = (image_idx, dL/d(NDC mean) (N,2), screen radius (N,)) left for ``DensityControl``; with
    ``screen_statistics="abs"`` gsx_render_backward_screen_abs, the same and a fourth entry, the absolute statistic (N,2).  An SH scene: the library is handed this camera's evaluated colours, so its dL/dcolors is dL/d(view-dependent
    colour), and gsx_sh_backward carries that on to dL/dsh and -- with geometry gradients -- adds the view direction's
    share to dL/dpoints; ``colors`` gets None (the frame does not read it).  The backward does not use what the forward computed:
    it reads the live scene again (the arrays, the row order, the view's camera, the active SH degree) and trusts only
    the forward's counts.  Two checks hold the two together.  The tensors are saved, so autograd's version counters catch
    an edit IN PLACE between forward and backward (autograd's error).  ``_check_pending`` catches what autograd cannot
    see -- ``set_world2view`` on the view, ``active_sh_degree`` / ``sh_degree`` changed, an array, the row order or the
    container REPLACED (``densify_and_prune``, ``relocate``, an assignment) -- and refuses the backward by name
    (RuntimeError) before anything is launched.  Frames of other views, tile sizes or scenes rendered in between change
    nothing.  ``world2view`` (None unless ``camera_gradients=True``
    and the view's tensor requires grad) gets the total derivative of the pose: gsx_render_backward_camera's
    dL/dworld2view + dL/dfull_proj @ projection_matrix^T, plus, on an SH scene, the camera centre's share.
    ``semantics="std_3dgs"`` in ``kw`` (with its ``background``, ``published_rects`` and ``antialiased``): the frame is the std_3dgs frame and
    the backward is one gsx_render_backward_std call for the same outputs, the screen statistics included; no pose and no
    absolute statistic there."""

    @staticmethod
    def forward(ctx, scene, image_idx, tile_size, layout, kw, points, scales, quaternions, opacity, colors, sh,
                world2view=None):
        kw = dict(kw)
        ctx.camera = world2view is not None
        ctx.geometry = bool(kw.pop("geometry_gradients", False)) or ctx.camera
        mode = kw.pop("screen_statistics", False)
        ctx.screen, ctx.screen_abs = bool(mode), mode == "abs"
        # semantics="std_3dgs": the frame's rules, background and rectangles, which gsx_render_backward_std is told again
        ctx.std = (tuple(float(v) for v in kw.get("background", (0.0, 0.0, 0.0))), bool(kw.get("published_rects", False)),
                   bool(kw.get("antialiased", False))) if kw.get("semantics", "ref_cpu") == "std_3dgs" else None
        user_stats, st = kw.pop("stats", None), {}
        frame = scene.render_image_hip(image_idx, tile_size=tile_size, layout=layout, stats=st, **kw)
        if user_stats is not None:
            user_stats.update(st)
        ctx.scene, ctx.image_idx, ctx.tile_size, ctx.layout = scene, image_idx, tile_size, layout
        ctx.n_instances, ctx.n_visible = int(st["n_instances"]), int(st["n_visible"])
        ctx.has_sh = sh is not None
        ctx.pending = _pending_snapshot(scene, image_idx, points, scales, quaternions, opacity, colors, sh)
        ctx.save_for_backward(points, scales, quaternions, opacity, colors, frame, *((sh,) if ctx.has_sh else ()))
        return frame

    @staticmethod
    def backward(ctx, grad_frame):
        points, scales, quaternions, opacity, colors, frame = ctx.saved_tensors[:6]
        _check_pending(ctx.pending)         # before any library call: the backward reads the live scene again
        scene = ctx.scene
        want = ctx.needs_input_grad
        # the colour-only call gives the same colour and opacity bits; the screen entry runs whoever requires grad
        camera = ctx.camera and want[11]
        geometry = ctx.geometry and (ctx.screen or camera or any(want[5:8]))
        grads = scene._render_backward(ctx.image_idx, ctx.tile_size, ctx.layout, frame, grad_frame,
                                       ctx.n_instances, ctx.n_visible, geometry=geometry, screen=ctx.screen, camera=camera,
                                       screen_abs=ctx.screen_abs, std=ctx.std)
        gc, go = grads[:2]
        gp, gs, gq = grads[2:5] if geometry else (None, None, None)
        if ctx.screen_abs:
            scene.screen_statistics = (ctx.image_idx, grads[5], grads[6].view(-1), grads[7])
        elif ctx.screen:
            scene.screen_statistics = (ctx.image_idx, grads[5], grads[6].view(-1))
        gw2v = None
        if camera:          # full_proj = world2view @ projection_matrix: the two partial derivatives into the total one
            image = scene.images[ctx.image_idx]
            gw2v = grads[-2] + grads[-1] @ image.projection_matrix.t()
        gsh = None
        if ctx.has_sh:      # gc is dL/d(view-dependent colour): on to the coefficients, and through the direction to the mean
            sh = ctx.saved_tensors[6]
            gsh, gview = scene._sh_backward(ctx.image_idx, gc, with_points=camera or (geometry and want[5]))
            gsh, gc = gsh.view(sh.shape), None
            if gview is not None and camera:
                # the direction is point - centre: dL/dcentre = -sum of the rows; centre = inverse(world2view)[3,:3], and
                # d inverse(V) = -inverse(V) dV inverse(V), so dL/dV = -inverse(V)^T G inverse(V)^T with G[3,:3] = dL/dcentre
                inv_t = image.view2world.t()
                G = torch.zeros((4, 4), dtype=torch.float32, device=gview.device)
                G[3, :3] = -gview.sum(0)
                gw2v = gw2v - inv_t @ G @ inv_t
            if gview is not None and gp is not None and want[5]:
                gp = gp + gview
        return (None, None, None, None, None,
                gp.view(points.shape) if gp is not None and want[5] else None,
                gs.view(scales.shape) if gs is not None and want[6] else None,
                gq.view(quaternions.shape) if gq is not None and want[7] else None,
                go.view(opacity.shape) if want[8] else None,
                gc.view(colors.shape) if gc is not None and want[9] else None,
                gsh if want[10] else None,
                gw2v)


class _RenderImageDepthFunction(torch.autograd.Function):
    """(frame, depth image) of the ref_cpu frame as a function of (points, scales, quaternions, opacity, colors, sh): the
    frame of ``_RenderImageFunction`` and gsx_render_depth's (D, A).  Backward: gsx_render_backward_depth, once, for
    dL/dframe and dL/ddepth together (either may be missing: zeros); the SH share as in ``_RenderImageFunction``, and the
    same two checks between forward and backward: autograd's version counters for an edit in place, ``_check_pending`` for a
    pose, an SH degree or an array that was replaced."""

    @staticmethod
    def forward(ctx, scene, image_idx, tile_size, layout, kw, points, scales, quaternions, opacity, colors, sh):
        ctx.screen = bool(kw.get("screen_statistics", False))
        user_stats, st = kw.get("stats", None), {}
        frame = scene.render_image_hip(image_idx, tile_size=tile_size, layout=layout, stats=st)
        if user_stats is not None:
            user_stats.update(st)
        ctx.scene, ctx.image_idx, ctx.tile_size, ctx.layout = scene, image_idx, tile_size, layout
        ctx.n_instances, ctx.n_visible = int(st["n_instances"]), int(st["n_visible"])
        depth = scene._render_depth(image_idx, tile_size, layout, ctx.n_instances, ctx.n_visible)
        ctx.has_sh = sh is not None
        ctx.pending = _pending_snapshot(scene, image_idx, points, scales, quaternions, opacity, colors, sh)
        ctx.save_for_backward(points, scales, quaternions, opacity, colors, frame, depth, *((sh,) if ctx.has_sh else ()))
        return frame, depth

    @staticmethod
    def backward(ctx, grad_frame, grad_depth):
        points, scales, quaternions, opacity, colors, frame, depth = ctx.saved_tensors[:7]
        _check_pending(ctx.pending)
        scene = ctx.scene
        want = ctx.needs_input_grad
        if grad_frame is None:
            grad_frame = torch.zeros_like(frame)
        if grad_depth is None:
            grad_depth = torch.zeros_like(depth)
        grads = scene._render_backward(ctx.image_idx, ctx.tile_size, ctx.layout, frame, grad_frame, ctx.n_instances,
                                       ctx.n_visible, geometry=True, screen=ctx.screen, depth=depth, grad_depth=grad_depth)
        gc, go, gp, gs, gq = grads[:5]
        if ctx.screen:
            scene.screen_statistics = (ctx.image_idx, grads[5], grads[6].view(-1))
        gsh = None
        if ctx.has_sh:
            sh = ctx.saved_tensors[7]
            gsh, gview = scene._sh_backward(ctx.image_idx, gc, with_points=want[5])
            gsh, gc = gsh.view(sh.shape), None
            if gview is not None:
                gp = gp + gview
        return (None, None, None, None, None,
                gp.view(points.shape) if want[5] else None,
                gs.view(scales.shape) if want[6] else None,
                gq.view(quaternions.shape) if want[7] else None,
                go.view(opacity.shape) if want[8] else None,
                gc.view(colors.shape) if gc is not None and want[9] else None,
                gsh if want[10] else None)


class GaussianScene:
    def __init__(self, colmap_path: str, gaussians: Gaussians) -> None:
        self._init_from_views(read_camera_file(colmap_path), read_image_file(colmap_path), gaussians)

    @classmethod
    def from_views(cls, cameras, images, gaussians: Gaussians) -> "GaussianScene":
        """The scene of ``cameras`` (id -> ``colmap.Camera``) and ``images`` (id -> ``colmap.Image``), the two dicts the
        constructor reads from disk: ``GaussianScene(colmap_path, g)`` is ``from_views(read_camera_file(colmap_path),
        read_image_file(colmap_path), g)``, one body.  For cameras that are not on disk as they are wanted
        (``capture.load_capture``: the rectified pinholes of a capture's lens-distorted cameras)."""
        scene = cls.__new__(cls)
        scene._init_from_views(cameras, images, gaussians)
        return scene

    def _init_from_views(self, cameras, images, gaussians: Gaussians) -> None:
        self.images: Dict[int, GaussianImage] = {}
        for idx, image in images.items():
            self.images[idx] = GaussianImage(camera=cameras[image.camera_id], image=image,
                                             device=gaussians.device)
        self.gaussians = gaussians
        self._instances_hint = 0      # workspace sizing: largest instance count seen (+10 %)
        self._last_instances = 0      # instance count of the latest full frame
        self._cap_hints = {}          # (image, tile, window, semantics) -> pair capacity for the next frame
        self._kept_hints = {}         # same key -> Gaussians that reached a tile of the window (GsxParams.kept_hint)
        self._n_redo_seen = {}         # same key -> tiles of the last frame that held an ill-conditioned footprint (n_redo)
        self._hints = _Lru(_HINT_VIEWS)   # (same key, stream) -> [GsxParams.hints buffer, a frame has run with it?]
        self._pending = []            # speculative frames awaiting confirm_frames()
        self._part_events = {}        # (stream, K) -> K HIP events the library records behind the parts of a frame
        self._pinned_pool = None
        self._pinned_next = 0
        # (image_idx, dL/d(NDC mean) (N,2), radius (N,)) of the latest screen_statistics backward; "abs": + the absolute one (N,2)
        self.screen_statistics = None
        self._pose_seen = {}          # image -> GaussianImage.pose_version its last frame was planned with (_check_pose)

    # ------------------------------------------------------------------ helpers
    def _colors(self, image_idx: int) -> torch.Tensor:
        """``gaussians.colors`` like the reference, or -- build extension -- the view-dependent colour
        of this camera evaluated on the GPU from the active bands of ``gaussians.sh`` (gsx_sh_to_rgb_active: with every
        stored band active, gsx_sh_to_rgb's kernels)."""
        g = self.gaussians
        if getattr(g, "sh", None) is None:
            return g.colors
        lib = _ffi.load()
        dev = g.points.device
        _require_gpu(dev)
        n = int(g.points.shape[0])
        pts = _check_f32("points", g.points.reshape(n, 3), dev)
        sh, degree = self._sh_flat(n, dev)
        out = torch.empty((n, 3), dtype=torch.float32, device=dev)
        center = (ctypes.c_float * 3)(*self.images[image_idx].camera_center_host)   # no device read per frame
        with torch.cuda.device(dev):
            rc = lib.gsx_sh_to_rgb_active(_ptr(pts), _ptr(sh), degree, self._active_sh_degree(), n, center, _ptr(out),
                                          _stream_handle(dev))
        _ffi.check(rc)
        return out

    def _sh_flat(self, n: int, dev) -> Tuple[torch.Tensor, int]:
        """(``gaussians.sh`` as the library reads it: contiguous float32 (n, K, 3) on ``dev``; its degree, K = (degree + 1)^2)."""
        g = self.gaussians
        degree = int(g.sh_degree)
        return _check_f32("sh", g.sh.reshape(n, (degree + 1) ** 2, 3), dev), degree

    def _active_sh_degree(self) -> int:
        """``gaussians.active_sh_degree``, checked against the stored degree (a container without the attribute: the stored
        degree)."""
        g = self.gaussians
        stored = int(g.sh_degree)
        active = int(getattr(g, "active_sh_degree", stored))
        if not 0 <= active <= stored:
            raise ValueError("gaussians.active_sh_degree = %d is outside 0..%d (sh_degree)" % (active, stored))
        return active

    def _sh_truncated(self) -> bool:
        """An SH scene on its degree schedule: fewer bands active than stored.  Its frames are rendered from this camera's
        evaluated colours (``_colors``), not from GsxParams.sh, whose projection kernel evaluates every stored band."""
        g = self.gaussians
        return getattr(g, "sh", None) is not None and self._active_sh_degree() < int(g.sh_degree)

    def _inputs(self, image_idx: Optional[int] = None, inline_sh: bool = False):
        """The five parameter tensors the library reads.  With ``inline_sh`` and an SH scene the last one is
        None: the whole-path entry evaluates the colour itself from ``gaussians.sh`` (GsxParams.sh)."""
        g = self.gaussians
        dev = g.points.device
        _require_gpu(dev)
        n = int(g.points.shape[0])
        has_sh = getattr(g, "sh", None) is not None
        tensors = [
            _check_f32("points", g.points.reshape(n, 3), dev),
            _check_f32("scales", g.scales.reshape(n, 3), dev),
            _check_f32("quaternions", g.quaternions.reshape(n, 4), dev),
            _check_f32("opacity", g.opacity.reshape(n, 1), dev),
        ]
        if has_sh and inline_sh:
            tensors.append(None)
        else:
            colors = g.colors if (image_idx is None or not has_sh) else self._colors(image_idx)
            tensors.append(_check_f32("colors", colors.reshape(n, 3), dev))
        return dev, n, tensors

    def _original_index(self, dev, n: int) -> Optional[torch.Tensor]:
        """``gaussians.original_index`` (Gaussians.spatially_ordered) as the library wants it -- int32, contiguous, n
        entries, on the device of the parameters -- or None for rows in the caller's own order."""
        oi = getattr(self.gaussians, "original_index", None)
        if oi is None:
            return None
        if oi.device != dev or oi.dtype != torch.int32 or not oi.is_contiguous() or oi.numel() != n:
            raise ValueError("gaussians.original_index must be a contiguous int32 tensor of %d entries on %s" % (n, dev))
        return oi

    def _frame_params(self, dev, n: int, layout: str, semantics: str):
        """(GsxParams, original_index or None) of a whole-path call: the layout, the rule set and, for spatially ordered
        rows, GsxParams.original_index / row_of_index, both checked.  render_image_hip and the backward start from it."""
        params = _ffi.default_params()
        oi = self._original_index(dev, n)
        if oi is not None:          # spatially ordered rows (Gaussians.spatially_ordered): same frame, bit for bit
            ro = getattr(self.gaussians, "row_of_index", None)
            if ro is None or ro.device != dev or ro.dtype != torch.int32 or not ro.is_contiguous() or ro.numel() != n:
                raise ValueError("gaussians.row_of_index (the inverse of original_index) must be a contiguous int32 tensor "
                                 "of %d entries on %s" % (n, dev))
            params.original_index, params.row_of_index = oi.data_ptr(), ro.data_ptr()
        params.layout = _ffi.GSX_LAYOUT_WH3 if layout == "wh3" else _ffi.GSX_LAYOUT_HW3
        params.semantics = _SEMANTICS[semantics]
        return params, oi

    # ------------------------------------------------------------------ stage 1
    def preprocess(self, image_idx: int) -> PreprocessedScene:
        """Projection + depth sort on the GPU (gsx_preprocess); fields as splat/schema.py:13-25."""
        lib = _ffi.load()
        dev, n, tensors = self._inputs(image_idx)
        cam = self.images[image_idx].gsx_camera()
        # one allocation for the eleven float outputs (21 floats per Gaussian) and the order, carved into views
        flat = torch.empty(max(n, 1) * 22, dtype=torch.float32, device=dev)
        off = [0]

        def f(*shape):
            cnt = 1
            for v in shape:
                cnt *= v
            view = flat[off[0]:off[0] + cnt].view(*shape)
            off[0] += cnt
            return view

        xy, col, c2, dep, inv, rad = f(n, 2), f(n, 3), f(n, 2, 2), f(n), f(n, 2, 2), f(n)
        mnx, mxx, mny, mxy, sop = f(n), f(n), f(n), f(n), f(n, 1)
        order = f(n).view(torch.int32)
        nvis = ctypes.c_int64(0)
        params = _ffi.default_params()
        oi = self._original_index(dev, n)
        if oi is not None:          # spatially ordered rows: everything is filed and reported under the original index
            params.original_index = oi.data_ptr()
        with torch.cuda.device(dev):
            nbytes = lib.gsx_workspace_bytes(n, cam.width, cam.height, 16, 1)
            ws = _WORKSPACE.get(dev, nbytes)
            for _ in range(2):
                rc = lib.gsx_preprocess(ctypes.byref(cam), *[_ptr(t) for t in tensors], n,
                                        *[_ptr(t) for t in (xy, col, c2, dep, inv, rad, mnx, mxx, mny, mxy, sop)],
                                        _ptr(order), ctypes.byref(nvis), ctypes.byref(params), _ptr(ws), ws.numel(),
                                        _stream_handle(dev))
                # at most three Gaussians pass the cull, fewer than the call assumed: the reference's BLAS then sums its
                # products over the visible ones in another order (GSX_FLAG_SMALL_BATCH / _ONE_VISIBLE, include/gsx.h) --
                # once more, in that order
                again = _ffi.visible_rows_flag(n, int(nvis.value), params.flags) if rc == _ffi.GSX_OK else 0
                if not again:
                    break
                params.flags = _ffi.with_rows_flag(params.flags, again)
        _ffi.check(rc)
        m = nvis.value
        self.last_order = order[:m]
        return PreprocessedScene(points=xy[:m], colors=col[:m], covariance_2d=c2[:m], depths=dep[:m],
                                 inverse_covariance_2d=inv[:m], radius=rad[:m], points_xy=xy[:m],
                                 min_x=mnx[:m], min_y=mny[:m], max_x=mxx[:m], max_y=mxy[:m],
                                 sigmoid_opacity=sop[:m])

    # ------------------------------------------------------------------ whole path
    def render_image_hip(self, image_idx: int, tile_size: int = 16, layout: str = "wh3",
                         tile_window: Optional[Tuple[int, int, int, int]] = None,
                         out: Optional[torch.Tensor] = None, out_origin: Tuple[int, int] = (0, 0),
                         stats: Optional[dict] = None, timing: bool = False,
                         no_sync: bool = False, semantics: str = "ref_cpu",
                         background: Tuple[float, float, float] = (0.0, 0.0, 0.0),
                         generic_kernels: bool = False, published_rects: bool = False,
                         camera_buffer: Optional[torch.Tensor] = None,
                         tile_counts: Optional[torch.Tensor] = None, split_long_tiles: bool = True,
                         tile_schedule: Optional[bool] = None, use_hints: bool = True,
                         substrips: Optional[Sequence[int]] = None, substrip_events: Optional[list] = None,
                         _private: Optional[dict] = None, geometry_gradients: bool = False,
                         screen_statistics: bool = False, camera_gradients: bool = False,
                         antialiased: bool = False) -> torch.Tensor:
        """Full forward render in libgsx (gsx_render_forward).

        semantics: "ref_cpu" (the reference's ``render_image``), "ref_cuda" (its CUDA kernel's rules
        on the same stage 1) or "std_3dgs" (build extension: the published 3DGS forward pass --
        0.3 dilation, alpha clamp 0.99, 1/255 skip, T < 1e-4 stop, ``background`` behind the last
        Gaussian, every tile of the frame; see include/gsx.h).

        layout "wh3" -> (W,H,3) indexed [x,y] like ``render_image``; "hw3" -> (H,W,3).
        tile_window (tx0,tx1,ty0,ty1) renders only those tiles (row/column strips for multi-GPU);
        ``out`` may then be a strip-sized buffer whose pixel (0,0) is frame pixel ``out_origin``.
        ``timing`` asks the library for per-stage HIP-event times (``stats["stage_ms"]``); the call
        then waits for the frame.
        ``tile_counts`` (int32 / uint32 device tensor, one entry per tile of the window, x-major) receives
        the length of every tile's Gaussian list (GsxParams.tile_counts; ``strips.balanced_plan``).
        ``use_hints`` (default): every (camera, tile size, window, rule set, stream) of this scene keeps a small
        device buffer (GsxParams.hints) in which a frame leaves the depth-sort splitters and what every tile cost
        for the NEXT frame of that view, which then skips the two kernels that would compute them on its own critical
        path; stale hints (the Gaussians or the camera changed) cost time, never a pixel.  ``use_hints=False``
        renders every frame from scratch (tests hold the two against each other).
        ``substrips`` (GsxParams.n_substrips): K + 1 ascending tile coordinates along the layout's LEADING axis (x for
        "wh3", y for "hw3") that cut the window into K parts; projection, depth order and binning run once, the
        compositing launch once per part, and ``substrip_events`` (a list the caller passes in) receives K ``_hip.Event``
        objects, event k recorded on the current stream right behind part k -- a multi-GPU rank starts sending part k
        while part k + 1 is composited (``strips.render_overlapped``).  Same pixels bit for bit.
        ``no_sync`` (GSX_FLAG_NO_SYNC) enqueues the frame without waiting for the device at all: the
        counts arrive later in pinned memory and ``confirm_frames()`` must be called (it
        synchronises) before the images are trusted -- it re-renders, on the normal path, any frame
        whose pair count exceeded the workspace capacity it was enqueued with.
        ``geometry_gradients``: the frame is differentiable whenever grad mode is on and ``gaussians.colors`` or
        ``gaussians.opacity`` require grad (gsx_render_backward: those two gradients, ``None`` for the geometry, as
        under the reference's autograd).  ``geometry_gradients=True`` also records gradients when only ``points``,
        ``scales`` or ``quaternions`` require grad, and delivers dL/dpoints, dL/dscales and dL/dquaternions
        (gsx_render_backward_geometry) to those of the three that do.  The frame is the same bits either way.
        Several differentiable frames -- of other views, through ``render_image_depth_hip`` too -- may be pending before the
        first ``backward()``; each backward recomputes its view from the live scene, so ``set_world2view`` on the view, another
        ``active_sh_degree``, or a parameter array REPLACED (``DensityControl.densify_and_prune``, ``MCMCControl.relocate``, an
        assignment) between a frame's forward and its backward is refused by name (RuntimeError: render the frame again); an
        edit in place is autograd's own error.
        An SH scene is differentiable when ``gaussians.sh`` requires grad: dL/dsh (gsx_sh_backward) and dL/dopacity, and
        with ``geometry_gradients=True`` the geometry too, dL/dpoints including the share that reaches the mean through the
        view direction; an SH scene whose ``sh`` does not require grad is refused when gradients are asked for.
        ``screen_statistics`` (needs ``geometry_gradients=True``): when the frame is differentiable its ``backward()`` runs
        gsx_render_backward_screen -- whichever tensors require grad -- and leaves ``scene.screen_statistics`` =
        (image_idx, dL/d(NDC mean) (N,2), screen radius in pixels (N,)), one row per row of the container, zeros for a
        Gaussian the frame listed on no tile; every such backward replaces it -- with several such frames pending the slot
        holds the view whose backward ran LAST, which is autograd's choice, not the order of the forwards --,
        ``DensityControl(statistic="screen")`` consumes it.  It is the rasteriser's share, the published ``viewspace_points.grad[:, :2]``: an SH scene's
        view-direction term (gsx_sh_backward) reaches ``points.grad`` only.  Gradients and frame are the same bits either way.
        ``screen_statistics="abs"``: the backward runs gsx_render_backward_screen_abs instead and leaves a 4-tuple, the three
        entries above -- the same bits -- and the ABSOLUTE statistic (N,2): per component the sum over the Gaussian's pixels of
        the absolute value of each pixel's term of dL/d(NDC mean), which a large Gaussian over fine detail does not cancel
        (AbsGS's "gradient collision"); ``DensityControl(statistic="screen_abs")`` consumes it.  Not with
        ``camera_gradients=True`` (ValueError): the pose entry has no absolute statistic.
        ``gaussians.active_sh_degree`` below ``sh_degree`` (the SH degree schedule): the frame, with or without gradients,
        is the one of the scene truncated to the active bands -- rendered from this camera's evaluated colours
        (gsx_sh_to_rgb_active) instead of GsxParams.sh, one (N,3) array per frame; dL/dsh is zero in the inactive bands.
        ``camera_buffer`` is then refused (ValueError).
        ``camera_gradients``: when ``scene.images[image_idx].world2view.requires_grad`` is set (and grad mode is on) the
        frame is differentiable for the pose -- alone, or beside whichever Gaussian arrays require grad -- and
        ``backward()`` leaves in ``world2view.grad`` the total derivative dL/dworld2view + dL/dfull_proj @
        projection_matrix^T of gsx_render_backward_camera (full_proj_transform = world2view @ projection_matrix; the
        intrinsics are constants), plus, on an SH scene, the share that reaches the pose through the camera centre
        (the view direction's gradient of gsx_sh_backward_active, which this path always requests, through
        inverse(world2view)[3,:3]).  It implies the geometry kernels whether or not a geometry array requires grad; the
        Gaussian gradients and the frame are the same bits either way.  The frame is rendered from the ``GsxCamera`` baked
        by the image: editing ``world2view`` in place does NOT move the camera, ``GaussianImage.set_world2view`` does
        (``CameraRefiner`` steps the pose that way).  The refusals are those of the other gradient paths.
        ``semantics="std_3dgs"`` with gradients: the frame is the std_3dgs frame rendered without them, bit for bit, over
        ``background`` and with ``published_rects`` as given, and ``backward()`` is one gsx_render_backward_std call: dL/dcolors
        (or dL/dsh through gsx_sh_backward) and dL/dopacity, with ``geometry_gradients=True`` dL/dpoints, dL/dscales and
        dL/dquaternions through that rule set's own stage 1, with ``screen_statistics=True`` ``scene.screen_statistics`` as
        above (dL/d(NDC mean) and the published radius).  A clamped alpha (0.99) passes gradient to its colour only.  Refused
        by name there (ValueError; all of them run under ``torch.no_grad()``): ``camera_gradients=True``,
        ``screen_statistics="abs"``, a ``background`` that requires grad (dL/dbackground is not computed), and the arguments
        the ref_cpu gradient path refuses; ``semantics="ref_cuda"`` has no gradient.
        ``antialiased`` (``semantics="std_3dgs"`` only, GSX_FLAG_ANTIALIASED): the anti-aliased variant of that rule set --
        Mip-Splatting's 2D filter, the published rasteriser's ``antialiasing`` switch, gsplat's
        ``rasterize_mode="antialiased"``.  The 0.3 dilation stays and the opacity is multiplied by
        rho = sqrt(max(0.000025, det(cov2d) / det(cov2d + 0.3 I))), so a widened Gaussian keeps the energy of the original;
        the 1/255 skip, the 0.99 clamp and the stop rule see the product.  With gradients the same one backward call, with
        dL/dopacity through sigmoid * rho and dL/drho on to points, scales and quaternions (a rho on its floor, 0.005,
        passes none).  ``antialiased=True`` under any other semantics is refused (ValueError), and so is what std_3dgs
        refuses: ``camera_gradients=True``, ``screen_statistics="abs"``, the depth image (``render_image_depth_hip`` renders
        the ref_cpu frame and has no such argument; gsx_render_depth refuses the flag by name).
        """
        _check_antialiased(antialiased, semantics, camera_gradients, screen_statistics)
        screen_statistics = _screen_mode(screen_statistics)
        if screen_statistics and not geometry_gradients:
            raise ValueError("screen_statistics=%r needs geometry_gradients=True: the statistic comes out of the geometry "
                             "backward (gsx_render_backward_screen)" % (screen_statistics,))
        if screen_statistics == "abs" and camera_gradients:
            raise ValueError("screen_statistics='abs' cannot be combined with camera_gradients=True: "
                             "gsx_render_backward_camera has no absolute statistic; pass screen_statistics=True with the pose, "
                             "or refine the pose in frames of its own")
        g = self.gaussians
        w2v = self.images[image_idx].world2view if _private is None and \
            _camera_wants_grad(self.images[image_idx], camera_gradients) else None
        if _private is None and (w2v is not None or _wants_grad(g, bool(geometry_gradients))):
            # gradients (gsx_render_backward, gsx_render_backward_geometry, gsx_sh_backward): the whole ref_cpu frame, or
            # (gsx_render_backward_std) the whole std_3dgs frame -- decided here, the other arguments go through _refusals
            std = semantics == "std_3dgs"
            if std:
                for what, bad in (("camera_gradients=True", bool(camera_gradients)),
                                  ("screen_statistics='abs'", screen_statistics == "abs"),
                                  ("a background that requires grad",
                                   any(getattr(v, "requires_grad", False) for v in (background, *tuple(background))))):
                    if bad:
                        _refuse_std_with_grad(what)
            for what, bad in _refusals(g, "ref_cpu" if std else semantics, tile_window, out, substrips, no_sync, camera_buffer):
                if bad:
                    _refuse_with_grad(what)
            kw = dict(stats=stats, timing=timing, generic_kernels=generic_kernels, tile_counts=tile_counts,
                      split_long_tiles=split_long_tiles, tile_schedule=tile_schedule, use_hints=use_hints,
                      geometry_gradients=bool(geometry_gradients), screen_statistics=screen_statistics)
            if std:
                kw.update(semantics=semantics, background=background, published_rects=published_rects,
                          antialiased=bool(antialiased))
            return _RenderImageFunction.apply(self, image_idx, tile_size, layout, kw, g.points, g.scales, g.quaternions,
                                              g.opacity, g.colors, getattr(g, "sh", None), w2v)
        own = _OwnedFrame.of(_private)
        speculative = bool(no_sync and not timing)
        plan = self._plan_frame(image_idx, tile_size, layout, tile_window, out, out_origin, timing, semantics, background,
                                generic_kernels, published_rects, camera_buffer, tile_counts, split_long_tiles,
                                tile_schedule, substrips, substrip_events, bool(antialiased))
        cap, hint_slot = self._view_state(plan, own, tile_size, tile_window, semantics, generic_kernels, use_hints)
        pinned, st = self._issue(plan, own, cap, tile_size, semantics, speculative)
        if hint_slot is not None:
            # (stream order: the next frame on this stream finds what this one left -- or, where the library took a
            # path that does not use the buffer, the zeros it was created with: its header then says "nothing here")
            hint_slot[1] = True
        ran_plain = bool(plan.params.flags & _ffi.GSX_FLAG_PLAIN_FOOTPRINTS)
        if own is None and speculative:
            # counts are still in flight: remember what has to be confirmed
            self._pending.append(_PendingFrame(pinned, plan.cap_key, ran_plain, dict(
                image_idx=image_idx, tile_size=tile_size, layout=layout, tile_window=tile_window, out=plan.out,
                out_origin=out_origin, semantics=semantics, background=background,
                generic_kernels=generic_kernels, published_rects=published_rects, camera_buffer=camera_buffer,
                tile_counts=tile_counts, split_long_tiles=split_long_tiles, tile_schedule=tile_schedule,
                use_hints=use_hints, antialiased=bool(antialiased))))
        elif own is None:
            self._note_count(plan.cap_key, int(st.n_instances), int(st.n_kept), int(st.n_redo))
        if stats is not None:
            _report(stats, st, ran_plain, own is not None, speculative, timing)
        return plan.out

    def _plan_frame(self, image_idx, tile_size, layout, tile_window, out, out_origin, timing, semantics, background,
                    generic_kernels, published_rects, camera_buffer, tile_counts, split_long_tiles, tile_schedule,
                    substrips, substrip_events, antialiased=False):
        """Validates the arguments of ``render_image_hip`` and fills GsxParams: all but the per-view state (``_view_state``)."""
        _ffi.load()         # (a missing library is reported before anything about the arguments)
        truncated = self._sh_truncated()
        if truncated and camera_buffer is not None:
            raise ValueError("camera_buffer with gaussians.active_sh_degree = %d below sh_degree = %d: the frame is rendered "
                             "from colours evaluated for camera %r, which a camera rewritten on the device would not "
                             "follow; raise active_sh_degree to sh_degree first"
                             % (self._active_sh_degree(), int(self.gaussians.sh_degree), image_idx))
        dev, n, tensors = self._inputs(image_idx, inline_sh=not truncated)
        self._check_pose(image_idx)
        cam = self.images[image_idx].gsx_camera()
        width, height = cam.width, cam.height
        params, oi = self._frame_params(dev, n, layout, semantics)
        owned_inputs = [t for t in tensors if t is not None]
        if tensors[4] is None:      # SH scene: the projection kernel evaluates the view-dependent colour itself
            sh_flat, params.sh_degree = self._sh_flat(n, dev)
            params.sh = sh_flat.data_ptr()
            owned_inputs.append(sh_flat)
        if oi is not None:
            owned_inputs += [oi, self.gaussians.row_of_index]
            bb = self._block_bounds(dev, n)
            if bb is not None:
                params.block_bounds = bb.data_ptr()
                owned_inputs.append(bb)
        params.background[0], params.background[1], params.background[2] = [float(v) for v in background]
        if timing:
            params.flags |= _ffi.GSX_FLAG_TIMING
        if generic_kernels:     # tests: the any-tile-size kernels also at tile 16 (same pixels)
            params.flags |= _ffi.GSX_FLAG_GENERIC_KERNELS
        if not split_long_tiles:   # tests: every tile on one wave (same pixels as the four-wave path of long tiles)
            params.flags |= _ffi.GSX_FLAG_NO_LONG_TILE_SPLIT
        if tile_schedule is not None:   # tiles handed out by list length (default: scenes of >= 300 000 Gaussians)
            params.flags |= _ffi.GSX_FLAG_TILE_SCHEDULE if tile_schedule else _ffi.GSX_FLAG_NO_TILE_SCHEDULE
        if published_rects:     # std_3dgs: bin with the published 3-sigma squares (same pixels, longer lists)
            params.flags |= _ffi.GSX_FLAG_PUBLISHED_RECTS
        if antialiased:         # std_3dgs: the opacity compensation of the dilation (sigmoid * rho in the record)
            params.flags |= _ffi.GSX_FLAG_ANTIALIASED
        if camera_buffer is not None:   # GsxParams.camera_device: the kernels read the camera from this buffer
            if camera_buffer.device != dev or camera_buffer.dtype != torch.uint8 or \
                    camera_buffer.numel() != ctypes.sizeof(_ffi.GsxCamera):
                raise ValueError("camera_buffer must be %d bytes (uint8) on %s" % (ctypes.sizeof(_ffi.GsxCamera), dev))
            params.camera_device = camera_buffer.data_ptr()
        if tile_window is not None:
            params.tile_x0, params.tile_x1, params.tile_y0, params.tile_y1 = [int(v) for v in tile_window]
        cut = substrips is not None and len(substrips) > 2
        keep_alive = self._plan_substrips(params, dev, layout, substrips, substrip_events) if cut else []
        if tile_counts is not None:
            if tile_counts.device != dev or tile_counts.dtype not in (torch.int32, torch.uint32) or \
                    not tile_counts.is_contiguous():
                raise ValueError("tile_counts must be a contiguous int32 tensor on %s" % dev)
            tx, ty = _window_tiles(width, height, tile_size, semantics, tile_window)
            if tile_counts.numel() < tx * ty:
                raise ValueError("tile_counts holds %d entries, the window has %d tiles" % (tile_counts.numel(), tx * ty))
            params.tile_counts = tile_counts.data_ptr()
        if out is None:
            shape = (width, height, 3) if layout == "wh3" else (height, width, 3)
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        else:
            _check_f32("out", out, dev)
            if not out.is_contiguous():
                raise ValueError("out must be contiguous")
            ow, oh = (out.shape[0], out.shape[1]) if layout == "wh3" else (out.shape[1], out.shape[0])
            params.out_x0, params.out_y0, params.out_w, params.out_h = int(out_origin[0]), int(out_origin[1]), int(ow), int(oh)
        cap_key = (image_idx, tile_size, None if tile_window is None else tuple(int(v) for v in tile_window),
                   semantics + ("/published" if published_rects else "") + ("/antialiased" if antialiased else ""))
        return _FramePlan(dev, n, cam, tensors, params, out, cap_key, owned_inputs, keep_alive)

    def _block_bounds(self, dev, n: int) -> Optional[torch.Tensor]:
        """``gaussians.block_bounds``, checked, or None: a strip's projection drops whole blocks of 256 rows of a spatially
        ordered scene after reading their box (recomputed here when points / scales were modified since)."""
        g = self.gaussians
        bb = g.current_block_bounds() if hasattr(g, "current_block_bounds") else getattr(g, "block_bounds", None)
        if bb is not None and (bb.device != dev or bb.dtype != torch.float32 or not bb.is_contiguous() or
                               tuple(bb.shape) != (-(-n // _ffi.GSX_BOUNDS_ROWS), 8)):
            raise ValueError("gaussians.block_bounds must be a contiguous float32 (%d, 8) tensor on %s "
                             "(Gaussians.refresh_block_bounds)" % (-(-n // _ffi.GSX_BOUNDS_ROWS), dev))
        return bb

    def _plan_substrips(self, params, dev, layout: str, substrips, substrip_events) -> list:
        """GsxParams.n_substrips, the bounds and one event per part; returns the host arrays ``params`` now points to."""
        k_parts = len(substrips) - 1
        bounds = (ctypes.c_int32 * (k_parts + 1))(*[int(v) for v in substrips])
        evs = self._part_events.setdefault((torch.cuda.current_stream(dev).cuda_stream, k_parts),
                                           [_hip.Event() for _ in range(k_parts)])
        handles = (ctypes.c_void_p * k_parts)(*[e.handle for e in evs])
        params.n_substrips, params.substrip_axis = k_parts, 0 if layout == "wh3" else 1
        params.substrip_bounds = ctypes.cast(bounds, ctypes.POINTER(ctypes.c_int32))
        params.substrip_events = ctypes.cast(handles, ctypes.POINTER(ctypes.c_void_p))
        if substrip_events is not None:
            substrip_events[:] = evs
        return [bounds, handles]

    def _view_state(self, plan, own: Optional[_OwnedFrame], tile_size, tile_window, semantics, generic_kernels, use_hints):
        """What earlier frames of this view left for the call, from the scene's dictionaries or from the frame's own record,
        into ``plan.params`` (kept_hint, the plain-footprints and row-class flags, hints).  Returns (pair capacity, hints slot)."""
        params, cap_key, dev, rec = plan.params, plan.cap_key, plan.dev, own if own is not None else _UNOWNED
        # pair capacity: 1.1 x the count this (camera, tile size, window, semantics) produced last time
        # -- the binning kernels' grids are sized by it -- or a generous guess for a first frame
        cap = int(rec.cap) if rec.cap is not None else \
            self._cap_hints.get(cap_key, 0) or max(self._instances_hint, 8 * plan.n + 4096)
        if rec.inputs is not None:  # capture_frame: the tensors whose addresses the graph bakes in stay alive with it
            g = self.gaussians
            scene_own = [g.points, g.scales, g.quaternions, g.opacity, g.sh if plan.tensors[4] is None else g.colors]
            if any(t.data_ptr() != a.data_ptr() for t, a in zip(plan.owned_inputs, scene_own)):
                raise ValueError("capture_frame needs contiguous float32 Gaussian tensors: a captured frame replays "
                                 "from the scene's own memory, and a non-contiguous attribute would be copied once, "
                                 "at capture time")
            rec.inputs[:] = plan.owned_inputs
        # how many Gaussians reached a tile of this window last time: picks the depth-sort route (a hint)
        params.kept_hint = int(rec.kept if rec.kept is not None else self._kept_hints.get(cap_key, 0))
        # GSX_FLAG_PLAIN_FOOTPRINTS: no tile of the last frame of this view held an ill-conditioned footprint, so this one runs
        # the compositing instance that cannot evaluate them -- where that pays: from _PLAIN_MIN_TILES tiles (measured: 6 %
        # of a 4K frame of 5M Gaussians, nothing at 1080p); its own n_redo says whether that held (_next_attempt /
        # confirm_frames / CapturedFrame.confirm: a frame that was wrong about it is rendered again without the flag)
        # (not _window_tiles: the threshold was measured against THIS count, the window as given or the frame's ceil-division)
        n_window_tiles = (tile_window[1] - tile_window[0]) * (tile_window[3] - tile_window[2]) if tile_window is not None \
            else (-(-plan.cam.width // tile_size) * -(-plan.cam.height // tile_size) if tile_size > 0 else 0)
        plain = bool(rec.plain) if rec.plain is not None else \
            (self._n_redo_seen.get(cap_key) == 0 and n_window_tiles >= _PLAIN_MIN_TILES)
        if plain and semantics == "ref_cpu" and tile_size == 16 and not generic_kernels:
            params.flags |= _ffi.GSX_FLAG_PLAIN_FOOTPRINTS
        # capture_frame: the row class (GSX_FLAG_SMALL_BATCH / _ONE_VISIBLE) the view's uncaptured frame ended up with is
        # baked into the graph -- a captured call cannot be issued again when n_visible says it assumed wrongly
        params.flags |= int(rec.rows_flag)
        if not use_hints:
            return cap, None
        # GsxParams.hints: one buffer per view and stream (a captured frame owns its own), valid once a frame has filled it
        hint_slot = rec.hints
        if hint_slot is None:
            hkey = (cap_key, torch.cuda.current_stream(dev).cuda_stream)
            hint_slot = self._hints.lookup(hkey)
            hbytes = _ffi.load().gsx_hints_bytes(plan.cam.width, plan.cam.height, tile_size)
            if hint_slot is None or hint_slot[0].numel() != hbytes or hint_slot[0].device != dev:
                hint_slot = self._hints.store(hkey, [torch.zeros(hbytes, dtype=torch.uint8, device=dev), False])
        params.hints = hint_slot[0].data_ptr()
        if hint_slot[1]:
            params.flags |= _ffi.GSX_FLAG_HINTS_VALID
        return cap, hint_slot

    def _issue(self, plan, own: Optional[_OwnedFrame], cap: int, tile_size: int, semantics: str, speculative: bool):
        """gsx_render_forward until ``_next_attempt`` says done (each of its reasons at most once or twice); raises for what it
        ended with.  Returns (pinned slot or None, GsxFrameStats): a speculative frame's counts arrive later, in pinned memory."""
        lib = _ffi.load()
        dev, n, cam, params = plan.dev, plan.n, plan.cam, plan.params
        own_ws, pinned = (None, None) if own is None else (own.workspace, own.pinned)
        if speculative:
            params.flags |= _ffi.GSX_FLAG_NO_SYNC
            if pinned is None:
                if len(self._pending) >= _PINNED_SLOTS:
                    self.confirm_frames()
                pinned = self._pinned_slot()
            st = _frame_stats(pinned)
        else:
            pinned, st = None, _ffi.GsxFrameStats()
        with torch.cuda.device(dev):
            for _ in range(6):
                nbytes = lib.gsx_workspace_bytes(n, cam.width, cam.height, tile_size, cap)
                if nbytes == 0:
                    raise _ffi.GsxError(_ffi.GSX_ERR_INVALID_ARGUMENT, "gsx_workspace_bytes rejected the sizes")
                ws = _WORKSPACE.get(dev, nbytes) if own_ws is None else own_ws
                if ws.numel() < nbytes:
                    raise ValueError("private workspace holds %d bytes, the frame needs %d" % (ws.numel(), nbytes))
                # hand over exactly the bytes of `cap` pairs (the buffer may be larger): the library
                # derives its pair capacity -- and the binning grids -- from the size it is given
                rc = lib.gsx_render_forward(ctypes.byref(cam), *[_ptr(t) for t in plan.tensors], n, tile_size, _ptr(plan.out),
                                            ctypes.byref(params), ctypes.byref(st), _ptr(ws), nbytes, _stream_handle(dev))
                what, value = _next_attempt(rc, int(st.n_visible), int(st.n_instances), int(st.n_redo), params.flags, n,
                                            speculative, own is not None, own is not None and own.cap is not None, semantics)
                if what == "done":
                    break
                if what == "flags":
                    params.flags = value
                else:
                    cap = value
        _ffi.check(rc)
        return pinned, st

    def _walk_lists(self, image_idx: int, tile_size: int, layout: str, semantics: str, n_instances: int, prepare):
        """The frame of every call that walks the forward's lists again (``_render_backward``, ``_render_depth``,
        ``_render_contribution``): the scene's inputs, detached, the view's camera and the frame's params; then
        ``prepare(lib, dev, n, cam, params)``, which sets the call's flags, checks and makes what is the call's own and
        returns (size function, what to say when it returns 0, entry, its arguments between ``tile_size`` and ``params``
        -- tensors, None or ints --, the result); then the workspace for ``n_instances + 4096`` pairs, the call, its
        check.  Returns the result."""
        lib = _ffi.load()
        with torch.no_grad():
            dev, n, tensors = self._inputs(image_idx)
            tensors = [t.detach() for t in tensors]
            cam = self.images[image_idx].gsx_camera()
            params, _ = self._frame_params(dev, n, layout, semantics)
            size_fn, rejected, entry, args, result = prepare(lib, dev, n, cam, params)
            cap = int(n_instances) + 4096
            with torch.cuda.device(dev):
                nbytes = size_fn(n, cam.width, cam.height, tile_size, cap)
                if nbytes == 0:
                    raise _ffi.GsxError(_ffi.GSX_ERR_INVALID_ARGUMENT, rejected)
                ws = _WORKSPACE.get(dev, nbytes)
                rc = entry(ctypes.byref(cam), *[_ptr(t) for t in tensors], n, tile_size,
                           *[a if isinstance(a, int) else _ptr(a) for a in args], ctypes.byref(params), _ptr(ws), nbytes,
                           _stream_handle(dev))
            _ffi.check(rc)
        return result

    def _render_backward(self, image_idx: int, tile_size: int, layout: str, frame: torch.Tensor, grad_frame: torch.Tensor,
                         n_instances: int, n_visible: int, flags: int = 0, geometry: bool = False,
                         screen: bool = False, camera: bool = False, depth: Optional[torch.Tensor] = None,
                         grad_depth: Optional[torch.Tensor] = None, screen_abs: bool = False,
                         std: Optional[tuple] = None) -> Tuple[torch.Tensor, ...]:
        """gsx_render_backward: (dL/dcolors (N,3), dL/dopacity (N,1)) of the ref_cpu frame ``frame`` for dL/dframe =
        ``grad_frame``; with ``geometry`` gsx_render_backward_geometry: those two and (dL/dpoints (N,3), dL/dscales (N,3),
        dL/dquaternions (N,4)); with ``screen`` besides gsx_render_backward_screen: those five and (dL/d(NDC mean) (N,2),
        screen radius (N,1)); with ``camera`` (with or without ``screen``) gsx_render_backward_camera: the same, and last
        (dL/dworld2view (4,4), dL/dfull_proj (4,4)), the two matrices as independent inputs.  With ``depth`` (needs
        ``geometry``, excludes ``camera``) gsx_render_backward_depth: the screen entry's outputs -- the five, or with
        ``screen`` the seven -- for L(frame, depth image), ``depth`` the image ``_render_depth`` returned and ``grad_depth``
        dL/d(that image).  With ``screen_abs`` (needs ``geometry`` and ``screen``, excludes ``camera`` and ``depth``)
        gsx_render_backward_screen_abs: the seven and (the absolute screen statistic (N,2)).
        With ``std`` = (background, published_rects, antialiased) (excludes ``camera``, ``depth`` and ``screen_abs``) ``frame`` is the
        std_3dgs frame rendered with those three and the one call is gsx_render_backward_std: the two, the five or the seven.
        The projection, depth order and binning run again in the library (the same lists as the
        forward's); the scene's hints buffers are not touched.  ``flags``: GSX_FLAG_* added to the call's own (the test
        library's stage times: GSX_FLAG_TIMING, tools/bench_backward.py)."""
        def prepare(lib, dev, n, cam, params):
            if std is None:
                params.flags |= _ffi.rows_flag(n, n_visible) | int(flags)     # the row class the forward ended up with
            else:
                if camera or depth is not None or screen_abs:
                    raise ValueError("std excludes camera, depth and screen_abs: gsx_render_backward_std has none of them")
                params.background[0], params.background[1], params.background[2] = [float(v) for v in std[0]]
                params.flags |= int(flags) | (_ffi.GSX_FLAG_PUBLISHED_RECTS if std[1] else 0) | \
                    (_ffi.GSX_FLAG_ANTIALIASED if len(std) > 2 and std[2] else 0)
            gf = _check_f32("grad_frame", grad_frame.detach(), dev)
            img = _check_f32("frame", frame.detach(), dev)
            if tuple(gf.shape) != tuple(img.shape):
                raise ValueError("grad_frame has shape %s, the frame %s" % (tuple(gf.shape), tuple(img.shape)))
            gc = torch.empty((n, 3), dtype=torch.float32, device=dev)
            go = torch.empty((n, 1), dtype=torch.float32, device=dev)
            outs = [gc, go]
            if screen_abs and (not geometry or not screen or camera or depth is not None):
                raise ValueError("screen_abs needs geometry and screen and excludes camera and depth: only "
                                 "gsx_render_backward_screen_abs has the absolute statistic")
            if geometry:
                outs += [torch.empty((n, k), dtype=torch.float32, device=dev)
                         for k in (3, 3, 4) + ((2, 1) if screen else ()) + ((2,) if screen_abs else ())]
            elif screen or camera:
                raise ValueError("screen and camera need geometry: both come out of the geometry backward")
            if depth is not None:
                if not geometry or camera:
                    raise ValueError("depth needs geometry and excludes camera: gsx_render_backward_depth has no pose gradient")
                dimg = _check_f32("depth", depth.detach(), dev)
                gd = _check_f32("grad_depth", grad_depth.detach(), dev)
                if tuple(gd.shape) != tuple(dimg.shape) or tuple(dimg.shape) != tuple(img.shape[:2]) + (2,):
                    raise ValueError("depth has shape %s and grad_depth %s, the frame %s" % (tuple(dimg.shape), tuple(gd.shape),
                                                                                          tuple(img.shape)))
            size_fn = lib.gsx_backward_geometry_workspace_bytes if geometry else lib.gsx_backward_workspace_bytes
            entry = (lib.gsx_render_backward_screen if screen else lib.gsx_render_backward_geometry) if geometry \
                else lib.gsx_render_backward
            if screen_abs:
                entry = lib.gsx_render_backward_screen_abs
            args = outs
            if camera:
                cam_outs = [torch.empty((4, 4), dtype=torch.float32, device=dev) for _ in range(2)]
                args = outs + ([] if screen else [None, None]) + cam_outs       # grad_means2d, screen_radius: NULL
                outs = outs + cam_outs
                size_fn, entry = lib.gsx_backward_camera_workspace_bytes, lib.gsx_render_backward_camera
            if depth is not None:
                args = outs + ([] if screen else [None, None]) + [dimg, gd]     # grad_means2d, screen_radius: NULL
                size_fn, entry = lib.gsx_backward_depth_workspace_bytes, lib.gsx_render_backward_depth
            if std is not None:     # one entry: NULL for the outputs that were not asked for
                args = outs + [None] * (7 - len(outs))
                size_fn, entry = lib.gsx_backward_std_workspace_bytes, lib.gsx_render_backward_std
            return size_fn, "the backward workspace function rejected the sizes", entry, [img, gf] + args, tuple(outs)

        return self._walk_lists(image_idx, tile_size, layout, "ref_cpu" if std is None else "std_3dgs", n_instances, prepare)

    def _render_depth(self, image_idx: int, tile_size: int, layout: str, n_instances: int, n_visible: int) -> torch.Tensor:
        """gsx_render_depth: the (D, A) image of the whole ref_cpu frame, (W,H,2) for ``layout`` "wh3" and (H,W,2) for "hw3";
        ``n_instances`` and ``n_visible`` are the frame's counts (its workspace and row class)."""
        def prepare(lib, dev, n, cam, params):
            params.flags |= _ffi.rows_flag(n, n_visible)
            shape = (cam.width, cam.height, 2) if layout == "wh3" else (cam.height, cam.width, 2)
            out = torch.empty(shape, dtype=torch.float32, device=dev)
            return lib.gsx_depth_workspace_bytes, "gsx_depth_workspace_bytes rejected the sizes", lib.gsx_render_depth, [out], out

        return self._walk_lists(image_idx, tile_size, layout, "ref_cpu", n_instances, prepare)

    def render_image_depth_hip(self, image_idx: int, tile_size: int = 16, layout: str = "wh3",
                               screen_statistics: bool = False, stats: Optional[dict] = None):
        """``(frame, depth)`` of the whole ref_cpu frame.  ``frame`` is ``render_image_hip``'s, bit for bit; ``depth`` has
        the frame's two leading axes and a last axis of 2: expected depth ``D = sum T alpha z`` and coverage
        ``A = sum T alpha`` (gsx_render_depth; ``z`` the view-space depth, ``D`` not divided by ``A`` -- write ``D / A``
        in torch where it is wanted).  Under ``no_grad``, or when none of ``points``, ``scales``, ``quaternions``,
        ``opacity``, ``colors`` / ``sh`` requires grad, neither has a ``grad_fn``.  Otherwise both come out of one autograd
        function whose ``backward`` runs gsx_render_backward_depth once, for whichever of dL/dframe and dL/ddepth arrived
        (a missing one counts as zeros), and delivers gradients to those of the five arrays that require grad: the
        geometry gradients need no opt-in here.  ``screen_statistics=True`` leaves ``scene.screen_statistics`` as
        ``render_image_hip(..., screen_statistics=True)`` does, depth's share included.  An SH scene's dL/dcolour goes
        through gsx_sh_backward as for the frame (depth adds nothing to it).  The refusals of the frame's gradient path
        apply with or without gradients; a view whose ``world2view`` requires grad is refused: the pose has no gradient
        through depth yet."""
        if layout not in ("wh3", "hw3"):
            raise ValueError("layout must be 'wh3' or 'hw3', got %r" % (layout,))
        if _screen_mode(screen_statistics) == "abs":
            raise ValueError("screen_statistics='abs' is not available in render_image_depth_hip: gsx_render_backward_depth "
                             "has no absolute statistic; pass screen_statistics=True, or render the frame with render_image_hip")
        g = self.gaussians
        for what, bad in _refusals(g):
            if bad:
                _refuse_with_grad(what)
        if torch.is_grad_enabled() and getattr(self.images[image_idx].world2view, "requires_grad", False):
            raise ValueError("render_image_depth_hip has no pose gradient: world2view of image %r requires grad, and the "
                             "gradient through depth (Sz [p, 1] into a column of dL/dworld2view) is not implemented; "
                             "detach the pose or render the frame with render_image_hip(camera_gradients=True)" % (image_idx,))
        if _wants_grad(g, True):
            kw = dict(stats=stats, screen_statistics=bool(screen_statistics))
            return _RenderImageDepthFunction.apply(self, image_idx, tile_size, layout, kw, g.points, g.scales, g.quaternions,
                                                   g.opacity, g.colors, getattr(g, "sh", None))
        with torch.no_grad():
            st = {}
            frame = self.render_image_hip(image_idx, tile_size=tile_size, layout=layout, stats=st)
            if stats is not None:
                stats.update(st)
            return frame, self._render_depth(image_idx, tile_size, layout, int(st["n_instances"]), int(st["n_visible"]))

    def _render_contribution(self, image_idx: int, tile_size: int, semantics: str, n_instances: int, n_visible: int,
                             out: Optional[Contribution] = None, published_rects: bool = False,
                             antialiased: bool = False) -> Contribution:
        """gsx_render_contribution on view ``image_idx``: a new ``Contribution`` (every row written), or ``out`` with the
        view merged into it (accumulate).  ``n_instances`` and ``n_visible`` are the counts of the view's frame under
        ``semantics`` (the workspace and the row class), as for ``_render_backward``."""
        def prepare(lib, dev, n, cam, params):
            if semantics == "ref_cpu":
                params.flags |= _ffi.rows_flag(n, n_visible)
            elif published_rects:
                params.flags |= _ffi.GSX_FLAG_PUBLISHED_RECTS
            if antialiased:
                params.flags |= _ffi.GSX_FLAG_ANTIALIASED
            if out is None:
                con = Contribution(torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
                                   torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
            else:
                con = out
                for name, t, dtype in zip(Contribution._fields, con, (torch.float32, torch.float32, torch.int32, torch.int32)):
                    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (n,) or t.device != dev \
                            or not t.is_contiguous():
                        raise ValueError("out.%s must be a contiguous %s tensor of shape (%d,) on %s: a Contribution of this "
                                         "container" % (name, dtype, n, dev))
            return (lib.gsx_contribution_workspace_bytes, "gsx_contribution_workspace_bytes rejected the sizes",
                    lib.gsx_render_contribution, list(con) + [0 if out is None else 1], con)

        return self._walk_lists(image_idx, tile_size, "wh3", semantics, n_instances, prepare)

    def render_contribution_hip(self, image_idx: int, semantics: str = "ref_cpu", tile_size: int = 16,
                                out: Optional[Contribution] = None, tile_window=None,
                                published_rects: bool = False, antialiased: bool = False) -> Contribution:
        """What every Gaussian contributes to the frame of view ``image_idx`` (gsx_render_contribution): a ``Contribution``
        of device tensors, one row per row of the container -- ``weight_max``, the largest blend weight ``T alpha`` the
        Gaussian reaches in any pixel (RadSplat's prune score), ``weight_sum``, the sum of its weights (the score
        LightGaussian and Mini-Splatting rank on), ``pixels``, the number of pixels that composited it, and ``views``, 1
        where the frame listed it on a tile.  ``semantics``: "ref_cpu" or "std_3dgs" (``published_rects`` and ``antialiased`` as for
        the frame -- the weights of the anti-aliased frame are T alpha with alpha = sigmoid * rho * G --;
        the background changes no weight).  The walk is the gradient entries' own: ``weight_sum`` is, bit for bit, what
        ``colors.grad[:, 0]`` is after ``frame.sum().backward()``.  ``out``: a ``Contribution`` of this container; the view
        is merged into it (max, +=, +=, views += 1; rows the view does not list are not touched) and it is returned.
        Refused by name: tensors that are not on the GPU (there is no CPU fallback), ``semantics="ref_cuda"``, a
        ``tile_window``.  The view's frame is rendered first, under ``no_grad``, for its counts -- the pair count that sizes the
        workspace and the visible count that names the row class, which reach the host as every frame's counts do -- so a
        call costs that frame (0.43 ms at 1080p and 1M Gaussians) on top of the pass; no tensor is read back."""
        _check_antialiased(antialiased, semantics)
        _require_gpu(self.gaussians.points.device)
        if semantics == "ref_cuda":
            raise ValueError("semantics='ref_cuda' has no contribution pass: gsx_render_contribution walks the gradient "
                             "entries' lists, and only the ref_cpu and std_3dgs frames have them")
        if semantics not in ("ref_cpu", "std_3dgs"):
            raise ValueError("semantics = %r is neither 'ref_cpu' nor 'std_3dgs'" % (semantics,))
        if tile_window is not None:
            raise ValueError("tile_window is not available in render_contribution_hip: gsx_render_contribution walks the "
                             "whole frame (no tile window, no strips)")
        if out is not None and not isinstance(out, Contribution):
            raise TypeError("out must be a Contribution, got %s" % type(out).__name__)
        with torch.no_grad():
            st: dict = {}
            kw = dict(semantics=semantics, published_rects=published_rects, antialiased=bool(antialiased)) \
                if semantics == "std_3dgs" else {}
            self.render_image_hip(image_idx, tile_size=tile_size, stats=st, **kw)
            return self._render_contribution(image_idx, tile_size, semantics, int(st["n_instances"]), int(st["n_visible"]),
                                             out=out, published_rects=published_rects, antialiased=bool(antialiased))

    def contribution(self, indices=None, semantics: str = "ref_cpu", tile_size: int = 16,
                     published_rects: bool = False, antialiased: bool = False) -> Contribution:
        """``render_contribution_hip`` swept over the views ``indices`` (default: every view of the scene, in the order of
        ``scene.images``): the maximum, the sums and the view count over all of them, one library call per view merging
        into the first view's arrays.  No tensor is read back to the host: per view, the frame rendered for its counts delivers
        those counts and the library call synchronises once, as the backward's does.  An empty ``indices`` is refused."""
        views = list(self.images) if indices is None else list(indices)
        if not views:
            raise ValueError("indices is empty: no view to measure a contribution in")
        for idx in views:
            if idx not in self.images:
                raise ValueError("indices names image %r, which the scene does not have" % (idx,))
        con = None
        for idx in views:
            con = self.render_contribution_hip(idx, semantics=semantics, tile_size=tile_size, out=con,
                                               published_rects=published_rects, antialiased=antialiased)
        return con

    def _sh_backward(self, image_idx: int, grad_colors: torch.Tensor,
                     with_points: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """gsx_sh_backward_active: (dL/dsh (N,K,3), exact zeros in the inactive bands; dL/dpoints (N,3) through the view
        direction, or None without ``with_points``) of this camera's view-dependent colours for dL/dcolour =
        ``grad_colors`` (N,3)."""
        lib = _ffi.load()
        g = self.gaussians
        with torch.no_grad():
            dev = g.points.device
            _require_gpu(dev)
            n = int(g.points.shape[0])
            pts = _check_f32("points", g.points.detach().reshape(n, 3), dev)
            sh, degree = self._sh_flat(n, dev)      # (under no_grad: nothing is recorded)
            gc = _check_f32("grad_colors", grad_colors.detach().reshape(n, 3), dev)
            gsh = torch.empty(sh.shape, dtype=torch.float32, device=dev)
            gview = torch.empty((n, 3), dtype=torch.float32, device=dev) if with_points else None
            center = (ctypes.c_float * 3)(*self.images[image_idx].camera_center_host)
            with torch.cuda.device(dev):
                rc = lib.gsx_sh_backward_active(_ptr(pts), _ptr(sh), degree, self._active_sh_degree(), n, center, _ptr(gc),
                                                _ptr(gsh), _ptr(gview), _stream_handle(dev))
            _ffi.check(rc)
        return gsh, gview

    def _note_count(self, cap_key, n_instances: int, n_kept: int = 0, n_redo: Optional[int] = None) -> None:
        self._instances_hint = max(self._instances_hint, int(n_instances * 1.1))
        self._cap_hints[cap_key] = int(n_instances * 1.1) + 4096
        self._kept_hints[cap_key] = max(1, int(n_kept))
        if n_redo is not None:
            self._n_redo_seen[cap_key] = int(n_redo)
        if cap_key[2] is None and cap_key[3] == "ref_cpu":
            self._last_instances = n_instances

    def _check_pose(self, image_idx) -> None:
        """``GaussianImage.set_world2view`` moved this view since its last frame: what the scene keeps for the view from
        earlier frames was measured at the old pose -- the pair capacity, the kept count, the n_redo count (which chooses
        GSX_FLAG_PLAIN_FOOTPRINTS) and the GsxParams.hints buffers (depth-sort splitters, tile schedule) of every tile
        size, window, rule set and stream.  All four are dropped for this view, so its next frame is a first frame.  The
        scene-wide workspace sizing stays: it is a size, not a statement about a pose."""
        version = getattr(self.images[image_idx], "pose_version", 0)
        if self._pose_seen.get(image_idx, 0) == version:
            return
        self._pose_seen[image_idx] = version
        for table in (self._cap_hints, self._kept_hints, self._n_redo_seen):
            for key in [k for k in table if k[0] == image_idx]:
                del table[key]
        for key in [k for k in self._hints if k[0][0] == image_idx]:
            del self._hints[key]

    def gaussians_changed(self) -> None:
        """Tell the scene that the ROWS of ``gaussians`` changed -- their number or which Gaussian a row holds
        (``DensityControl.densify_and_prune`` calls it; so does a user who replaces the arrays).  Everything the scene keeps
        per view from earlier frames was measured on the old rows: the pair capacities, the kept counts, the n_redo counts,
        the per-row hints buffers and the workspace sizing.  All of it is dropped, so the next frame of every view is a first
        frame."""
        self._cap_hints.clear()
        self._kept_hints.clear()
        self._n_redo_seen.clear()
        self._hints.clear()
        self._instances_hint = 0
        self._last_instances = 0
        self.screen_statistics = None       # its rows were the old rows

    # ------------------------------------------------------------------ the world's frame
    def _move_views(self, sim) -> None:
        """Every view follows the world transform ``sim`` (x' = s R x + t) so that it sees what it saw.  With the view's
        rigid pose x_view = Rc x + T (``world2view`` is its transpose, row-vector convention): x = R^T (x' - t) / s, and the
        new RIGID pose is the one with x'_view = s x_view: Rc' = Rc R^T (orthonormal: s is not folded into it),
        T' = s T - Rc' t; the last column of ``world2view`` stays (0, 0, 0, 1).  Float64 on the host, rounded once."""
        import numpy as np

        for image in self.images.values():
            V = image.world2view.detach().to("cpu", torch.float64).numpy()
            Rc, T = V[:3, :3].T, V[3, :3]
            Rn = Rc @ sim.R.T
            W = np.zeros((4, 4))
            W[:3, :3] = Rn.T
            W[3, :3] = sim.s * T - Rn @ sim.t
            W[3, 3] = 1.0
            image.set_world2view(torch.from_numpy(W.astype(np.float32)))

    def transform(self, R, s: float = 1.0, t=None):
        """Re-expresses the whole scene in the world ``x' = s R x + t``: the Gaussians (``Gaussians.transform``: one
        gsx_transform_gaussians launch) AND every view (``set_world2view``), so that every frame is unchanged -- up to
        rounding, and up to the discrete decisions rounding can flip (a tile rectangle's edge, a cull, a depth tie).
        View space is SCALED by ``s``: view-space depths, ``render_image_depth_hip``'s D, and the distances the near
        (z_view >= 0.2) and far tests compare all grow by ``s``; coverage does not change.  ``depth_targets`` of a fit are
        the caller's to scale.  Everything kept per view from earlier frames is dropped (``gaussians_changed``); a frame
        captured earlier (``capture_frame``) has the old camera baked in: capture it again, or ``set_camera`` one that was
        captured with ``movable_camera=True``.  Adam
        moments, ``DensityControl`` / ``MCMCControl`` statistics and thresholds are not touched: transform before a fit or
        after one.  Returns the validated ``transform.Similarity`` (unpacks as ``(R, s, t)``)."""
        from .transform import similarity

        sim = similarity(R, s, t)
        self.gaussians.transform(*sim)
        self._move_views(sim)
        self.gaussians_changed()
        return sim

    def cameras_extent(self):
        """``(center, radius)``: the normalisation of the published 3D Gaussian Splatting trainer -- the mean of the camera
        centres (float64 numpy, (3,)) and 1.1 x the largest distance of a camera centre from it (a float)."""
        import numpy as np

        centers = np.array([image.camera_center_host for image in self.images.values()], dtype=np.float64).reshape(-1, 3)
        center = centers.mean(axis=0)
        radius = 1.1 * float(np.sqrt(((centers - center[None, :]) ** 2).sum(axis=1)).max())
        return center, radius

    def normalize(self):
        """Moves the scene into the frame the published trainer's rates and thresholds are quoted in: the camera centres'
        mean at the origin and ``cameras_extent()[1] == 1`` (``s = 1 / radius``, ``t = -center / radius``, ``R = I``).
        ``DEFAULT_LR``'s position rate, ``DensityControl(dense_scale=, prune_scale=)`` and ``MCMCControl(noise_lr=)`` then
        apply as quoted.  Returns the triple: ``scene.transform(*transform.inverse(triple))`` puts the scene back, before
        ``save_trained`` for instance.  Refused when all cameras share one centre (radius 0)."""
        import numpy as np

        center, radius = self.cameras_extent()
        if not radius > 0.0:
            raise ValueError("cameras_extent() has radius %r: the scene has no extent to normalise by" % (radius,))
        return self.transform(np.eye(3), 1.0 / radius, -center / radius)

    def _pinned_slot(self) -> torch.Tensor:
        """One 64-byte slot of a pinned ring (pinning memory per frame would dominate the frame)."""
        if self._pinned_pool is None:
            self._pinned_pool = torch.zeros((_PINNED_SLOTS, ctypes.sizeof(_ffi.GsxFrameStats)),
                                            dtype=torch.uint8).pin_memory()
        slot = self._pinned_pool[self._pinned_next % _PINNED_SLOTS]
        self._pinned_next += 1
        slot.zero_()
        return slot

    def confirm_frames(self) -> int:
        """Synchronises and validates every frame rendered with ``no_sync=True`` since the last call.
        A frame whose pair count exceeded the capacity of the workspace it was enqueued with (pairs
        were dropped) is rendered again on the normal path into the same output tensor.  Returns the
        number of re-renders."""
        if not self._pending:
            return 0
        torch.cuda.synchronize(self.gaussians.points.device)
        pending, self._pending = self._pending, []
        return sum(self._settle(frame) for frame in pending)

    def _settle(self, frame) -> bool:
        """The counts a ``no_sync`` frame left in its pinned slot (the caller has synchronised): filed for the view's next
        frame; pairs dropped or tiles left undone: rendered again, synchronously, into the same tensor.  Returns whether."""
        st = _frame_stats(frame.pinned)
        self._note_count(frame.cap_key, int(st.n_instances), int(st.n_kept), int(st.n_redo))
        # more pairs than the workspace held (dropped), or tiles left to a second compositing launch that was not issued
        again = bool(st.n_instances > st.reserved or (frame.ran_plain and st.n_redo > 0))
        if again:
            self.render_image_hip(**frame.call)
        return again

    def capture_frame(self, image_idx: int, tile_size: int = 16, layout: str = "wh3",
                      semantics: str = "ref_cpu", movable_camera: bool = False,
                      headroom: float = 1.1, antialiased: bool = False) -> "CapturedFrame":
        """Records one whole frame of this camera (every launch, clear and the asynchronous count
        copy) into a hipGraph.  ``frame.replay()`` then re-renders it with ONE graph launch (~20 us
        of host time instead of ~120 us for ~30 separate launches) from the CURRENT contents of the
        Gaussian tensors -- all buffer addresses are baked in, and so are the camera constants unless
        ``movable_camera`` is set: then the projection kernel reads them from a device buffer
        (GsxParams.camera_device) that ``frame.set_camera(other_image_idx)`` rewrites between replays
        (same frame size; SH scenes too: the colour is evaluated inside the projection kernel with the
        camera centre of that buffer).  The graph holds room for ``headroom`` x the pair count of the captured view; a replay
        that needs more (another camera may) is reported by ``confirm()``.  Possible because the
        no-sync frame has no host dependency at all.  ``antialiased``: as in ``render_image_hip`` (std_3dgs only); the graph
        bakes the mode in."""
        _check_antialiased(antialiased, semantics)
        if _wants_grad(self.gaussians):
            _refuse_with_grad("capture_frame")
        if self._sh_truncated():
            raise ValueError("capture_frame with gaussians.active_sh_degree = %d below sh_degree = %d: the graph would bake in "
                             "a buffer of colours evaluated now, which goes stale with the next step; raise "
                             "active_sh_degree to sh_degree first"
                             % (self._active_sh_degree(), int(self.gaussians.sh_degree)))
        dev = self.gaussians.points.device
        _require_gpu(dev)
        cam = self.images[image_idx].gsx_camera()
        shape = (cam.width, cam.height, 3) if layout == "wh3" else (cam.height, cam.width, 3)
        out = torch.empty(shape, dtype=torch.float32, device=dev)
        cam_buf = None
        if movable_camera:
            cam_buf = torch.frombuffer(bytearray(bytes(cam)), dtype=torch.uint8).to(dev)
        kw = dict(tile_size=tile_size, layout=layout, out=out, semantics=semantics, camera_buffer=cam_buf)
        if antialiased:
            kw["antialiased"] = True
        st = {}
        self.render_image_hip(image_idx, stats=st, **kw)    # normal path: the pair count of this view
        # What the graph bakes in belongs to this frame alone: the pair capacity the recorded launches are
        # sized for (headroom x this view's count), a scratch buffer of exactly that size and a pinned
        # slot for the counts.  None of them comes from (or goes back to) the scene's shared pools.
        lib = _ffi.load()
        n = int(self.gaussians.points.shape[0])
        cap = int(st["n_instances"] * max(float(headroom), 1.0)) + 4096
        nbytes = lib.gsx_workspace_bytes(n, cam.width, cam.height, tile_size, cap)
        if nbytes == 0:
            raise _ffi.GsxError(_ffi.GSX_ERR_INVALID_ARGUMENT, "gsx_workspace_bytes rejected the sizes")
        # the graph bakes in which compositing instance runs: the plain one (GSX_FLAG_PLAIN_FOOTPRINTS) only for a fixed camera
        # whose frame held no ill-conditioned footprint, where it pays (confirm() checks every replay's n_redo); a movable
        # camera may turn to such footprints
        own = _OwnedFrame(
            cap=cap, workspace=torch.empty(nbytes, dtype=torch.uint8, device=dev), kept=int(st["n_kept"]),
            rows_flag=0 if semantics == "std_3dgs" else _ffi.rows_flag(n, int(st["n_visible"])),
            plain=(not movable_camera) and int(st.get("n_redo", 1)) == 0 and int(st.get("n_tiles", 0)) >= _PLAIN_MIN_TILES,
            pinned=torch.zeros(ctypes.sizeof(_ffi.GsxFrameStats), dtype=torch.uint8).pin_memory(), inputs=[],
            hints=[torch.zeros(lib.gsx_hints_bytes(cam.width, cam.height, tile_size), dtype=torch.uint8, device=dev), False])
        stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(stream):   # the same call once on the capture stream, outside the capture
            self.render_image_hip(image_idx, _private=own, **kw)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            self.render_image_hip(image_idx, no_sync=True, _private=own, **kw)
        call = dict(image_idx=image_idx, **kw)
        frame = CapturedFrame(self, graph, out, own.pinned, call, camera_buffer=cam_buf, workspace=own.workspace,
                              capacity=cap, inputs=own.inputs)
        frame._hints = own.hints[0]     # the recorded kernels read and refresh this buffer on every replay
        frame._plain_footprints = bool(own.plain)
        return frame

    def render_image(self, image_idx: int, tile_size: int = 16, geometry_gradients: bool = False,
                     screen_statistics: bool = False, camera_gradients: bool = False) -> torch.Tensor:
        """(W,H,3) float32 indexed [x,y]; same result as the reference's pure-Python
        ``render_image`` (gaussian_scene.py:200-238), computed on the GPU and -- like the reference,
        whose image is a CPU tensor (gaussian_scene.py:206) -- returned in host memory, so that
        ``plt.imshow(scene.render_image(i))`` keeps working.  ``render_image_hip`` is the same frame
        left on the device.  ``geometry_gradients``, ``screen_statistics``, ``camera_gradients``: as in
        ``render_image_hip``."""
        frame = self.render_image_hip(image_idx, tile_size=tile_size, layout="wh3", geometry_gradients=geometry_gradients,
                                      screen_statistics=screen_statistics, camera_gradients=camera_gradients)
        # page-locked destination (torch's caching host allocator keeps the pages registered between
        # calls): the copy runs at PCIe rate instead of through a pageable staging loop
        host = torch.empty(frame.shape, dtype=frame.dtype, pin_memory=True)
        host.copy_(frame, non_blocking=True)
        torch.cuda.current_stream(frame.device).synchronize()
        return host

    render = render_image  # the name BASELINE.json's north star uses

    def rendered_region(self, image_idx: int, tile_size: int = 16, layout: str = "wh3",
                        semantics: str = "ref_cpu") -> Tuple[int, int]:
        """Extent (a, b) of what a ``ref_cpu`` frame of this camera renders, in the order of the frame's two leading axes:
        whole tiles from the origin, the last tile row and column left out (``strips.tiles_along``).  Everything outside is
        the zeros the frame was cleared to -- not a rendering of black.  ``semantics="std_3dgs"``: the whole frame (that
        rule set renders partial edge tiles)."""
        if layout not in ("wh3", "hw3"):
            raise ValueError("layout must be 'wh3' or 'hw3', got %r" % (layout,))
        cam = self.images[image_idx].gsx_camera()
        if semantics == "std_3dgs":
            return (int(cam.width), int(cam.height)) if layout == "wh3" else (int(cam.height), int(cam.width))
        if semantics != "ref_cpu":
            raise ValueError("rendered_region knows the ref_cpu and std_3dgs frames, not semantics=%r" % (semantics,))
        w = tiles_along(int(cam.width), int(tile_size)) * int(tile_size)
        h = tiles_along(int(cam.height), int(tile_size)) * int(tile_size)
        return (w, h) if layout == "wh3" else (h, w)

    def photometric_loss(self, image_idx: int, frame: torch.Tensor, target: torch.Tensor, tile_size: int = 16,
                         lambda_dssim: float = 0.2, layout: str = "wh3", terms: Optional[dict] = None,
                         weight: Optional[torch.Tensor] = None, exposure: Optional[torch.Tensor] = None,
                         semantics: str = "ref_cpu") -> torch.Tensor:
        """``loss.photometric_loss`` of a ``ref_cpu`` frame of this camera against ``target`` over ``rendered_region``: the
        rim no tile covers takes no part and receives an exact zero gradient.  ``weight`` (a per-pixel weight of the frame's
        two leading axes) and ``exposure`` (a (3, 4) colour transform of the frame) are passed through as they are.
        ``semantics="std_3dgs"``: the frame is a std_3dgs frame and the region is all of it."""
        region = self.rendered_region(image_idx, tile_size, layout, semantics)
        if region[0] <= 0 or region[1] <= 0:
            raise ValueError("a %s frame of camera %r has no rendered tile at tile_size %d (extent <= tile)" % (
                layout, image_idx, tile_size))
        if weight is None and exposure is None:
            return photometric_loss(frame, target, lambda_dssim=lambda_dssim, region=region, terms=terms)
        return photometric_loss(frame, target, lambda_dssim=lambda_dssim, region=region, terms=terms, weight=weight,
                                exposure=exposure)

    def render_images(self, image_indices, tile_size: int = 16):
        """``render_image`` for a sequence of cameras -- the reference's own loop renders one image index after another
        (splat/gaussian_scene.py:200-203) --, as a generator of (W,H,3) HOST tensors with the device-to-host copy of
        frame i overlapped with the rendering of frame i + 1: two device frames and two page-locked host buffers take
        turns, the copy runs on a stream of its own behind an event.  A frame's host tensor stays valid until the
        generator has yielded two more (copy it if it has to live longer).  At 1M Gaussians / 1080p the 25 MB copy
        is longer than the render (0.36 ms): the loop runs at the copy's pace, 0.68 ms per frame measured, where
        ``render_image`` called per frame pays render + copy + two synchronisations, 0.97-1.02 ms (bench.py: host_frames)."""
        if _wants_grad(self.gaussians):
            _refuse_with_grad("render_images")
        dev = self.gaussians.points.device
        _require_gpu(dev)
        copy_stream = torch.cuda.Stream(dev)
        frames, hosts, copied, checks, pending = [None, None], [None, None], [None, None], [None, None], None

        def finish(k: int) -> torch.Tensor:
            copied[k].synchronize()
            if checks[k] is not None and self._settle(checks[k]):    # dropped pairs / tiles left undone: rendered once more
                hosts[k].copy_(frames[k])
            return hosts[k]

        for n, idx in enumerate(image_indices):
            k = n & 1
            cam = self.images[idx].gsx_camera()
            shape = (cam.width, cam.height, 3)
            if frames[k] is None or tuple(frames[k].shape) != shape:
                frames[k] = torch.empty(shape, dtype=torch.float32, device=dev)
                hosts[k] = torch.empty(shape, dtype=torch.float32, pin_memory=True)
            if copied[k] is not None:
                torch.cuda.current_stream(dev).wait_event(copied[k])     # the copy that last read this device frame
            # enqueued without waiting for the device (GSX_FLAG_NO_SYNC: the pair list is sized by this view's last count);
            # the counts land in pinned memory before the copy below has finished and are looked at when the frame is
            # handed out -- a frame that needed more pairs than it was given room for is rendered again, synchronously
            self.render_image_hip(idx, tile_size=tile_size, layout="wh3", out=frames[k], no_sync=True)
            checks[k] = self._pending.pop() if self._pending else None
            done = torch.cuda.current_stream(dev).record_event()
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(done)
                hosts[k].copy_(frames[k], non_blocking=True)
                copied[k] = copy_stream.record_event()
            if pending is not None:                 # hand out the frame before this one: its copy ran under this render
                yield finish(pending)
            pending = k
        if pending is not None:
            yield finish(pending)

    def compile_cuda_ext(self) -> NativeExtension:
        """The reference's drop-in boundary (splat/gaussian_scene.py:240-261): returns an object whose
        ``render_image(image_height, image_width, tile_size, point_means, point_colors, inverse_covariance_2d,
        min_x, max_x, min_y, max_y, opacity)`` is the native entry point.  Nothing is compiled here (libgsx.so is
        built ahead of time by hipcc for gfx950); the call costs nothing and may be repeated per frame as the
        reference does."""
        return NativeExtension()

    def render_image_cuda(self, image_idx: int, tile_size: int = 16) -> torch.Tensor:
        """(H,W,3) float32 indexed [y,x] with the semantics of the reference's CUDA kernel
        (``render_image_cuda``, splat/gaussian_scene.py:263-285 -> splat/c/render.cu): the same flow as the
        reference, call for call -- ``preprocess``, ``compile_cuda_ext``, the native ``render_image`` on the
        stage-1 arrays, one device synchronisation."""
        pre = self.preprocess(image_idx)
        height, width = self.images[image_idx].height, self.images[image_idx].width
        ext = self.compile_cuda_ext()
        image = ext.render_image(height, width, tile_size, pre.points.contiguous(), pre.colors.contiguous(),
                                 pre.inverse_covariance_2d.contiguous(), pre.min_x.contiguous(), pre.max_x.contiguous(),
                                 pre.min_y.contiguous(), pre.max_y.contiguous(), pre.sigmoid_opacity.contiguous())
        torch.cuda.synchronize(image.device)
        return image

    def render_preprocessed(self, image_idx: int, pre: PreprocessedScene, tile_size: int = 16,
                            layout: str = "wh3", stats: Optional[dict] = None) -> torch.Tensor:
        cam = self.images[image_idx].gsx_camera()
        return render_preprocessed(cam.height, cam.width, tile_size, pre.points, pre.colors,
                                   pre.inverse_covariance_2d, pre.min_x, pre.max_x, pre.min_y, pre.max_y,
                                   pre.sigmoid_opacity, layout=layout, stats=stats)

    # ------------------------------------------------------------------ debug helpers
    def render_points_image(self, image_idx: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """Projected (x_pix, y_pix, ndc_z) of the in-view points and their colours
        (gaussian_scene.py:44-51 -> image.py:72-89)."""
        return self.images[image_idx].project_point_to_camera_perspective_projection(
            self.gaussians.points, self.gaussians.colors)

    def get_2d_covariance(self, image_idx: int, points: torch.Tensor, covariance_3d: torch.Tensor) -> torch.Tensor:
        """(n,2,2) EWA covariance of ``points`` (n,3) with 3D covariances (n,3,3) under camera
        ``image_idx`` (gaussian_scene.py:53-68 -> utils.py:320-354), computed by gsx_covariance_2d."""
        lib = _ffi.load()
        dev = points.device
        _require_gpu(dev)
        n = int(points.shape[0])
        pts = _check_f32("points", points.reshape(n, 3), dev)
        cov = _check_f32("covariance_3d", covariance_3d.reshape(n, 3, 3), dev)
        out = torch.empty((n, 2, 2), dtype=torch.float32, device=dev)
        cam = self.images[image_idx].gsx_camera()
        with torch.cuda.device(dev):
            rc = lib.gsx_covariance_2d(ctypes.byref(cam), _ptr(pts), _ptr(cov), n, _ptr(out), _stream_handle(dev))
        _ffi.check(rc)
        return out
