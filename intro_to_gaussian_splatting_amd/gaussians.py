"""Gaussian parameter container with the reference's attribute layout (splat/gaussians.py:9-33).

``points (N,3)``, ``colors (N,3)`` = rgb/256, ``scales (N,3)`` linear (no exp), ``quaternions
(N,4)`` (w,x,y,z), ``opacity (N,1)`` logit -- float32 PyTorch-ROCm tensors resident in HBM.
Differences from the reference, on purpose: the constructor has no file side effect (the
reference writes ``point_cloud.ply``, gaussians.py:17-18) and does not track gradients on its own.
The reference's image IS differentiable -- with respect to ``colors`` and ``opacity`` only: its
Gaussian weight is a Python float (splat/utils.py:357-365, ``.item()``), which cuts every path
through the means and the covariances.  Here gradients are opt-in: ``g.colors.requires_grad_(True)``
and / or ``g.opacity.requires_grad_(True)``, and ``GaussianScene.render_image`` /
``render_image_hip`` then return a frame with a ``grad_fn`` whose backward runs in libgsx
(gsx_render_backward); points, scales and quaternions get no gradient, like the reference's
(``geometry_gradients=True`` delivers them).  An SH scene (``sh`` set) is differentiable when
``g.sh.requires_grad_(True)``: dL/dsh comes from gsx_sh_backward.  ``active_sh_degree`` (0..``sh_degree``, default
``sh_degree``) is the SH degree schedule of a fit: only the bands up to it are evaluated and differentiated, the arrays keep
the stored layout (gsx_sh_to_rgb_active, gsx_sh_backward_active).
"""
from __future__ import annotations

from typing import Optional

import torch


SH_C0 = 0.28209479177387814      # Y_0: colour = 0.5 + SH_C0 sh[0] at degree 0 (csrc/gsx_sh_device.h)


class Gaussians:
    def __init__(self, points: torch.Tensor, colors: torch.Tensor, model_path: str = ".",
                 device: Optional[str] = None) -> None:
        dev = torch.device(device) if device is not None else torch.device(
            "cuda" if torch.cuda.is_available() else "cpu")
        self.device = dev
        self.model_path = model_path
        n = points.shape[0]
        f32 = torch.float32
        self.points = torch.as_tensor(points).detach().to(dev, f32).contiguous()
        self.colors = (torch.as_tensor(colors).detach().to(f32) / 256).to(dev).contiguous()
        self.scales = torch.full((n, 3), 0.001, dtype=f32, device=dev)          # gaussians.py:23
        self.quaternions = torch.zeros((n, 4), dtype=f32, device=dev)           # gaussians.py:29-30
        self.quaternions[:, 0] = 1.0
        p = 0.9999 * torch.ones((n, 1), dtype=f32)                             # gaussians.py:31-33
        self.opacity = torch.log(p / (1 - p)).to(dev)
        # build extension: spherical-harmonic colour (N,K,3); None = use `colors` like the reference
        self.sh: Optional[torch.Tensor] = None
        self.sh_degree = 0
        self._active_sh_degree: Optional[int] = None      # None: the stored degree (``active_sh_degree``)
        # build extension (spatially_ordered): int32 (N,), the ORIGINAL index of the Gaussian in every row; None = the rows
        # are in the caller's own order
        self.original_index: Optional[torch.Tensor] = None
        self.row_of_index: Optional[torch.Tensor] = None      # its inverse: row_of_index[original_index[i]] == i
        # ... and float32 (ceil(N / 256), 8): per block of 256 rows (min xyz, largest |scale|, max xyz, 0) -- GsxParams.block_bounds
        self.block_bounds: Optional[torch.Tensor] = None

    def __len__(self) -> int:
        return int(self.points.shape[0])

    @property
    def active_sh_degree(self) -> int:
        """The SH bands a frame evaluates and differentiates: 0..``sh_degree``, the stored degree unless set.  ``sh``, its
        gradient and its Adam moments keep the stored layout (N, (sh_degree + 1)^2, 3); the coefficients of the inactive
        bands are not read and receive an exact zero gradient."""
        active = getattr(self, "_active_sh_degree", None)
        return int(self.sh_degree) if active is None else min(int(active), int(self.sh_degree))

    @active_sh_degree.setter
    def active_sh_degree(self, degree: int) -> None:
        if isinstance(degree, bool) or int(degree) != degree:
            raise ValueError("active_sh_degree = %r is not an integer" % (degree,))
        if not 0 <= int(degree) <= int(self.sh_degree):
            raise ValueError("active_sh_degree = %r is outside 0..%d (sh_degree, the stored degree)"
                             % (degree, int(self.sh_degree)))
        self._active_sh_degree = int(degree)

    def oneup_sh_degree(self) -> int:
        """Raises ``active_sh_degree`` by one, up to the stored degree, and returns it (the published schedule calls this
        every 1000 steps)."""
        self.active_sh_degree = min(self.active_sh_degree + 1, int(self.sh_degree))
        return self.active_sh_degree

    def init_sh(self, degree: int) -> None:
        """Turns an RGB container (a point cloud) into an SH one stored at ``degree``: ``sh[:, 0] = (colors - 0.5) / C0``,
        so that degree 0 reproduces ``colors``, the higher bands zero, ``active_sh_degree`` 0 -- the published initialisation.
        ``sh`` requires grad when ``colors`` did."""
        if isinstance(degree, bool) or int(degree) != degree or not 0 <= int(degree) <= 3:
            raise ValueError("init_sh: degree = %r is outside 0..3" % (degree,))
        if self.sh is not None:
            raise ValueError("init_sh: the container already holds SH coefficients (sh_degree %d)" % int(self.sh_degree))
        degree = int(degree)
        n = len(self)
        colors = self.colors.detach().reshape(n, 3)
        sh = torch.zeros((n, (degree + 1) ** 2, 3), dtype=torch.float32, device=colors.device)
        sh[:, 0, :] = (colors - 0.5) / SH_C0
        self.sh = sh.requires_grad_(bool(self.colors.requires_grad))
        self.sh_degree = degree
        self._active_sh_degree = 0

    def to(self, device) -> "Gaussians":
        dev = torch.device(device)
        for name in ("points", "colors", "scales", "quaternions", "opacity"):
            setattr(self, name, getattr(self, name).to(dev).contiguous())
        if self.sh is not None:
            self.sh = self.sh.to(dev).contiguous()
        if self.original_index is not None:
            self.original_index = self.original_index.to(dev).contiguous()
            self.row_of_index = self.row_of_index.to(dev).contiguous()
        if self.block_bounds is not None:
            self.block_bounds = self.block_bounds.to(dev).contiguous()
        self.device = dev
        return self

    def refresh_block_bounds(self, rows: int = 256) -> None:
        """(Re)computes ``block_bounds`` from the CURRENT points and scales of a spatially ordered container: per block of
        ``rows`` = GSX_BOUNDS_ROWS consecutive rows the box of the means and the largest |scale|.  Call it again after
        changing ``points`` or ``scales`` in place -- the library trusts the bounds (include/gsx.h: block_bounds)."""
        n = len(self)
        nb = -(-n // rows)
        p = self.points.reshape(n, 3)
        s = self.scales.reshape(n, 3).abs().amax(dim=1) if n else torch.zeros(0, device=p.device)
        pad = nb * rows - n
        big = torch.finfo(torch.float32).max
        lo_src = torch.cat([p, torch.full((pad, 3), big, device=p.device)]) if pad else p
        hi_src = torch.cat([p, torch.full((pad, 3), -big, device=p.device)]) if pad else p
        s_src = torch.cat([s, torch.zeros(pad, device=p.device)]) if pad else s
        out = torch.zeros((nb, 8), dtype=torch.float32, device=p.device)
        if nb:
            out[:, 0:3] = lo_src.reshape(nb, rows, 3).amin(dim=1)
            out[:, 4:7] = hi_src.reshape(nb, rows, 3).amax(dim=1)
            out[:, 3] = s_src.reshape(nb, rows).amax(dim=1)
        old = self.block_bounds
        if old is not None and old.shape == out.shape and old.device == out.device and old.is_contiguous():
            old.copy_(out)          # in place: a captured frame (hipGraph) has this tensor's address baked in
        else:
            self.block_bounds = out.contiguous()
        self._bounds_of = self._bounds_stamp()

    def _bounds_stamp(self):
        """What ``block_bounds`` was computed from: the identity and in-place version of ``points`` and ``scales`` (torch
        counts in-place modifications of a tensor: ``_version``)."""
        return (self.points.data_ptr(), self.points._version, tuple(self.points.shape),
                self.scales.data_ptr(), self.scales._version, tuple(self.scales.shape))

    def current_block_bounds(self) -> Optional[torch.Tensor]:
        """``block_bounds`` for the arrays AS THEY ARE NOW: recomputed first when ``points`` or ``scales`` were replaced or
        modified in place since (an optimiser step, an edit) -- stale boxes would make a strip's projection drop Gaussians
        that have moved into its window.  None for a container whose rows are in the caller's own order."""
        if self.original_index is None:
            return None
        if self.block_bounds is None or getattr(self, "_bounds_of", None) != self._bounds_stamp():
            self.refresh_block_bounds()
        return self.block_bounds

    def spatially_ordered(self, bits: int = 10) -> "Gaussians":
        """A COPY of this container with the rows of every parameter array reordered along a 3D Morton (Z-order) curve of
        the means (``bits`` per axis over the cloud's bounding box; ties by original index), carrying ``original_index``.
        Opt-in, one time, view independent.  What it buys: Gaussians that are close in space -- hence on screen -- are
        close in memory, so a call that renders a PART of the frame (a multi-GPU rank's strip, a tile window) finds the
        survivors of its window test in runs and reads whole cache lines of their scales / quaternions / opacities /
        colours instead of a scattered eighth of every line.  What it does not change: the
        frame.  The library files every depth key under the Gaussian's ORIGINAL index (GsxParams.original_index) and
        sorts them in that order, so equal depths composite in original-index order, ``GaussianScene.last_order`` and
        ``preprocess`` report original indices, and every pixel is the unordered scene's, bit for bit (tested); records
        and rectangles stay in row order (``row_of_index``, the inverse permutation, takes the sort from one to the other).
        Per block of 256 rows ``block_bounds`` holds the box of the means: a strip's projection drops far blocks unread.  The
        reference's arrays stay the default; nothing else of the reference's surface sees the permutation."""
        if self.original_index is not None:
            return self
        n = len(self)
        p = self.points.reshape(n, 3)
        g = Gaussians.__new__(Gaussians)
        g.device, g.model_path, g.sh_degree = self.device, self.model_path, self.sh_degree
        g._active_sh_degree = getattr(self, "_active_sh_degree", None)
        if n == 0:
            perm = torch.zeros(0, dtype=torch.int64, device=p.device)
        else:
            from .knn import morton_permutation

            perm = morton_permutation(p, bits)
        for name in ("points", "colors", "scales", "quaternions", "opacity"):
            setattr(g, name, getattr(self, name)[perm].contiguous())
        g.sh = None if self.sh is None else self.sh[perm].contiguous()
        g.original_index = perm.to(torch.int32).contiguous()
        g.row_of_index = torch.empty_like(g.original_index)
        g.row_of_index[perm] = torch.arange(n, dtype=torch.int32, device=perm.device)
        g.block_bounds = None
        g.refresh_block_bounds()
        return g

    def initialize_scale(self, rule: str = "reference") -> None:
        """The reference's ``initialize_scale`` (splat/gaussians.py:35-52), which it leaves switched off because its
        n x n x 3 difference tensor does not fit: the scale of every Gaussian from the distances to its three nearest other
        points, exact, in one library call (gsx_knn3; ``knn.nearest3``).
        ``rule="reference"`` does what the reference does, quirk included: ``scales *= max(mean(d0, d1, d2), 1e-5)`` in
        place, so the constructor's 0.001 gives 0.001 x the mean distance, and fewer than four points give inf.
        ``rule="published"`` assigns sqrt(max(mean(d0^2, d1^2, d2^2), 1e-7)), the initial scale of the published 3D Gaussian
        Splatting trainer, to all three axes.  The rows are visited along a 21-bit Morton curve (10 bits leave the clusters
        of a trained scene unordered inside one cell); a spatially ordered container is visited as it is.  The in-place
        write is what ``current_block_bounds()`` watches."""
        from .knn import morton_permutation, nearest3

        n = len(self)
        p = self.points.detach().reshape(n, 3)
        order = None
        if self.original_index is None and n > 0 and p.device.type == "cuda":
            order = morton_permutation(p, 21).to(torch.int32).contiguous()
        _, scale = nearest3(p, order=order, rule=rule)
        with torch.no_grad():
            if rule == "reference":
                self.scales *= scale
            else:
                self.scales.copy_(scale.expand(n, 3))

    def transform(self, R, s: float = 1.0, t=None) -> None:
        """Moves the container into the world ``x' = s R x + t`` (``R`` a proper rotation, ``s > 0``; validated by
        ``transform.similarity``), IN PLACE, in one library call (gsx_transform_gaussians, include/gsx.h):
        ``points' = s R p + t``, ``scales' = s scales``, ``quaternions' = q_R (x) q`` (not renormalised) and, for an SH
        container, every STORED band of ``sh`` rotated by the matrices of ``transform.sh_rotation_matrices`` -- whatever
        ``active_sh_degree`` is -- so that the colour seen along ``R d`` is the colour that was seen along ``d``.
        ``opacity`` and ``colors`` do not change.  The library writes through raw pointers; the tensors' versions are
        bumped, so a spatially ordered container's ``current_block_bounds()`` recomputes.  ``.grad``s are left as they are,
        and an optimiser's moments are NOT rotated (``exp_avg_sq`` is not covariant): transform before a fit or after one.
        Cameras do not move: ``GaussianScene.transform`` moves them along."""
        import ctypes

        from . import _ffi
        from .transform import sh_rotation_matrices, similarity

        sim = similarity(R, s, t)
        n = len(self)
        degree = int(self.sh_degree) if self.sh is not None else 0
        arrays = [("points", self.points, 3), ("scales", self.scales, 3), ("quaternions", self.quaternions, 4)]
        if self.sh is not None:
            if not 0 <= degree <= 3:
                raise ValueError("sh_degree = %r is outside 0..3" % (self.sh_degree,))
            arrays.append(("sh", self.sh, 3 * (degree + 1) ** 2))
        dev = self.points.device
        for name, a, width in arrays:
            if a.device.type != "cuda":
                raise ValueError("%s is on %s: transform runs only as a HIP kernel on an AMD GPU (torch device 'cuda'); "
                                 "there is no CPU fallback" % (name, a.device))
            if a.device != dev:
                raise ValueError("%s is on %s, points on %s" % (name, a.device, dev))
            if a.dtype != torch.float32 or not a.is_contiguous() or a.shape[0] != n or a.numel() != n * width:
                raise ValueError("%s must be a contiguous float32 tensor of %d rows of %d" % (name, n, width))
            if torch.is_grad_enabled() and not a.is_leaf:
                raise ValueError("%s is not a leaf and gradients are enabled: an in-place transform would invalidate the "
                                 "graph that made it; detach it or call transform under torch.no_grad()" % name)
        T = _ffi.GsxTransform()
        T.R[:] = [float(v) for v in sim.R.reshape(-1)]
        T.s = sim.s
        T.t[:] = [float(v) for v in sim.t]
        T.q_R[:] = [float(v) for v in sim.q]
        for field, M in zip(("M1", "M2", "M3"), sh_rotation_matrices(sim.R)):
            getattr(T, field)[:] = [float(v) for v in M.reshape(-1)]
        if n == 0:              # (an empty tensor has no address to hand over)
            return
        with torch.cuda.device(dev):
            rc = _ffi.load().gsx_transform_gaussians(
                self.points.data_ptr(), self.scales.data_ptr(), self.quaternions.data_ptr(),
                self.sh.data_ptr() if self.sh is not None else None, degree, n, ctypes.byref(T),
                ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        _ffi.check(rc)
        # the library wrote through raw pointers: tell torch (current_block_bounds reads _version)
        for _, a, _ in arrays:
            torch.autograd.graph.increment_version(a)

    def get_3d_covariance_matrix(self) -> torch.Tensor:
        """(N,3,3) Sigma = (R S)(R S)^T, computed on the GPU (gsx_covariance_3d); same result as the
        reference's method (splat/gaussians.py:54-69).  The render path does not call this (the
        projection kernel computes Sigma inline); it exists for users of the reference's API."""
        import ctypes

        from . import _ffi

        lib = _ffi.load()
        dev = self.points.device
        if dev.type != "cuda":
            raise RuntimeError("get_3d_covariance_matrix runs as a HIP kernel: the tensors are on %s "
                               "(no CPU fallback)" % dev)
        n = len(self)
        s = self.scales.reshape(n, 3).contiguous()
        q = self.quaternions.reshape(n, 4).contiguous()
        out = torch.empty((n, 3, 3), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.gsx_covariance_3d(ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(q.data_ptr()), n,
                                       ctypes.c_void_p(out.data_ptr()),
                                       ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        _ffi.check(rc)
        return out

    @classmethod
    def from_arrays(cls, points, colors_0_255, scales, quaternions, opacity_logit, device=None) -> "Gaussians":
        """Builds a container and overwrites the constructor's defaults with explicit values."""
        g = cls(torch.as_tensor(points), torch.as_tensor(colors_0_255), device=device)
        f32 = torch.float32
        g.scales = torch.as_tensor(scales).to(g.device, f32).reshape(-1, 3).contiguous()
        g.quaternions = torch.as_tensor(quaternions).to(g.device, f32).reshape(-1, 4).contiguous()
        g.opacity = torch.as_tensor(opacity_logit).to(g.device, f32).reshape(-1, 1).contiguous()
        return g

    @classmethod
    def from_colmap_points(cls, points3D, min_track_length: int = 2, device=None) -> "Gaussians":
        """A container from COLMAP's sparse points (``colmap.read_points3D_file``: id -> ``Point3D``): the points seen by at
        least ``min_track_length`` images (the filter of the reference's notebook), one row each, in ASCENDING POINT ID --
        whatever order the file or the dict had, so the container is a pure function of the model -- and then the
        constructor's own arithmetic (``colors = rgb / 256``, the default scales, quaternions and opacity).  Scales from the
        neighbours (``initialize_scale``) and SH (``init_sh``) stay the caller's lines."""
        import numpy as np

        if isinstance(min_track_length, bool) or int(min_track_length) != min_track_length or int(min_track_length) < 0:
            raise ValueError("min_track_length = %r is not a non-negative integer" % (min_track_length,))
        kept = [points3D[k] for k in sorted(points3D) if len(points3D[k].image_ids) >= int(min_track_length)]
        xyz = np.array([p.xyz for p in kept], dtype=np.float64).reshape(-1, 3)
        rgb = np.array([p.rgb for p in kept], dtype=np.float64).reshape(-1, 3)
        return cls(torch.from_numpy(xyz), torch.from_numpy(rgb), device=device)

    @classmethod
    def from_ply(cls, path: str, device=None) -> "Gaussians":
        """Loads a ``.ply``: a trained 3D Gaussian Splatting checkpoint (log-scales -> linear, SH
        coefficients, logit opacity) or a plain xyz+rgb point cloud (then the reference's
        constructor defaults apply).  Build extension -- see ``ply.py``."""
        from .ply import load_gaussians

        d = load_gaussians(path)
        if "sh" not in d:
            return cls(torch.from_numpy(d["points"]), torch.from_numpy(d["colors_0_255"]), device=device)
        n = d["points"].shape[0]
        g = cls.from_arrays(d["points"], torch.zeros((n, 3)), d["scales"], d["quaternions"], d["opacity"],
                            device=device)
        g.sh = torch.from_numpy(d["sh"]).to(g.device).contiguous()
        g.sh_degree = int(d["sh_degree"])
        return g
