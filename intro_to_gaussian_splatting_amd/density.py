"""Adaptive density control of a splat fit on the GPU: ``DensityControl`` (gsx_density_accumulate / gsx_density_plan /
gsx_density_apply and, with ``statistic="screen"``, gsx_density_accumulate_screen / gsx_density_plan_screen, include/gsx.h).

After every ``backward()`` ``accumulate()`` adds the norm of each Gaussian's ``points.grad`` -- or, with
``statistic="screen"``, of its screen-space mean gradient, the published statistic -- to a running statistic; every few
hundred steps ``densify_and_prune()`` gives every Gaussian one action -- prune, clone, split or keep -- and rewrites every
array of the container and both moment arrays of the optimiser in ONE library call: a survivor keeps the bits of its
parameters and of its Adam moments, a new Gaussian starts with zero moments, and rows stay in source order with the children
beside their parent.  ``prune_contribution()`` prunes by what a Gaussian shows instead -- the largest blend weight it reaches
in any pixel of the views ``GaussianScene.contribution()`` swept (gsx_density_plan_contribution) -- through the same rewrite.
There is no torch composition behind it and no CPU path.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional

import torch

from . import _ffi
from ._device import _stream_handle
from .optim import GROUP_NAMES

_ROLES = {"points": _ffi.GSX_DENSITY_POINTS, "scales": _ffi.GSX_DENSITY_SCALES, "quaternions": _ffi.GSX_DENSITY_QUATS}
COUNT_NAMES = ("n_out", "n_pruned", "n_cloned", "n_split")


class DensityControl:
    """Prune / clone / split over ``gaussians`` (and ``optimizer``'s moments, and ``scene``'s per-view caches).

    The rules (include/gsx.h, gsx_density_plan), in this order: PRUNE where the opacity LOGIT is below ``prune_logit`` or the
    largest scale above ``prune_scale``; otherwise, where the mean accumulated gradient norm is at least ``grad_threshold``,
    SPLIT in two (scales divided by ``split_shrink``, positions drawn from the parent's own Gaussian) when the largest scale
    is above ``dense_scale`` and CLONE when it is not; KEEP everything else.  ``max_gaussians``: when a round would leave
    more rows than this, it prunes only.

    ``statistic``: what ``accumulate()`` adds up.
    ``"points"`` (default): the norm of dL/dpoints, in world units, over the backward passes that gave the Gaussian a non-zero
    gradient.  That is not the published statistic, so the published 2e-4 is only a default to start from: set
    ``grad_threshold`` and ``dense_scale`` for the scene (the attributes may be changed between rounds).
    ``"screen"`` (needs ``scene``): the published one.  Render with ``geometry_gradients=True, screen_statistics=True``;
    ``accumulate()`` then consumes ``scene.screen_statistics`` -- the norm of dL/d(NDC mean), so ``grad_threshold`` is in
    loss per NDC unit, the published convention, and the published 2e-4 means what it means there -- and counts a Gaussian as
    seen whenever the frame listed it on a tile, zero gradient or not (gsx_density_accumulate_screen).  It also keeps the
    largest screen radius seen, ``radius_max``, and a round PRUNES, besides the rules above, where that is above
    ``prune_radius`` pixels (``math.inf``: never; gsx_density_plan_screen).
    ``"screen_abs"`` (needs ``scene``): AbsGS's statistic, gsplat's ``absgrad``.  dL/d(NDC mean) is a signed sum over the pixels
    a Gaussian touches; a large Gaussian over fine detail gets terms of both signs, they cancel, and the blur never splits.
    Render with ``geometry_gradients=True, screen_statistics="abs"``; ``accumulate()`` then adds the norm of the ABSOLUTE
    statistic (gsx_render_backward_screen_abs: per component the sum of the absolute values of the pixels' terms) through the
    same gsx_density_accumulate_screen, so seen-if-listed, ``radius_max`` and ``prune_radius`` work exactly as for
    ``"screen"``.  The unit is still loss per NDC unit, but the value is never below the signed one and on this project's
    fixtures is typically several times it: the published 2e-4 belongs to the SIGNED statistic, and this project has
    measured no value for the absolute one -- ``grad_threshold`` has no default that means anything here; set it for the
    scene."""

    STATISTICS = ("points", "screen", "screen_abs")
    _SCREEN = ("screen", "screen_abs")          # the statistics that read scene.screen_statistics and keep radius_max

    def __init__(self, gaussians, optimizer=None, scene=None, grad_threshold: float = 2e-4, dense_scale: float = 0.01,
                 prune_logit: float = -5.3, prune_scale: float = math.inf, split_shrink: float = 1.6,
                 max_gaussians: Optional[int] = None, statistic: str = "points", prune_radius: float = math.inf) -> None:
        if statistic not in self.STATISTICS:
            raise ValueError("statistic = %r is neither 'points' nor 'screen' nor 'screen_abs'" % (statistic,))
        if statistic in self._SCREEN and scene is None:
            raise ValueError("statistic=%r needs scene: accumulate() reads scene.screen_statistics" % (statistic,))
        if math.isnan(float(prune_radius)):
            raise ValueError("prune_radius is NaN")
        if getattr(gaussians, "original_index", None) is not None:
            raise ValueError("the container is spatially ordered: its permutation and block boxes would be stale after a "
                             "round.  Densify the plain container and call spatially_ordered() again")
        if optimizer is not None and optimizer.gaussians is not gaussians:
            raise ValueError("optimizer belongs to another container than gaussians")
        if scene is not None and scene.gaussians is not gaussians:
            raise ValueError("scene renders another container than gaussians")
        if not (float(split_shrink) > 0.0 and math.isfinite(float(split_shrink))):
            raise ValueError("split_shrink = %r is not a positive finite number" % (split_shrink,))
        if max_gaussians is not None and int(max_gaussians) < 0:
            raise ValueError("max_gaussians = %r is negative" % (max_gaussians,))
        self.gaussians, self.optimizer, self.scene = gaussians, optimizer, scene
        self.grad_threshold, self.dense_scale = float(grad_threshold), float(dense_scale)
        self.prune_logit, self.prune_scale = float(prune_logit), float(prune_scale)
        self.split_shrink = float(split_shrink)
        self.max_gaussians = None if max_gaussians is None else int(max_gaussians)
        self.statistic, self.prune_radius = statistic, float(prune_radius)
        self._check_arrays()
        dev = gaussians.points.device
        n = len(gaussians)
        self.grad_sum = torch.zeros(n, dtype=torch.float32, device=dev)
        self.seen = torch.zeros(n, dtype=torch.int32, device=dev)        # (the library's uint32)
        self.radius_max = torch.zeros(n, dtype=torch.float32, device=dev) if statistic in self._SCREEN else None
        self._workspace: Optional[torch.Tensor] = None
        self._groups = (_ffi.GsxDensityGroup * _ffi.GSX_DENSITY_MAX_GROUPS)()

    # ------------------------------------------------------------------ helpers
    def _names(self):
        return tuple(name for name in GROUP_NAMES if getattr(self.gaussians, name, None) is not None)

    def _check_arrays(self) -> None:
        g = self.gaussians
        if getattr(g, "original_index", None) is not None:
            raise ValueError("the container is spatially ordered: densify the plain container and call spatially_ordered() again")
        n = len(g)
        dev = g.points.device
        for name in self._names():
            t = getattr(g, name)
            if t.device.type != "cuda":
                raise ValueError("%s is on %s: density control runs only as HIP kernels on an AMD GPU (torch device 'cuda'); "
                                 "there is no CPU fallback" % (name, t.device))
            if t.device != dev:
                raise ValueError("%s is on %s, points on %s" % (name, t.device, dev))
            if t.dtype != torch.float32 or not t.is_contiguous() or t.shape[0] != n:
                raise ValueError("%s must be a contiguous float32 tensor of %d rows" % (name, n))

    def _rules(self, grad_threshold: float) -> _ffi.GsxDensityRules:
        return _ffi.GsxDensityRules(grad_threshold, self.dense_scale, self.prune_logit, self.prune_scale, self.split_shrink, 0)

    def _plan(self, n: int, grad_threshold: float, dev) -> Dict[str, int]:
        g = self.gaussians
        need = int(_ffi.load().gsx_density_workspace_bytes(n))
        if need == 0:
            raise ValueError("%d Gaussians are more than density control takes (2^30)" % n)
        if self._workspace is None or self._workspace.numel() < need or self._workspace.device != dev:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        counts = (ctypes.c_int64 * 4)()
        rules = self._rules(grad_threshold)
        with torch.cuda.device(dev):
            if self.statistic in self._SCREEN:
                rc = _ffi.load().gsx_density_plan_screen(self.grad_sum.data_ptr(), self.seen.data_ptr(), g.scales.data_ptr(),
                                                         g.opacity.data_ptr(), self.radius_max.data_ptr(), self.prune_radius, n,
                                                         ctypes.byref(rules), self._workspace.data_ptr(),
                                                         self._workspace.numel(), counts, _stream_handle(dev))
            else:
                rc = _ffi.load().gsx_density_plan(self.grad_sum.data_ptr(), self.seen.data_ptr(), g.scales.data_ptr(),
                                                  g.opacity.data_ptr(), n, ctypes.byref(rules), self._workspace.data_ptr(),
                                                  self._workspace.numel(), counts, _stream_handle(dev))
        _ffi.check(rc)
        return dict(zip(COUNT_NAMES, (int(c) for c in counts)))

    # ------------------------------------------------------------------ the surface
    def accumulate(self) -> None:
        """After ``backward()``: adds |points.grad| of every Gaussian with a non-zero gradient row to the statistic and counts
        it as seen (gsx_density_accumulate).  Allocates nothing after the first call.  ``statistic="screen"`` and
        ``"screen_abs"``: consume ``scene.screen_statistics`` instead (``_accumulate_screen``)."""
        if self.statistic in self._SCREEN:
            return self._accumulate_screen()
        g = self.gaussians
        grad = g.points.grad
        if grad is None:
            raise ValueError("points has no .grad: call backward() (with geometry_gradients=True) before accumulate()")
        n = len(g)
        if grad.dtype != torch.float32 or not grad.is_contiguous() or tuple(grad.shape) != tuple(g.points.shape):
            raise ValueError("points.grad must be contiguous float32 and of the shape of points")
        if grad.device.type != "cuda" or grad.device != self.grad_sum.device:
            raise ValueError("points.grad is on %s, the statistic on %s; there is no CPU fallback" % (grad.device, self.grad_sum.device))
        if self.grad_sum.shape[0] != n:
            raise ValueError("the container has %d rows, the statistic %d: rows changed outside densify_and_prune()"
                             % (n, self.grad_sum.shape[0]))
        dev = grad.device
        with torch.cuda.device(dev):
            rc = _ffi.load().gsx_density_accumulate(grad.data_ptr(), grad.numel() // n if n else 3, n, self.grad_sum.data_ptr(),
                                                    self.seen.data_ptr(), _stream_handle(dev))
        _ffi.check(rc)

    def _accumulate_screen(self) -> None:
        """After a ``backward()`` of a frame rendered with ``screen_statistics=True``: adds the norm of dL/d(NDC mean) of
        every Gaussian the frame listed to the statistic, counts it as seen and keeps its largest radius
        (gsx_density_accumulate_screen), then sets ``scene.screen_statistics`` to None: one backward is counted once.
        ``statistic="screen_abs"``: the same call on the absolute statistic, the fourth entry ``screen_statistics="abs"``
        leaves; ``"screen"`` reads the first three entries of either tuple."""
        stat = self.scene.screen_statistics
        if stat is None:
            raise ValueError("scene.screen_statistics is None: render with geometry_gradients=True, screen_statistics=%s and "
                             "call backward() before every accumulate()"
                             % ("'abs'" if self.statistic == "screen_abs" else "True"))
        if self.statistic == "screen_abs":
            if len(stat) < 4:
                raise ValueError("scene.screen_statistics holds no absolute statistic: statistic='screen_abs' needs frames "
                                 "rendered with screen_statistics='abs', not True")
            _, _, radius, grad = stat[:4]
        else:
            _, grad, radius = stat[:3]
        n = len(self.gaussians)
        if grad.shape[0] != n or radius.shape[0] != n or self.grad_sum.shape[0] != n:
            raise ValueError("the container has %d rows, scene.screen_statistics %d and the statistic %d: rows changed "
                             "outside densify_and_prune()" % (n, grad.shape[0], self.grad_sum.shape[0]))
        dev = self.grad_sum.device
        for name, t, shape in (("grad_means2d", grad, (n, 2)), ("screen_radius", radius, (n,))):
            if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape or t.device != dev:
                raise ValueError("scene.screen_statistics: %s must be contiguous float32 of shape %s on %s; there is no CPU "
                                 "fallback" % (name, shape, dev))
        with torch.cuda.device(dev):
            rc = _ffi.load().gsx_density_accumulate_screen(grad.data_ptr(), radius.data_ptr(), n, self.grad_sum.data_ptr(),
                                                           self.seen.data_ptr(), self.radius_max.data_ptr(),
                                                           _stream_handle(dev))
        _ffi.check(rc)
        self.scene.screen_statistics = None

    def densify_and_prune(self, generator: Optional[torch.Generator] = None) -> Dict[str, int]:
        """One round: plan, rewrite every array and moment, install, reset the statistic and the scene's caches.  Returns
        ``n_out``, ``n_pruned``, ``n_cloned``, ``n_split``.  The split positions draw ``torch.randn((n, 2, 3))`` from
        ``generator`` (a generator of the container's device): the same seed gives the same container."""
        n, dev = self._check_round()
        counts = self._plan(n, self.grad_threshold, dev)
        if self.max_gaussians is not None and counts["n_out"] > self.max_gaussians:
            counts = self._plan(n, math.inf, dev)           # prune only
        noise = torch.randn((n, 2, 3), generator=generator, device=dev, dtype=torch.float32)
        self._apply(n, counts["n_out"], noise, dev)
        return counts

    def _check_round(self):
        """What a round checks before it plans: the arrays, the statistic's length, the optimiser's moments.  (n, device)."""
        self._check_arrays()
        g, opt = self.gaussians, self.optimizer
        n = len(g)
        dev = g.points.device
        if self.grad_sum.shape[0] != n:
            raise ValueError("the container has %d rows, the statistic %d: rows changed outside densify_and_prune()"
                             % (n, self.grad_sum.shape[0]))
        if opt is not None:
            if opt.gaussians is not g:
                raise ValueError("optimizer belongs to another container than gaussians")
            for name in opt.names:
                for key in ("exp_avg", "exp_avg_sq"):
                    m = getattr(opt, key)[name]
                    if tuple(m.shape) != tuple(getattr(g, name).shape) or m.device != dev or not m.is_contiguous():
                        raise ValueError("optimizer.%s[%r] is not of the shape and device of %s" % (key, name, name))
        return n, dev

    def _apply(self, n: int, n_out: int, noise: Optional[torch.Tensor], dev) -> None:
        """gsx_density_apply on the plan the workspace holds: every array of the container and both moment arrays rewritten
        and installed, the statistic reset to ``n_out`` rows of zeros, the scene's caches dropped."""
        g, opt = self.gaussians, self.optimizer

        names = self._names()
        # (noise None: a plan of KEEP and PRUNE alone -- no row is split, every array is a plain copy and needs no noise)
        roles = _ROLES if noise is not None else {}
        jobs = [(name, getattr(g, name), roles.get(name, _ffi.GSX_DENSITY_COPY)) for name in names]
        if opt is not None:
            jobs += [((key, name), getattr(opt, key)[name], _ffi.GSX_DENSITY_ZERO_NEW)
                     for name in opt.names for key in ("exp_avg", "exp_avg_sq")]
        if len(jobs) > _ffi.GSX_DENSITY_MAX_GROUPS:
            raise ValueError("%d arrays are more than one call rewrites (%d)" % (len(jobs), _ffi.GSX_DENSITY_MAX_GROUPS))
        new = {}
        for i, (key, src, role) in enumerate(jobs):
            dst = torch.empty((n_out,) + tuple(src.shape[1:]), dtype=torch.float32, device=dev)
            new[key] = dst
            grp = self._groups[i]
            grp.src, grp.dst = src.data_ptr(), dst.data_ptr()
            grp.width = src.numel() // n if n else max(1, math.prod(src.shape[1:]))
            grp.role = role
        with torch.cuda.device(dev):
            rc = _ffi.load().gsx_density_apply(self._groups, len(jobs), n, n_out, None if noise is None else noise.data_ptr(), None,
                                               self._workspace.data_ptr(), self._workspace.numel(), _stream_handle(dev))
        _ffi.check(rc)

        for name in names:
            old = getattr(g, name)
            setattr(g, name, new[name].requires_grad_(old.requires_grad))        # a leaf again, .grad None
        if opt is not None:
            opt.exp_avg = {name: new[("exp_avg", name)] for name in opt.names}
            opt.exp_avg_sq = {name: new[("exp_avg_sq", name)] for name in opt.names}
        self.grad_sum = torch.zeros(n_out, dtype=torch.float32, device=dev)
        self.seen = torch.zeros(n_out, dtype=torch.int32, device=dev)
        if self.radius_max is not None:
            self.radius_max = torch.zeros(n_out, dtype=torch.float32, device=dev)
        if self.scene is not None:
            self.scene.gaussians_changed()

    def prune_contribution(self, contribution, threshold: float = 0.01, require_seen: bool = True) -> Dict[str, int]:
        """Prunes by what the Gaussians show (gsx_density_plan_contribution, then the gsx_density_apply of a round): a row
        goes where ``contribution.weight_max`` -- the largest blend weight it reaches in any pixel of the views
        ``scene.contribution(...)`` swept -- is below ``threshold`` (float32; exactly equal is kept, a NaN weight is kept)
        and, with ``require_seen``, where no view listed it (``contribution.views == 0``), whatever its weight.  The
        published threshold is 0.01 (RadSplat); the rules of ``densify_and_prune`` ask nothing of the kind: an opaque
        Gaussian buried behind a surface passes all of them.  Survivors keep the bits of their parameters and Adam moments,
        in order; the accumulated densification statistic is dropped and ``scene.gaussians_changed()`` called exactly as by
        ``densify_and_prune``.  Returns its counts (``n_cloned`` = ``n_split`` = 0).  Refused: a ``contribution`` that is
        not of this container's length or device, a NaN or negative ``threshold``."""
        n, dev = self._check_round()
        threshold = float(threshold)
        if not threshold >= 0.0:
            raise ValueError("threshold = %r is NaN or negative" % (threshold,))
        wmax, views = getattr(contribution, "weight_max", None), getattr(contribution, "views", None)
        if not isinstance(wmax, torch.Tensor) or not isinstance(views, torch.Tensor):
            raise TypeError("contribution must be a Contribution (scene.contribution(...)), got %s" % type(contribution).__name__)
        for name, t, dtype in (("weight_max", wmax, torch.float32), ("views", views, torch.int32)):
            if t.dim() != 1 or t.shape[0] != n:
                raise ValueError("contribution.%s has shape %s, the container %d rows: it was measured on other rows -- sweep the "
                                 "views again (scene.contribution) after the rows changed" % (name, tuple(t.shape), n))
            if t.device.type != "cuda" or t.device != dev:
                raise ValueError("contribution.%s is on %s, the container on %s; there is no CPU fallback" % (name, t.device, dev))
            if t.dtype != dtype or not t.is_contiguous():
                raise ValueError("contribution.%s must be a contiguous %s tensor" % (name, dtype))
        need = int(_ffi.load().gsx_density_workspace_bytes(n))
        if need == 0:
            raise ValueError("%d Gaussians are more than density control takes (2^30)" % n)
        if self._workspace is None or self._workspace.numel() < need or self._workspace.device != dev:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        counts = (ctypes.c_int64 * 4)()
        with torch.cuda.device(dev):
            rc = _ffi.load().gsx_density_plan_contribution(wmax.data_ptr(), views.data_ptr() if require_seen else None, threshold,
                                                           n, self._workspace.data_ptr(), self._workspace.numel(), counts,
                                                           _stream_handle(dev))
        _ffi.check(rc)
        out = dict(zip(COUNT_NAMES, (int(c) for c in counts)))
        self._apply(n, out["n_out"], None, dev)
        return out

    def reset_opacity(self, cap_logit: float) -> None:
        """The published trainer's opacity reset, on the logit: ``opacity.clamp_(max=cap_logit)`` in place and zeros in the
        optimiser's two opacity moment arrays.  Plain torch -- it runs once in thousands of steps."""
        g = self.gaussians
        if g.opacity.device.type != "cuda":
            raise ValueError("opacity is on %s; there is no CPU fallback" % g.opacity.device)
        with torch.no_grad():
            g.opacity.clamp_(max=float(cap_logit))
            opt = self.optimizer
            if opt is not None and "opacity" in opt.exp_avg:
                opt.exp_avg["opacity"].zero_()
                opt.exp_avg_sq["opacity"].zero_()
