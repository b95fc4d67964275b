"""Fixed-budget densification of a splat fit on the GPU: ``MCMCControl`` (gsx_mcmc_regularize / gsx_mcmc_perturb /
gsx_mcmc_plan / gsx_mcmc_apply, include/gsx.h) -- the strategy of 3DGS-MCMC (Kheradmand et al. 2024).

The container never holds more than ``cap_max`` rows.  After every ``backward()`` ``regularize()`` adds the gradients of an
opacity and a scale regulariser; after every optimiser step ``perturb()`` adds an opacity-gated noise term to the positions;
every few hundred steps ``relocate()`` moves the dead Gaussians onto live ones drawn in proportion to opacity, grows the
container by ``growth`` towards ``cap_max`` the same way, and corrects opacity and scale so that N coincident copies
composite like the one they came from.  It needs no densification statistic: no ``screen_statistics`` export, no
``accumulate()``.  Every part is ONE library call; there is no torch composition behind it and no CPU path.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional

import torch

from . import _ffi
from ._device import _stream_handle
from .optim import GROUP_NAMES

_ROLES = {"opacity": _ffi.GSX_MCMC_OPACITY, "scales": _ffi.GSX_MCMC_SCALES}
COUNT_NAMES = ("n_out", "n_dead", "n_live", "n_new")


class MCMCControl:
    """Relocation, growth and noise over ``gaussians`` (and ``optimizer``'s moments, and ``scene``'s per-view caches).

    ``cap_max`` (required, at least ``len(gaussians)``): the budget.  ``min_opacity``: a Gaussian whose opacity
    ``sigmoid(logit)`` is at most this is dead.  ``growth``: a round leaves ``min(cap_max, max(n, floor(growth * n)))`` rows.
    ``noise_lr``: ``perturb()`` uses ``rate = noise_lr * (the position rate of the step just taken)``.  ``lambda_opacity``,
    ``lambda_scale``: the regularisers ``lambda_opacity * mean(sigmoid(opacity)) + lambda_scale * mean(|scales|)``, of which
    ``regularize()`` adds the GRADIENTS; their value is not computed, so the loss a ``Trainer`` reports stays the photometric
    one.  ``gate_k``, ``gate_x0``: the noise gate ``1 / (1 + exp(-gate_k * ((1 - sigmoid(opacity)) - gate_x0)))``.  The
    defaults are the published values; the attributes may be changed between steps.

    One round draws relocation and growth TOGETHER from the pre-round opacities.  The published code draws twice, the second
    time (the growth) from opacities the first draw has already reduced; here every drawn row -- a dead row's new place and
    a new row alike -- takes its own uniform against one table of weights.

    ``GaussianAdam(skip_zero_rows=True)`` skips nothing once ``regularize()`` has run: every row then has a gradient."""

    def __init__(self, gaussians, optimizer=None, scene=None, cap_max: Optional[int] = None, min_opacity: float = 0.005,
                 growth: float = 1.05, noise_lr: float = 5e5, lambda_opacity: float = 0.01, lambda_scale: float = 0.01,
                 gate_k: float = 100.0, gate_x0: float = 0.995) -> None:
        if getattr(gaussians, "original_index", None) is not None:
            raise ValueError("the container is spatially ordered: its permutation and block boxes would be stale after a "
                             "round.  Relocate in the plain container and call spatially_ordered() again")
        if optimizer is not None and optimizer.gaussians is not gaussians:
            raise ValueError("optimizer belongs to another container than gaussians")
        if scene is not None and scene.gaussians is not gaussians:
            raise ValueError("scene renders another container than gaussians")
        if cap_max is None:
            raise ValueError("cap_max is required: the budget of a fixed-budget strategy has no default")
        if isinstance(cap_max, bool) or int(cap_max) != cap_max:
            raise ValueError("cap_max = %r is not an integer" % (cap_max,))
        if int(cap_max) < len(gaussians):
            raise ValueError("cap_max = %d is below the %d Gaussians the container holds" % (int(cap_max), len(gaussians)))
        if not 0.0 < float(min_opacity) < 1.0:
            raise ValueError("min_opacity = %r is outside (0, 1)" % (min_opacity,))
        if not (float(growth) >= 1.0 and math.isfinite(float(growth))):
            raise ValueError("growth = %r is not a finite number >= 1" % (growth,))
        for name, value in (("noise_lr", noise_lr), ("lambda_opacity", lambda_opacity), ("lambda_scale", lambda_scale),
                            ("gate_k", gate_k)):
            if not (float(value) >= 0.0 and math.isfinite(float(value))):
                raise ValueError("%s = %r is negative or not finite" % (name, value))
        if not math.isfinite(float(gate_x0)):
            raise ValueError("gate_x0 = %r is not finite" % (gate_x0,))
        self.gaussians, self.optimizer, self.scene = gaussians, optimizer, scene
        self.cap_max, self.min_opacity, self.growth = int(cap_max), float(min_opacity), float(growth)
        self.noise_lr, self.lambda_opacity, self.lambda_scale = float(noise_lr), float(lambda_opacity), float(lambda_scale)
        self.gate_k, self.gate_x0 = float(gate_k), float(gate_x0)
        self._check_arrays()
        self._workspace: Optional[torch.Tensor] = None
        self._groups = (_ffi.GsxDensityGroup * _ffi.GSX_DENSITY_MAX_GROUPS)()

    # ------------------------------------------------------------------ helpers
    def _names(self):
        return tuple(name for name in GROUP_NAMES if getattr(self.gaussians, name, None) is not None)

    def _check_arrays(self) -> None:
        g = self.gaussians
        if getattr(g, "original_index", None) is not None:
            raise ValueError("the container is spatially ordered: relocate in the plain container and call spatially_ordered() again")
        n = len(g)
        dev = g.points.device
        for name in self._names():
            t = getattr(g, name)
            if t.device.type != "cuda":
                raise ValueError("%s is on %s: fixed-budget densification runs only as HIP kernels on an AMD GPU (torch device "
                                 "'cuda'); there is no CPU fallback" % (name, t.device))
            if t.device != dev:
                raise ValueError("%s is on %s, points on %s" % (name, t.device, dev))
            if t.dtype != torch.float32 or not t.is_contiguous() or t.shape[0] != n:
                raise ValueError("%s must be a contiguous float32 tensor of %d rows" % (name, n))

    @property
    def dead_logit(self) -> float:
        """logit(min_opacity): what gsx_mcmc_plan compares the opacity logits with."""
        return math.log(self.min_opacity / (1.0 - self.min_opacity))

    def n_out_for(self, n: int) -> int:
        """Rows a round over ``n`` rows leaves: ``min(cap_max, max(n, floor(growth * n)))``.  Host arithmetic."""
        return min(self.cap_max, max(int(n), int(math.floor(self.growth * int(n)))))

    # ------------------------------------------------------------------ the surface
    def regularize(self) -> None:
        """After ``backward()``, before ``opt.step()``: adds the regularisers' gradients to ``opacity.grad`` and
        ``scales.grad`` in place (gsx_mcmc_regularize, one launch).  A lambda of 0 leaves its array alone."""
        self._check_arrays()
        g = self.gaussians
        n = len(g)
        dev = g.points.device
        ptr = {}
        for name, lam in (("opacity", self.lambda_opacity), ("scales", self.lambda_scale)):
            if lam == 0.0:
                ptr[name] = None
                continue
            t = getattr(g, name)
            grad = t.grad
            if grad is None:
                raise ValueError("%s has no .grad: call backward() before regularize()" % name)
            if grad.dtype != torch.float32 or not grad.is_contiguous() or tuple(grad.shape) != tuple(t.shape) or grad.device != dev:
                raise ValueError("%s.grad must be contiguous float32, of the shape of %s and on %s" % (name, name, dev))
            ptr[name] = grad.data_ptr()
        with torch.cuda.device(dev):
            rc = _ffi.load().gsx_mcmc_regularize(g.opacity.data_ptr(), g.scales.data_ptr(), n, self.lambda_opacity,
                                                 self.lambda_scale, ptr["opacity"], ptr["scales"], _stream_handle(dev))
        _ffi.check(rc)

    def point_rate(self) -> float:
        """The position learning rate of the optimiser step just taken."""
        opt = self.optimizer
        if opt is None:
            raise ValueError("perturb() reads the position rate from the optimizer: MCMCControl was built without one")
        if "points" not in opt.lr:
            raise ValueError("the optimizer does not train points: there is no position rate to scale the noise with")
        if opt.step_count < 1:
            raise ValueError("the optimizer has taken no step: call perturb() after opt.step()")
        return opt._rate("points", opt.step_count)

    def perturb(self, generator: Optional[torch.Generator] = None) -> None:
        """After ``opt.step()``: ``points += noise_lr * lr_points(step) * gate * Sigma * eps`` in place (gsx_mcmc_perturb,
        one launch), ``eps = torch.randn((n, 3))`` from ``generator`` (a generator of the container's device).  A row whose
        step is not finite keeps its bits."""
        self._check_arrays()
        g = self.gaussians
        n = len(g)
        dev = g.points.device
        rate = self.noise_lr * self.point_rate()
        noise = torch.randn((n, 3), generator=generator, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            rc = _ffi.load().gsx_mcmc_perturb(g.points.data_ptr(), g.scales.data_ptr(), g.quaternions.data_ptr(),
                                              g.opacity.data_ptr(), noise.data_ptr(), n, rate, self.gate_k, self.gate_x0,
                                              _stream_handle(dev))
        _ffi.check(rc)
        # the library wrote through a raw pointer: tell torch (Gaussians.current_block_bounds reads _version)
        torch.autograd.graph.increment_version(g.points)

    def plan(self, n_out: int, generator: Optional[torch.Generator] = None):
        """gsx_mcmc_plan over the container's opacities: ``(counts, weights, source, count)`` with ``counts`` the dict
        ``relocate()`` returns and the three device arrays of the plan (int32; ``weights`` and ``count`` are the library's
        uint32).  Draws ``torch.rand(n_out, dtype=float64)`` from ``generator``."""
        g = self.gaussians
        n = len(g)
        dev = g.points.device
        need = int(_ffi.load().gsx_mcmc_workspace_bytes(n))
        if need == 0:
            raise ValueError("%d Gaussians are more than fixed-budget densification takes (2^30)" % n)
        if self._workspace is None or self._workspace.numel() < need or self._workspace.device != dev:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        uniforms = torch.rand(n_out, generator=generator, device=dev, dtype=torch.float64)
        weights = torch.empty(n, dtype=torch.int32, device=dev)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        source = torch.empty(n_out, dtype=torch.int32, device=dev)
        host = (ctypes.c_int64 * 3)()
        with torch.cuda.device(dev):
            rc = _ffi.load().gsx_mcmc_plan(g.opacity.data_ptr(), n, self.dead_logit, n_out, uniforms.data_ptr(),
                                           weights.data_ptr(), source.data_ptr(), count.data_ptr(), self._workspace.data_ptr(),
                                           self._workspace.numel(), host, _stream_handle(dev))
        _ffi.check(rc)
        counts = dict(zip(COUNT_NAMES, (int(n_out), int(host[0]), int(host[1]), int(host[2]))))
        return counts, weights, source, count

    def relocate(self, generator: Optional[torch.Generator] = None) -> Dict[str, int]:
        """One round: plan, rewrite every array and moment, install, reset the scene's caches.  Returns ``n_out``,
        ``n_dead``, ``n_live``, ``n_new``.  Raises ``ValueError`` when no Gaussian is alive (nothing is rewritten then).
        The same seed gives the same container."""
        self._check_arrays()
        g, opt = self.gaussians, self.optimizer
        n = len(g)
        dev = g.points.device
        if n > self.cap_max:
            raise ValueError("the container has %d rows, cap_max is %d: rows were added outside relocate()" % (n, self.cap_max))
        if opt is not None:
            if opt.gaussians is not g:
                raise ValueError("optimizer belongs to another container than gaussians")
            for name in opt.names:
                for key in ("exp_avg", "exp_avg_sq"):
                    m = getattr(opt, key)[name]
                    if tuple(m.shape) != tuple(getattr(g, name).shape) or m.device != dev or not m.is_contiguous():
                        raise ValueError("optimizer.%s[%r] is not of the shape and device of %s" % (key, name, name))
        n_out = self.n_out_for(n)
        counts, _, source, count = self.plan(n_out, generator)
        if counts["n_live"] == 0:
            raise ValueError("no Gaussian is alive: every opacity is at most min_opacity = %g (or not finite), there is "
                             "nothing to relocate onto" % self.min_opacity)

        names = self._names()
        jobs = [(name, getattr(g, name), _ROLES.get(name, _ffi.GSX_MCMC_COPY)) for name in names]
        if opt is not None:
            jobs += [((key, name), getattr(opt, key)[name], _ffi.GSX_MCMC_ZERO_MOVED)
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
            rc = _ffi.load().gsx_mcmc_apply(self._groups, len(jobs), n, n_out, source.data_ptr(), count.data_ptr(),
                                            self.min_opacity, _stream_handle(dev))
        _ffi.check(rc)

        for name in names:
            old = getattr(g, name)
            setattr(g, name, new[name].requires_grad_(old.requires_grad))        # a leaf again, .grad None
        if opt is not None:
            opt.exp_avg = {name: new[("exp_avg", name)] for name in opt.names}
            opt.exp_avg_sq = {name: new[("exp_avg_sq", name)] for name in opt.names}
        if self.scene is not None:
            self.scene.gaussians_changed()
        return counts
