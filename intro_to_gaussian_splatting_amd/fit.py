"""A fit loop over the parts the library has: ``Trainer``.

Every part of a splat fit is a HIP call behind a Python surface -- the differentiable frame (``render_image_hip``), the
photometric loss, ``GaussianAdam``, ``DensityControl`` and the SH degree schedule (``Gaussians.active_sh_degree``).  This
module adds no kernel and no arithmetic of its own: it fixes the ORDER of those calls, once, so that nobody has to re-derive
it.  One step, numbered from 1:

1. the view: the next index of a seeded CPU ``torch.randperm`` over ``targets``, drawn afresh for every epoch;
2. ``frame = scene.render_image_hip(idx, tile_size, geometry_gradients=True, screen_statistics=statistic == "screen")``;
3. ``loss = scene.photometric_loss(idx, frame, targets[idx], tile_size, lambda_dssim, terms=...)``;
4. ``loss.backward()``;
5. ``density.accumulate()``;
6. ``opt.step()``, then ``opt.zero_grad()``;
   With ``refine_poses`` the frame of 2 is rendered with ``camera_gradients=True`` besides, 4 leaves dL/dworld2view in
   ``scene.images[idx].world2view.grad``, and ``refiner.step()`` (``CameraRefiner``: the pose chain and its Adam step on
   the host, then ``set_world2view``) runs right here, after ``opt.zero_grad()`` and before the events: the Gaussians and
   the camera both step along gradients of the SAME frame;
7. the events ``events_at`` names for this step, in this order: ``density.densify_and_prune(generator)``,
   ``density.reset_opacity(opacity_reset_logit)``, ``gaussians.oneup_sh_degree()`` and, at the steps of
   ``prune_contribution_at``, ``density.prune_contribution(scene.contribution(indices, semantics, tile_size), threshold)``.

With ``depth_targets`` (image index -> (W,H) depth map) step 2 is ``frame, depth = scene.render_image_depth_hip(idx,
tile_size, screen_statistics=statistic == "screen")`` and step 3 adds ``lambda_depth * depth_loss(depth,
depth_targets[idx], scene.rendered_region(idx, tile_size))`` for the views that have a target; nothing else in the order
changes.  Without it every call is the one above.

With ``statistic="screen_abs"`` (the absolute screen statistic, ``DensityControl``) step 2 passes
``screen_statistics="abs"``; nothing else changes.  It is refused together with ``refine_poses`` or ``depth_targets``: the
pose and depth backward entries have no absolute statistic.

With ``masks`` (image index -> (W,H) weight) and/or ``exposure`` (an ``ExposureRefiner``) step 3 is
``scene.photometric_loss(..., weight=masks.get(idx), exposure=exposure_refiner.exposure(idx))`` -- the weighted loss of
gsx_photometric_loss_weighted, one call, with dL/dexposure left in the view's leaf by step 4 -- and
``exposure_refiner.step()`` runs in step 6 after ``opt.zero_grad()``, where the pose refiner's does; with both refiners the
pose refiner runs first.  A view that has neither a mask nor an exposure makes the call of step 3 as written there.  The depth
term is not masked.  Without the two arguments every call is the one above.

With ``strategy="mcmc"`` (fixed-budget densification, ``MCMCControl``) the order is the same and four calls differ: the frame
of step 2 is rendered with ``geometry_gradients=True`` and NO ``screen_statistics``; step 5 is ``density.regularize()``
instead of ``accumulate()``; ``density.perturb(generator)`` runs in step 6 after ``opt.zero_grad()`` and before the refiners;
the "densify" event of step 7 runs ``density.relocate(generator)``, and "opacity_reset" is never due.  The loss that is
returned stays the photometric one: the regularisers enter through their gradients only.  With ``strategy="adaptive"``, the
default, every call is the one above.

With ``semantics="std_3dgs"`` (and ``background=(r, g, b)``) step 2 passes the two to ``render_image_hip``: the frame is
the published rule set's and step 4 runs gsx_render_backward_std; the loss of step 3 covers the whole frame (that rule set
renders partial edge tiles) and ``evaluate()`` renders with the same rules.  ``statistic="screen"`` and ``strategy="mcmc"``
work as above.  ``refine_poses``, ``depth_targets`` and ``statistic="screen_abs"`` are refused together with it: the std_3dgs
backward has no pose gradient, no depth image and no absolute statistic.  With ``antialiased=True`` besides, the frames of
step 2, of ``evaluate()`` and of the "prune_contribution" event are the anti-aliased variant of that rule set
(``render_image_hip(..., antialiased=True)``: opacity times rho).  With ``semantics="ref_cpu"``, the default, every
call is the one above.

The coefficients keep ONE learning rate: a second rate for the higher bands, as published, needs an Adam group over a strided
part of ``sh`` and is not built.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Iterable, Optional, Tuple

import torch

from .density import DensityControl
from .mcmc import MCMCControl
from .exposure import ExposureRefiner
from .loss import depth_loss
from .optim import GROUP_NAMES, GaussianAdam
from .pose import CameraRefiner

EVENT_NAMES = ("densify", "opacity_reset", "sh_oneup", "prune_contribution")
# the published rates (Kerbl et al. 2023); the position rate is per unit of scene extent there: scale it for the scene, or
# move the scene into those units once, before the fit: GaussianScene.normalize()
DEFAULT_LR = {"points": 1.6e-4, "scales": 5e-3, "quaternions": 1e-3, "opacity": 5e-2, "colors": 2.5e-3, "sh": 2.5e-3}
DEFAULT_OPACITY_RESET_LOGIT = math.log(0.01 / 0.99)         # the published reset: opacity at most 0.01
STRATEGIES = ("adaptive", "mcmc")


class _Default(int):
    """The value of an argument nobody passed: an int like any other, told apart by identity."""


_OPACITY_RESET_EVERY = _Default(3000)


def _period(name: str, value) -> int:
    if value is None:
        return 0
    if isinstance(value, bool) or int(value) != value or int(value) < 0:
        raise ValueError("%s = %r is not a non-negative integer (0 or None: never)" % (name, value))
    return int(value)


def _steps(name: str, value) -> Tuple[int, ...]:
    if isinstance(value, (str, bytes)) or not isinstance(value, Iterable):
        raise ValueError("%s = %r is not a sequence of steps" % (name, value))
    out = tuple(value)
    for v in out:
        if isinstance(v, bool) or int(v) != v or int(v) < 1:
            raise ValueError("%s names %r, which is not a positive integer (the first step is 1)" % (name, v))
    return tuple(int(v) for v in out)


def events_at(step: int, sh_degree_every: Optional[int] = 1000, densify_from: int = 500, densify_every: Optional[int] = 100,
              densify_until: int = 15000, opacity_reset_every: Optional[int] = 3000,
              prune_contribution_at: Optional[Iterable[int]] = None) -> Tuple[str, ...]:
    """The events due after the optimiser step of ``step`` (1 for the first), in the order they run -- a pure function:
    "densify"        ``densify_from < step <= densify_until`` and ``step`` a multiple of ``densify_every``;
    "opacity_reset"  ``step <= densify_until`` and ``step`` a multiple of ``opacity_reset_every``;
    "sh_oneup"       ``step`` a multiple of ``sh_degree_every``;
    "prune_contribution"  ``step`` is one of ``prune_contribution_at`` (None, the default: never).
    A period of 0 or None switches its event off."""
    if isinstance(step, bool) or int(step) != step or int(step) < 1:
        raise ValueError("step = %r is not a positive integer (the first step is 1)" % (step,))
    step = int(step)
    sh_every, d_every, o_every = (_period("sh_degree_every", sh_degree_every), _period("densify_every", densify_every),
                                  _period("opacity_reset_every", opacity_reset_every))
    due = []
    if d_every and int(densify_from) < step <= int(densify_until) and step % d_every == 0:
        due.append("densify")
    if o_every and step <= int(densify_until) and step % o_every == 0:
        due.append("opacity_reset")
    if sh_every and step % sh_every == 0:
        due.append("sh_oneup")
    if prune_contribution_at is not None and step in _steps("prune_contribution_at", prune_contribution_at):
        due.append("prune_contribution")
    return tuple(due)


def _check_depth_targets(scene, targets, depth_targets, lambda_depth, refine_poses):
    """(dict or None, float): ``Trainer``'s ``depth_targets`` and ``lambda_depth``, refused by name."""
    lam = float(lambda_depth)
    if not (lam >= 0.0 and math.isfinite(lam)):
        raise ValueError("lambda_depth = %r is not a finite non-negative number" % (lambda_depth,))
    if depth_targets is None:
        if lam != 0.0:
            raise ValueError("lambda_depth = %r without depth_targets: there is no depth to weigh" % (lambda_depth,))
        return None, 0.0
    if refine_poses is not None:
        raise ValueError("depth_targets cannot be combined with refine_poses: render_image_depth_hip has no pose gradient")
    out = dict(depth_targets)
    for idx, t in out.items():
        if idx not in targets:
            raise ValueError("depth_targets names image %r, which targets does not have" % (idx,))
        cam = scene.images[idx].gsx_camera()
        want = (int(cam.width), int(cam.height))
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != want:
            raise ValueError("depth_targets[%r] must be a float32 tensor of shape %s (W, H), got %s" % (
                idx, want, "%s %s" % (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__))
        if t.device != scene.gaussians.points.device:
            raise ValueError("depth_targets[%r] is on %s, the scene's Gaussians on %s" % (idx, t.device,
                                                                                         scene.gaussians.points.device))
    return out, lam


def _check_masks(scene, targets, masks):
    """dict or None: ``Trainer``'s ``masks``, refused by name."""
    if masks is None:
        return None
    out = dict(masks)
    for idx, t in out.items():
        if idx not in targets:
            raise ValueError("masks names image %r, which targets does not have" % (idx,))
        cam = scene.images[idx].gsx_camera()
        want = (int(cam.width), int(cam.height))
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != want:
            raise ValueError("masks[%r] must be a float32 tensor of shape %s (W, H), got %s" % (
                idx, want, "%s %s" % (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__))
        if t.device != scene.gaussians.points.device:
            raise ValueError("masks[%r] is on %s, the scene's Gaussians on %s" % (idx, t.device,
                                                                                 scene.gaussians.points.device))
    return out


class Trainer:
    """Fits ``scene.gaussians`` to ``targets`` (image index -> (W,H,3) float32 tensor on the scene's GPU, the layout of
    ``render_image_hip``) with the composition of this module's docstring.

    ``lr``: name -> rate or callable of the step, as ``GaussianAdam`` takes it; the arrays it names that the container holds
    are set to require grad (an SH container trains ``sh``, never ``colors``).  ``statistic`` and ``density`` (keyword
    arguments) go to ``DensityControl``.  ``seed`` seeds both the view order (CPU) and the split positions (device).
    The schedule arguments are ``events_at``'s.  ``opt`` and ``density`` are public: their knobs may be changed between steps.
    ``refine_poses``: None (every call and every bit as without it), or a dict of ``CameraRefiner`` keywords
    (``lr_rotation`` and ``lr_translation`` are required there; ``indices`` defaults to the views of ``targets``): the
    cameras are refined beside the Gaussians, ``refiner`` is public.
    ``depth_targets``: None (every call and every bit as without it), or a dict image index -> (W,H) float32 depth map on
    the scene's GPU, view-space depth, 0 where unknown: the step renders ``render_image_depth_hip`` and adds
    ``lambda_depth * depth_loss`` over the rendered region for the views the dict names.  Not with ``refine_poses``: the
    pose has no gradient through depth.
    ``masks``: None, or a dict image index -> (W,H) float32 weight on the scene's GPU, finite and >= 0 (``photometric_loss``'s
    ``weight``); views it does not name are unweighted.  ``exposure``: None, or a dict of ``ExposureRefiner`` keywords
    (``lr`` is required there; ``indices`` defaults to the views of ``targets``): a (3, 4) colour transform per view is
    learned beside the Gaussians, ``exposure_refiner`` is public.  With both None every call and every bit is as without
    them.  The masks weigh the photometric term alone: the depth term is NOT masked.
    ``strategy``: ``"adaptive"`` (default: ``DensityControl``, every call and every bit as without the argument) or
    ``"mcmc"``: fixed-budget densification, ``density`` is then an ``MCMCControl`` built with the keywords of ``mcmc`` (a
    dict; ``cap_max`` is required there).  The "densify" event runs ``relocate()`` and there is no opacity reset: an explicit
    ``opacity_reset_every``, ``density=`` or ``statistic=`` is refused together with ``"mcmc"``, as is ``mcmc=`` without it.
    ``semantics``: ``"ref_cpu"`` (default: every call and every bit as without the argument) or ``"std_3dgs"``: the frames
    are rendered, differentiated and evaluated under the published rule set over ``background`` (r, g, b), and the loss
    covers the whole frame.  ``refine_poses``, ``depth_targets`` and ``statistic="screen_abs"`` are refused together with it;
    a ``background`` other than black is refused without it (the ref_cpu frame has none).
    ``antialiased`` (``semantics="std_3dgs"`` only; ValueError otherwise): every frame the Trainer renders -- ``step()``,
    ``evaluate()`` and the contribution sweep -- is the anti-aliased variant (``render_image_hip(..., antialiased=True)``).
    False, the default: every call and every bit as without the argument.
    ``prune_contribution_at``: None (every call and every bit as without it), or the steps after which the fit prunes by
    contribution: ``scene.contribution(indices)`` sweeps the views (``prune_contribution["indices"]``; None: every view of
    the scene) under the Trainer's ``semantics`` and tile size -- the background changes no blend weight -- and
    ``density.prune_contribution(...)`` drops what shows below ``prune_contribution["threshold"]`` (0.01) in all of them.
    ``prune_contribution`` (None: ``dict(threshold=0.01, indices=None)``) is read by that event alone.
    Refused with ``strategy="mcmc"``: a fixed budget relocates and does not prune."""

    def __init__(self, scene, targets: Dict[int, torch.Tensor], lr: Optional[dict] = None, lambda_dssim: float = 0.2,
                 tile_size: int = 16, statistic: Optional[str] = None, density: Optional[dict] = None,
                 sh_degree_every: Optional[int] = 1000, densify_from: int = 500, densify_every: Optional[int] = 100,
                 densify_until: int = 15000, opacity_reset_every: Optional[int] = _OPACITY_RESET_EVERY,
                 opacity_reset_logit: float = DEFAULT_OPACITY_RESET_LOGIT, seed: int = 0,
                 refine_poses: Optional[dict] = None, depth_targets: Optional[Dict[int, torch.Tensor]] = None,
                 lambda_depth: float = 0.0, masks: Optional[Dict[int, torch.Tensor]] = None,
                 exposure: Optional[dict] = None, strategy: str = "adaptive", mcmc: Optional[dict] = None,
                 semantics: str = "ref_cpu", background: Tuple[float, float, float] = (0.0, 0.0, 0.0),
                 prune_contribution_at: Optional[Iterable[int]] = None, prune_contribution: Optional[dict] = None,
                 antialiased: bool = False) -> None:
        g = scene.gaussians
        if prune_contribution_at is not None:
            prune_contribution_at = _steps("prune_contribution_at", prune_contribution_at)
            if strategy == "mcmc":
                raise ValueError("prune_contribution_at cannot be combined with strategy='mcmc': a fixed budget relocates "
                                 "and does not prune (MCMCControl has no prune_contribution)")
        pc = dict(threshold=0.01, indices=None)                 # (without prune_contribution_at no step reads it)
        for key, value in dict(prune_contribution or {}).items():
            if key not in pc:
                raise ValueError("prune_contribution names %r: it takes threshold and indices" % (key,))
            pc[key] = value
        if pc["indices"] is not None:
            pc["indices"] = list(pc["indices"])
            for idx in pc["indices"]:
                if idx not in scene.images:
                    raise ValueError("prune_contribution['indices'] names image %r, which the scene does not have" % (idx,))
        self.prune_contribution = pc
        if semantics not in ("ref_cpu", "std_3dgs"):
            raise ValueError("semantics = %r is neither 'ref_cpu' nor 'std_3dgs': no other frame is differentiable" % (semantics,))
        background = tuple(float(v) for v in background)
        if len(background) != 3:
            raise ValueError("background = %r is not (r, g, b)" % (background,))
        if semantics == "ref_cpu" and any(background):
            raise ValueError("background = %r needs semantics='std_3dgs': the ref_cpu frame has no background" % (background,))
        if semantics == "std_3dgs":
            for name, given in (("refine_poses", refine_poses is not None), ("depth_targets", depth_targets is not None),
                                ("statistic='screen_abs'", statistic == "screen_abs")):
                if given:
                    raise ValueError("%s cannot be combined with semantics='std_3dgs': gsx_render_backward_std has no pose "
                                     "gradient, no depth image and no absolute statistic" % name)
        if antialiased and semantics != "std_3dgs":
            raise ValueError("antialiased=True needs semantics='std_3dgs', got semantics=%r: the opacity compensation is a "
                             "variant of the published rule set" % (semantics,))
        self.semantics, self.background, self.antialiased = semantics, background, bool(antialiased)
        # (passed only when set: without it every call is the one it was)
        self._std_kw = dict(antialiased=True) if self.antialiased else {}
        if strategy not in STRATEGIES:
            raise ValueError("strategy = %r is neither 'adaptive' nor 'mcmc'" % (strategy,))
        if strategy == "mcmc":
            if density is not None:
                raise ValueError("density= goes to DensityControl, the adaptive strategy: with strategy='mcmc' pass mcmc=")
            if statistic is not None:
                raise ValueError("statistic= is the adaptive strategy's: strategy='mcmc' needs no densification statistic")
            if opacity_reset_every is not _OPACITY_RESET_EVERY:
                raise ValueError("opacity_reset_every cannot be combined with strategy='mcmc': it has no opacity reset")
            if mcmc is None or "cap_max" not in dict(mcmc):
                raise ValueError("strategy='mcmc' needs mcmc=dict(cap_max=...): the budget has no default")
            opacity_reset_every = None
        else:
            if mcmc is not None:
                raise ValueError("mcmc= goes to MCMCControl: pass strategy='mcmc' with it")
            if statistic is None:
                statistic = "screen"
            if statistic == "screen_abs" and (refine_poses is not None or depth_targets is not None):
                raise ValueError("statistic='screen_abs' cannot be combined with refine_poses or depth_targets: neither "
                                 "gsx_render_backward_camera nor gsx_render_backward_depth has the absolute statistic")
            if opacity_reset_every is _OPACITY_RESET_EVERY:
                opacity_reset_every = int(opacity_reset_every)
        if not targets:
            raise ValueError("targets is empty: nothing to fit")
        for idx in targets:
            if idx not in scene.images:
                raise ValueError("targets names image %r, which the scene does not have" % (idx,))
        lr = dict(DEFAULT_LR if lr is None else lr)
        for name in lr:
            if name not in GROUP_NAMES:
                raise ValueError("lr names %r, which is no array of a Gaussians container %s" % (name, GROUP_NAMES))
        has_sh = getattr(g, "sh", None) is not None
        lr.pop("colors" if has_sh else "sh", None)              # the frame reads one of the two
        if not 0.0 <= float(lambda_dssim) <= 1.0:
            raise ValueError("lambda_dssim = %r is outside [0, 1]" % (lambda_dssim,))
        self.depth_targets, self.lambda_depth = _check_depth_targets(scene, targets, depth_targets, lambda_depth, refine_poses)
        self.masks = _check_masks(scene, targets, masks)
        if exposure is not None and "lr" not in dict(exposure):
            raise ValueError("exposure needs an lr: ExposureRefiner has no default rate")
        self._schedule = dict(sh_degree_every=sh_degree_every, densify_from=int(densify_from), densify_every=densify_every,
                              densify_until=int(densify_until), opacity_reset_every=opacity_reset_every)
        if prune_contribution_at is not None:                   # (without it the schedule is the one it always was)
            self._schedule["prune_contribution_at"] = prune_contribution_at
        events_at(1, **self._schedule)                          # refuses a bad period here, not at step 1000
        for name in lr:
            if getattr(g, name, None) is not None:
                getattr(g, name).requires_grad_(True)
        self.scene, self.gaussians, self.targets = scene, g, dict(targets)
        self.lambda_dssim, self.tile_size, self.statistic = float(lambda_dssim), int(tile_size), statistic
        self.opacity_reset_logit = float(opacity_reset_logit)
        self.opt = GaussianAdam(g, lr=lr)
        self.strategy = strategy
        if strategy == "mcmc":
            self.density = MCMCControl(g, optimizer=self.opt, scene=scene, **dict(mcmc))
        else:
            self.density = DensityControl(g, optimizer=self.opt, scene=scene, statistic=statistic, **(density or {}))
        self.refiner = None
        if refine_poses is not None:
            kw = dict(refine_poses)
            self.refiner = CameraRefiner(scene, kw.pop("indices", sorted(self.targets)), **kw)
        self.exposure_refiner = None
        if exposure is not None:
            kw = dict(exposure)
            self.exposure_refiner = ExposureRefiner(scene, kw.pop("indices", sorted(self.targets)), **kw)
        self.step_count = 0
        self._views = sorted(self.targets)
        self._order: list = []
        self._view_generator = torch.Generator(device="cpu").manual_seed(int(seed))
        self._split_generator = torch.Generator(device=g.points.device).manual_seed(int(seed))

    def events_at(self, step: int) -> Tuple[str, ...]:
        return events_at(step, **self._schedule)

    def _weighting(self, idx: int) -> dict:
        """The ``weight`` and ``exposure`` keywords of view ``idx``'s loss call; empty when it has neither."""
        kw = {}
        if self.masks is not None and idx in self.masks:
            kw["weight"] = self.masks[idx]
        if self.exposure_refiner is not None and idx in self.exposure_refiner.exposures:
            kw["exposure"] = self.exposure_refiner.exposure(idx)
        return kw

    def _next_view(self) -> int:
        if not self._order:     # a new epoch: every view once, in a fresh order
            self._order = [self._views[i] for i in torch.randperm(len(self._views), generator=self._view_generator).tolist()]
        return self._order.pop(0)

    def step(self) -> Tuple[torch.Tensor, int]:
        """One step.  Returns ((3,) device tensor: loss, l1, ssim; the view): nothing is read back to the host here."""
        scene, g = self.scene, self.gaussians
        idx = self._next_view()
        depth = None
        region_kw = {}
        if self.semantics == "std_3dgs":
            frame = scene.render_image_hip(idx, tile_size=self.tile_size, geometry_gradients=True,
                                           screen_statistics=self.statistic == "screen", semantics=self.semantics,
                                           background=self.background, **self._std_kw)
            region_kw = dict(semantics=self.semantics)
        elif self.depth_targets is not None:
            frame, depth = scene.render_image_depth_hip(idx, tile_size=self.tile_size,
                                                        screen_statistics=self.statistic == "screen")
        elif self.statistic == "screen_abs":
            frame = scene.render_image_hip(idx, tile_size=self.tile_size, geometry_gradients=True, screen_statistics="abs")
        elif self.refiner is None:
            frame = scene.render_image_hip(idx, tile_size=self.tile_size, geometry_gradients=True,
                                           screen_statistics=self.statistic == "screen")
        else:
            frame = scene.render_image_hip(idx, tile_size=self.tile_size, geometry_gradients=True,
                                           screen_statistics=self.statistic == "screen", camera_gradients=True)
        terms: dict = {}
        loss = scene.photometric_loss(idx, frame, self.targets[idx], tile_size=self.tile_size,
                                      lambda_dssim=self.lambda_dssim, terms=terms, **self._weighting(idx), **region_kw)
        if depth is not None and idx in self.depth_targets:
            loss = loss + self.lambda_depth * depth_loss(depth, self.depth_targets[idx],
                                                         scene.rendered_region(idx, self.tile_size))
        loss.backward()
        if self.strategy == "mcmc":
            self.density.regularize()
        else:
            self.density.accumulate()
        self.opt.step()
        self.opt.zero_grad()
        if self.strategy == "mcmc":
            self.density.perturb(generator=self._split_generator)
        if self.refiner is not None:
            self.refiner.step()
        if self.exposure_refiner is not None:
            self.exposure_refiner.step()
        self.step_count += 1
        for event in self.events_at(self.step_count):
            if event == "densify" and self.strategy == "mcmc":
                self.density.relocate(generator=self._split_generator)
            elif event == "densify":
                self.density.densify_and_prune(generator=self._split_generator)
            elif event == "opacity_reset":
                self.density.reset_opacity(self.opacity_reset_logit)
            elif event == "prune_contribution":
                pc = self.prune_contribution
                con = scene.contribution(pc["indices"], semantics=self.semantics, tile_size=self.tile_size, **self._std_kw)
                self.density.prune_contribution(con, threshold=pc["threshold"])
            else:
                g.oneup_sh_degree()
        return torch.stack((loss.detach(), terms["l1"], terms["ssim"])), idx

    def fit(self, steps: int, callback: Optional[Callable] = None) -> None:
        """``steps`` steps; ``callback(trainer, losses, view)`` after each, with what ``step()`` returned."""
        for _ in range(int(steps)):
            losses, idx = self.step()
            if callback is not None:
                callback(self, losses, idx)

    def evaluate(self, indices: Optional[Iterable[int]] = None) -> Dict[int, Dict[str, float]]:
        """image index -> ``l1``, ``ssim`` (the loss's own terms) and ``psnr`` (dB, peak 1) of the current frame against its
        target over ``rendered_region``, under ``no_grad``; one host read per view.  A view with a mask or an exposure is
        measured as it is trained: the loss terms are the weighted ones, and the PSNR is that of the exposure-corrected
        frame with the mask's weights, ``mse = sum m (x' - y)^2 / (3 sum m)`` (infinite when every weight is zero)."""
        out = {}
        with torch.no_grad():
            for idx in (self._views if indices is None else indices):
                target = self.targets[idx]
                std = self.semantics == "std_3dgs"
                if std:
                    frame = self.scene.render_image_hip(idx, tile_size=self.tile_size, semantics=self.semantics,
                                                        background=self.background, **self._std_kw)
                else:
                    frame = self.scene.render_image_hip(idx, tile_size=self.tile_size)
                terms: dict = {}
                kw = self._weighting(idx)
                region_kw = dict(semantics=self.semantics) if std else {}
                self.scene.photometric_loss(idx, frame, target, tile_size=self.tile_size, lambda_dssim=self.lambda_dssim,
                                            terms=terms, **kw, **region_kw)
                a, b = self.scene.rendered_region(idx, self.tile_size, **region_kw)
                if not kw:
                    mse = ((frame[:a, :b] - target[:a, :b]) ** 2).mean()
                else:
                    shown = frame[:a, :b]
                    if "exposure" in kw:
                        E = kw["exposure"].detach()
                        shown = shown @ E[:, :3].t() + E[:, 3]
                    sq = ((shown - target[:a, :b]) ** 2).sum(dim=2)
                    if "weight" in kw:
                        m = kw["weight"][:a, :b]
                        mse = (m * sq).sum() / (3.0 * m.sum())      # 0 / 0 = NaN with every weight zero: reported as inf
                    else:
                        mse = sq.mean() / 3.0
                l1, ssim, mse = (float(v) for v in torch.stack((terms["l1"], terms["ssim"], mse)).tolist())
                out[idx] = dict(l1=l1, ssim=ssim, psnr=math.inf if (mse == 0.0 or mse != mse) else -10.0 * math.log10(mse))
        return out
