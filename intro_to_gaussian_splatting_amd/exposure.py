"""Per-view exposure: ``ExposureRefiner`` keeps one (3, 4) affine colour transform per view and steps it along dL/dexposure.

Photographs of one scene differ in exposure and white balance from shot to shot; a fit that has no term for it lets the
Gaussians absorb the difference as floaters.  ``photometric_loss(..., exposure=E)`` applies ``x' = E[:, :3] x + E[:, 3]`` to
the frame inside the loss call and, when ``E`` requires grad, leaves dL/dE in ``E.grad`` (gsx_photometric_loss_weighted: the
twelve sums come out of the same call, no torch composition).  This module holds the leaves, on the scene's device, each
``[I | 0]`` at the start, and one ``torch.optim.Adam`` per view: twelve floats per view are no hot path and get no kernel.

No learning rate is a default: this project has measured none.
"""
from __future__ import annotations

import copy
from typing import Callable, Dict, Iterable, Optional, Tuple, Union

import torch


class ExposureRefiner:
    """Adam on the exposures of ``indices`` (default: every image of the scene).  ``lr``: a float, or a callable of the
    view's step number (1 for its first step), so that ``optim.expon_lr`` fits.

    ``exposure(idx)``: the view's (3, 4) leaf, to be passed to ``photometric_loss(..., exposure=)``.
    ``step()``: every view whose leaf holds a gradient takes one Adam step (its own step count and moments) and has the
    gradient cleared; a view whose grad is None is left alone, moments and step count included.  Nothing is read back."""

    def __init__(self, scene, indices: Optional[Iterable[int]] = None, *, lr: Union[float, Callable[[int], float]],
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8) -> None:
        self.scene = scene
        self.indices = sorted(scene.images) if indices is None else [i for i in indices]
        for idx in self.indices:
            if idx not in scene.images:
                raise ValueError("indices names image %r, which the scene does not have" % (idx,))
        if not callable(lr) and not float(lr) >= 0.0:
            raise ValueError("lr must be non-negative (or a callable of the step)")
        b1, b2 = float(betas[0]), float(betas[1])
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0) or not float(eps) > 0.0:
            raise ValueError("betas must lie in [0, 1) and eps must be positive")
        self.lr = lr if callable(lr) else float(lr)
        self.betas, self.eps = (b1, b2), float(eps)
        device = scene.gaussians.points.device
        self.exposures: Dict[int, torch.Tensor] = {}
        self.steps: Dict[int, int] = {}
        self._opts: Dict[int, torch.optim.Adam] = {}
        for idx in self.indices:
            leaf = torch.eye(3, 4, dtype=torch.float32, device=device).requires_grad_(True)
            self.exposures[idx] = leaf
            self.steps[idx] = 0
            self._opts[idx] = torch.optim.Adam([leaf], lr=self._rate(1), betas=self.betas, eps=self.eps)

    def _rate(self, step: int) -> float:
        return float(self.lr(step)) if callable(self.lr) else self.lr

    def exposure(self, idx: int) -> torch.Tensor:
        """The (3, 4) leaf of view ``idx``."""
        return self.exposures[idx]

    def step(self) -> int:
        """Steps every refined view that holds a gradient and clears it; returns how many did."""
        stepped = 0
        for idx in self.indices:
            leaf = self.exposures[idx]
            if leaf.grad is None:
                continue
            self.steps[idx] += 1
            opt = self._opts[idx]
            opt.param_groups[0]["lr"] = self._rate(self.steps[idx])
            opt.step()
            leaf.grad = None
            stepped += 1
        return stepped

    def state_dict(self) -> dict:
        views = {idx: dict(exposure=self.exposures[idx].detach().clone(), step=self.steps[idx],
                           adam=copy.deepcopy(self._opts[idx].state_dict())) for idx in self.indices}
        return dict(views=views, lr=self.lr, betas=self.betas, eps=self.eps)

    def load_state_dict(self, state: dict) -> None:
        """Takes over the exposures, moments, step counts and rate of ``state`` (its views must be this refiner's)."""
        if sorted(state["views"]) != sorted(self.indices):
            raise ValueError("the state holds views %s, this refiner refines %s" % (sorted(state["views"]), sorted(self.indices)))
        self.lr = state["lr"] if callable(state["lr"]) else float(state["lr"])
        self.betas, self.eps = (float(state["betas"][0]), float(state["betas"][1])), float(state["eps"])
        for idx, src in state["views"].items():
            leaf = self.exposures[idx]
            with torch.no_grad():
                leaf.copy_(src["exposure"].to(leaf.device, torch.float32))
            leaf.grad = None
            self.steps[idx] = int(src["step"])
            self._opts[idx].load_state_dict(copy.deepcopy(src["adam"]))
            group = self._opts[idx].param_groups[0]
            group["betas"], group["eps"] = self.betas, self.eps


__all__ = ["ExposureRefiner"]
