"""Pose refinement: ``CameraRefiner`` steps the cameras of a ``GaussianScene`` along dL/dworld2view.

``render_image_hip(..., camera_gradients=True)`` leaves the total derivative of a loss with respect to a view's
``world2view`` in that tensor's ``.grad`` (gsx_render_backward_camera).  A pose has six degrees of freedom, not sixteen:
this module keeps, per refined view, float64 HOST parameters (omega, tau), both zero at the start, with

    R = exp([omega]x) R0        T = T0 + tau        world2view = [[R, T], [0, 1]]^T

(R0, T0: the view's pose when the refiner was built; [omega]x the skew matrix of omega), carries the 4x4 gradient through
that map in float64 on the CPU, takes an Adam step with state per view and hands the new matrix to
``GaussianImage.set_world2view``.  There is no kernel here: the poses are six numbers per view, and the one device read per
step and view is the 16 floats of the gradient.

No learning rate is a default: the published method does not refine poses, and this project has measured none.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Optional, Tuple

import torch


def _skew(w: torch.Tensor) -> torch.Tensor:
    z = torch.zeros((), dtype=w.dtype)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def pose_matrix(omega: torch.Tensor, tau: torch.Tensor, R0: torch.Tensor, T0: torch.Tensor) -> torch.Tensor:
    """world2view (4,4) of the parameters, in their dtype (float64 here): rows 0..2 hold R^T, row 3 holds T."""
    R = torch.linalg.matrix_exp(_skew(omega)) @ R0
    top = torch.cat([R.t(), torch.zeros((3, 1), dtype=R.dtype)], dim=1)
    bottom = torch.cat([T0 + tau, torch.ones(1, dtype=R.dtype)]).unsqueeze(0)
    return torch.cat([top, bottom], dim=0)


def pose_gradient(omega: torch.Tensor, tau: torch.Tensor, R0: torch.Tensor, T0: torch.Tensor,
                  grad_world2view: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dL/domega, dL/dtau) from dL/dworld2view (4,4), all float64 on the CPU: the chain through ``pose_matrix`` by
    autograd of its nine torch operations (matrix_exp is smooth at omega = 0, where the refiner starts)."""
    with torch.enable_grad():
        w = omega.detach().clone().requires_grad_(True)
        t = tau.detach().clone().requires_grad_(True)
        V = pose_matrix(w, t, R0, T0)
        gw, gt = torch.autograd.grad((V * grad_world2view).sum(), [w, t])
    return gw, gt


class CameraRefiner:
    """Adam on the poses of ``indices`` (default: every image of the scene).  ``lr_rotation`` (per radian of omega) and
    ``lr_translation`` (per scene unit of tau) are required.  The refined views' ``world2view`` are set to require grad.

    ``step()``: for every refined view whose ``world2view.grad`` is set -- one host read of its 16 floats, the chain to
    (omega, tau), one Adam step (bias-corrected, per-view step count), ``set_world2view`` of the new pose, grad cleared
    (the new tensor is a fresh leaf).  A view whose grad is None is left alone, moments and step count included."""

    def __init__(self, scene, indices: Optional[Iterable[int]] = None, *, lr_rotation: float, lr_translation: float,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8) -> None:
        self.scene = scene
        self.indices = sorted(scene.images) if indices is None else [i for i in indices]
        for idx in self.indices:
            if idx not in scene.images:
                raise ValueError("indices names image %r, which the scene does not have" % (idx,))
        if not (float(lr_rotation) >= 0.0 and float(lr_translation) >= 0.0):
            raise ValueError("lr_rotation and lr_translation must be non-negative")
        b1, b2 = float(betas[0]), float(betas[1])
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0) or not float(eps) > 0.0:
            raise ValueError("betas must lie in [0, 1) and eps must be positive")
        self.lr_rotation, self.lr_translation = float(lr_rotation), float(lr_translation)
        self.betas, self.eps = (b1, b2), float(eps)
        self.state: Dict[int, dict] = {}
        for idx in self.indices:
            ext = scene.images[idx].extrinsic_matrix.detach().to("cpu", torch.float64)
            self.state[idx] = dict(R0=ext[:3, :3].clone(), T0=ext[:3, 3].clone(), omega=torch.zeros(3, dtype=torch.float64),
                                   tau=torch.zeros(3, dtype=torch.float64), exp_avg=torch.zeros(6, dtype=torch.float64),
                                   exp_avg_sq=torch.zeros(6, dtype=torch.float64), step=0)
            scene.images[idx].world2view.requires_grad_(True)

    def world2view(self, idx: int) -> torch.Tensor:
        """The float32 (4,4) matrix of view ``idx``'s current parameters (what ``step`` hands to ``set_world2view``)."""
        st = self.state[idx]
        return pose_matrix(st["omega"], st["tau"], st["R0"], st["T0"]).to(torch.float32)

    def step(self) -> int:
        """Steps every refined view that holds a gradient; returns how many did."""
        stepped = 0
        b1, b2 = self.betas
        lr = torch.tensor([self.lr_rotation] * 3 + [self.lr_translation] * 3, dtype=torch.float64)
        for idx in self.indices:
            image = self.scene.images[idx]
            grad = image.world2view.grad
            if grad is None:
                continue
            st = self.state[idx]
            G = grad.detach().to("cpu", torch.float64)             # the one host read
            g = torch.cat(pose_gradient(st["omega"], st["tau"], st["R0"], st["T0"], G))
            st["step"] += 1
            st["exp_avg"] = b1 * st["exp_avg"] + (1.0 - b1) * g
            st["exp_avg_sq"] = b2 * st["exp_avg_sq"] + (1.0 - b2) * g * g
            m_hat = st["exp_avg"] / (1.0 - b1 ** st["step"])
            v_hat = st["exp_avg_sq"] / (1.0 - b2 ** st["step"])
            delta = lr * m_hat / (torch.sqrt(v_hat) + self.eps)
            st["omega"] = st["omega"] - delta[:3]
            st["tau"] = st["tau"] - delta[3:]
            image.world2view.grad = None
            image.set_world2view(self.world2view(idx))
            stepped += 1
        return stepped

    def state_dict(self) -> dict:
        views = {idx: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()} for idx, st in self.state.items()}
        return dict(views=views, lr_rotation=self.lr_rotation, lr_translation=self.lr_translation, betas=self.betas,
                    eps=self.eps)

    def load_state_dict(self, state: dict) -> None:
        """Takes over the parameters, moments, step counts and rates of ``state`` (its views must be this refiner's) and
        moves every refined camera to the pose its parameters give."""
        if sorted(state["views"]) != sorted(self.indices):
            raise ValueError("the state holds views %s, this refiner refines %s" % (sorted(state["views"]), sorted(self.indices)))
        self.lr_rotation, self.lr_translation = float(state["lr_rotation"]), float(state["lr_translation"])
        self.betas, self.eps = (float(state["betas"][0]), float(state["betas"][1])), float(state["eps"])
        for idx, src in state["views"].items():
            self.state[idx] = {k: (v.detach().to("cpu", torch.float64).clone() if torch.is_tensor(v) else int(v))
                               for k, v in src.items()}
            self.scene.images[idx].set_world2view(self.world2view(idx))


__all__ = ["CameraRefiner", "pose_matrix", "pose_gradient"]
