"""The optimiser step of a splat fit on the GPU: ``GaussianAdam`` (gsx_adam_step, include/gsx.h).

One library call -- one kernel launch -- steps every trained array of a ``Gaussians`` container along its ``.grad``: Adam,
with the groups named in ``log_groups`` (the scales, as in the published method) stepped in log space, so that a positive
scale stays positive for any step, and optionally the published trainer's sparse rule: with ``skip_zero_rows`` a Gaussian
whose gradients are all zero -- one that reached no tile of the frame -- keeps its parameters AND its moments.  There is no
torch composition behind it and no CPU path.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Iterable, Tuple, Union

import torch

from . import _ffi
from ._device import _stream_handle

GROUP_NAMES = ("points", "scales", "quaternions", "opacity", "colors", "sh")
LearningRate = Union[float, Callable[[int], float]]


def expon_lr(lr_init: float, lr_final: float, max_steps: int) -> Callable[[int], float]:
    """The published position schedule: log-linear interpolation from ``lr_init`` at step 0 to ``lr_final`` at ``max_steps``
    and ``lr_final`` from there on.  Host arithmetic only."""
    lr_init, lr_final, max_steps = float(lr_init), float(lr_final), int(max_steps)
    if not (lr_init > 0.0 and lr_final > 0.0 and math.isfinite(lr_init) and math.isfinite(lr_final)):
        raise ValueError("expon_lr needs positive finite rates, got %r and %r" % (lr_init, lr_final))
    if max_steps < 1:
        raise ValueError("expon_lr needs max_steps >= 1, got %r" % (max_steps,))

    def rate(step: int) -> float:
        t = float(step) / max_steps
        if t <= 0.0 or t >= 1.0:            # (the ends exactly, not through exp(log(.)))
            return lr_init if t <= 0.0 else lr_final
        return math.exp((1.0 - t) * math.log(lr_init) + t * math.log(lr_final))

    return rate


class GaussianAdam:
    """Adam over the arrays of ``gaussians`` that are present, named in ``lr`` and ``requires_grad``.

    ``lr``: name -> float, or a callable of the step number (1 for the first step); ``log_groups``: names stepped in log
    space (names that are not trained are ignored; a name that is no array of the container is refused);
    ``skip_zero_rows``: GSX_ADAM_SKIP_ZERO_ROWS.  The moments (``exp_avg`` / ``exp_avg_sq``, of dL/dlog p for a log group)
    are allocated here, once; ``step()`` allocates nothing on the device."""

    def __init__(self, gaussians, lr: Dict[str, LearningRate], betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 log_groups: Iterable[str] = ("scales",), skip_zero_rows: bool = False) -> None:
        for name in lr:
            if name not in GROUP_NAMES:
                raise ValueError("lr names %r, which is no array of a Gaussians container %s" % (name, GROUP_NAMES))
        log_groups = tuple(log_groups)
        for name in log_groups:
            if name not in GROUP_NAMES:
                raise ValueError("log_groups names %r, which is no array of a Gaussians container %s" % (name, GROUP_NAMES))
        b1, b2 = float(betas[0]), float(betas[1])
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError("betas = %r are outside [0, 1)" % (betas,))
        if not (float(eps) >= 0.0 and math.isfinite(float(eps))):
            raise ValueError("eps = %r is negative or not finite" % (eps,))
        self.gaussians = gaussians
        self.names = tuple(n for n in GROUP_NAMES if n in lr and getattr(gaussians, n, None) is not None
                           and getattr(gaussians, n).requires_grad)
        if not self.names:
            raise ValueError("nothing to optimise: no array of the container is named in lr and requires grad")
        n = len(gaussians)
        for name in self.names:
            t = getattr(gaussians, name)
            if t.device.type != "cuda":
                raise ValueError("%s is on %s: the step runs only as a HIP kernel on an AMD GPU (torch device 'cuda'); "
                                 "there is no CPU fallback" % (name, t.device))
            if t.dtype != torch.float32 or not t.is_contiguous() or t.shape[0] != n:
                raise ValueError("%s must be a contiguous float32 tensor of %d rows" % (name, n))
        self.lr = {name: lr[name] for name in self.names}
        self.betas, self.eps = (b1, b2), float(eps)
        self.log_groups = tuple(name for name in self.names if name in log_groups)
        self.skip_zero_rows = bool(skip_zero_rows)
        self.step_count = 0
        self.exp_avg = {name: torch.zeros_like(getattr(gaussians, name)) for name in self.names}
        self.exp_avg_sq = {name: torch.zeros_like(getattr(gaussians, name)) for name in self.names}
        self._groups = (_ffi.GsxAdamGroup * len(self.names))()

    def _rate(self, name: str, step: int) -> float:
        rate = self.lr[name]
        return float(rate(step)) if callable(rate) else float(rate)

    def zero_grad(self, set_to_none: bool = True) -> None:
        for name in self.names:
            t = getattr(self.gaussians, name)
            if t.grad is None:
                continue
            if set_to_none:
                t.grad = None
            else:
                t.grad.detach_()
                t.grad.zero_()

    def step(self) -> None:
        g = self.gaussians
        n = len(g)
        dev = getattr(g, self.names[0]).device
        step = self.step_count + 1
        for i, name in enumerate(self.names):
            t = getattr(g, name)
            grad = t.grad
            if grad is None:
                raise ValueError("%s has no .grad: call backward() before step()" % name)
            if grad.dtype != torch.float32:
                raise ValueError("%s.grad must be float32, got %s" % (name, grad.dtype))
            if grad.device != t.device or t.device != dev:
                raise ValueError("%s.grad is on %s, %s on %s, the step on %s" % (name, grad.device, name, t.device, dev))
            if not grad.is_contiguous() or tuple(grad.shape) != tuple(t.shape):
                raise ValueError("%s.grad must be contiguous and of the shape of %s" % (name, name))
            if not t.is_contiguous() or t.shape[0] != n:
                raise ValueError("%s must be a contiguous tensor of %d rows" % (name, n))
            grp = self._groups[i]
            grp.param, grp.grad = t.data_ptr(), grad.data_ptr()
            grp.exp_avg, grp.exp_avg_sq = self.exp_avg[name].data_ptr(), self.exp_avg_sq[name].data_ptr()
            grp.width = t.numel() // n if n else max(1, math.prod(t.shape[1:]))
            grp.transform = _ffi.GSX_ADAM_LOG if name in self.log_groups else _ffi.GSX_ADAM_LINEAR
            grp.lr, grp.reserved = self._rate(name, step), 0.0
        with torch.cuda.device(dev):
            rc = _ffi.load().gsx_adam_step(self._groups, len(self.names), n, step, self.betas[0], self.betas[1], self.eps,
                                           _ffi.GSX_ADAM_SKIP_ZERO_ROWS if self.skip_zero_rows else 0, _stream_handle(dev))
        _ffi.check(rc)
        self.step_count = step
        # the library wrote through raw pointers: tell torch (Gaussians.current_block_bounds reads _version)
        for name in self.names:
            torch.autograd.graph.increment_version(getattr(g, name))

    def state_dict(self) -> dict:
        return {"step": self.step_count, "names": self.names, "log_groups": self.log_groups, "betas": self.betas,
                "eps": self.eps, "skip_zero_rows": self.skip_zero_rows,
                "lr": {k: v for k, v in self.lr.items() if not callable(v)},
                "exp_avg": {k: v.clone() for k, v in self.exp_avg.items()},
                "exp_avg_sq": {k: v.clone() for k, v in self.exp_avg_sq.items()}}

    def load_state_dict(self, state: dict) -> None:
        """Takes over the step, the moments, the hyper-parameters and which groups are LOG.  The trained groups must be the
        same; a learning rate given as a callable is not part of the state and stays this optimiser's own."""
        if tuple(state["names"]) != self.names:
            raise ValueError("the state is of the groups %s, this optimiser of %s" % (tuple(state["names"]), self.names))
        for name in self.names:
            for key in ("exp_avg", "exp_avg_sq"):
                if tuple(state[key][name].shape) != tuple(getattr(self, key)[name].shape):
                    raise ValueError("%s of %s has shape %s" % (key, name, tuple(state[key][name].shape)))
        self.step_count = int(state["step"])
        self.log_groups = tuple(state["log_groups"])
        self.betas, self.eps = (float(state["betas"][0]), float(state["betas"][1])), float(state["eps"])
        self.skip_zero_rows = bool(state["skip_zero_rows"])
        self.lr.update({k: v for k, v in state["lr"].items() if k in self.lr and not callable(self.lr[k])})
        with torch.no_grad():
            for name in self.names:
                self.exp_avg[name].copy_(state["exp_avg"][name])
                self.exp_avg_sq[name].copy_(state["exp_avg_sq"][name])
