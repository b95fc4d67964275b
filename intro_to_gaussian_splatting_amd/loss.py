"""The photometric loss of a splat fit on the GPU: ``photometric_loss`` (gsx_photometric_loss, include/gsx.h).

``L = (1 - lambda) mean|frame - target| + lambda (1 - mean SSIM(frame, target))`` with the 11 x 11 Gaussian window of
sigma 1.5, over a region at the origin of the two images -- under ``ref_cpu`` rules the last tile row and column of a frame
are never rendered, and a loss over the whole frame would pull every Gaussian near the border toward black
(``GaussianScene.rendered_region`` / ``GaussianScene.photometric_loss``).  Value and dL/dframe come out of ONE library call;
there is no torch composition behind it and no CPU path.  For photographs the same function takes a per-pixel ``weight`` and
a per-view ``exposure`` (gsx_photometric_loss_weighted): weighted means, an affine colour transform of the frame, and
dL/dexposure from the same call.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _ffi
from ._device import _WORKSPACE, _ptr, _stream_handle


def _check_image(name: str, t: torch.Tensor, device: Optional[torch.device] = None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("%s must have shape (A, B, 3), got %s" % (name, tuple(t.shape)))
    if device is not None and t.device != device:
        raise ValueError("%s is on %s, expected %s" % (name, t.device, device))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def _call(frame: torch.Tensor, target: torch.Tensor, lam: float, region: Tuple[int, int], with_grad: bool):
    """(loss_out (3,) = loss, l1, ssim; dL/dframe of the frame's shape with zeros outside the region, or None)."""
    lib = _ffi.load()
    dev = frame.device
    a, b = region
    stride = int(frame.shape[1]) * 3
    out = torch.empty(3, dtype=torch.float32, device=dev)
    grad = None
    if with_grad:
        whole = (a, b) == (int(frame.shape[0]), int(frame.shape[1]))
        grad = (torch.empty if whole else torch.zeros)(frame.shape, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nbytes = lib.gsx_photometric_loss_workspace_bytes(a, b, 1 if with_grad else 0)
        if nbytes == 0:
            raise _ffi.GsxError(_ffi.GSX_ERR_INVALID_ARGUMENT, "gsx_photometric_loss_workspace_bytes rejected the region %s" % (region,))
        ws = _WORKSPACE.get(dev, nbytes)
        rc = lib.gsx_photometric_loss(_ptr(frame), stride, _ptr(target), stride, a, b, lam, _ptr(out), _ptr(grad), stride,
                                      _ptr(ws), nbytes, _stream_handle(dev))
    _ffi.check(rc)
    return out, grad


class _PhotometricLossFunction(torch.autograd.Function):
    """Forward: value and dL/dframe in the one library call, the gradient saved; backward: grad_output times it."""

    @staticmethod
    def forward(ctx, frame, target, lam, region):
        out, grad = _call(frame.detach(), target, lam, region, True)
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms):
        (grad,) = ctx.saved_tensors
        return grad_loss * grad, None, None, None


def _check_weight(weight, frame: torch.Tensor) -> torch.Tensor:
    if not isinstance(weight, torch.Tensor):
        raise TypeError("weight must be a torch.Tensor, got %s" % type(weight).__name__)
    if weight.dtype != torch.float32:
        raise TypeError("weight must be float32, got %s" % weight.dtype)
    if tuple(weight.shape) != tuple(frame.shape[:2]):
        raise ValueError("weight must have shape %s, the frame's two leading axes, got %s" % (
            tuple(frame.shape[:2]), tuple(weight.shape)))
    if weight.device != frame.device:
        raise ValueError("weight is on %s, expected %s" % (weight.device, frame.device))
    if not weight.is_contiguous():
        raise ValueError("weight must be contiguous")
    if weight.requires_grad:
        raise ValueError("weight requires grad: photometric_loss does not differentiate the weight (pass weight.detach())")
    return weight


def _check_exposure(exposure, frame: torch.Tensor) -> torch.Tensor:
    if not isinstance(exposure, torch.Tensor):
        raise TypeError("exposure must be a torch.Tensor, got %s" % type(exposure).__name__)
    if exposure.dtype != torch.float32:
        raise TypeError("exposure must be float32, got %s" % exposure.dtype)
    if tuple(exposure.shape) != (3, 4):
        raise ValueError("exposure must have shape (3, 4), got %s" % (tuple(exposure.shape),))
    if exposure.device != frame.device:
        raise ValueError("exposure is on %s, expected %s" % (exposure.device, frame.device))
    return exposure


def _call_weighted(frame: torch.Tensor, target: torch.Tensor, lam: float, region: Tuple[int, int], with_grad: bool,
                   weight: Optional[torch.Tensor], exposure: Optional[torch.Tensor], with_grad_exposure: bool = False):
    """gsx_photometric_loss_weighted: (loss_out (4,) = loss, l1, ssim, W; dL/dframe with zeros outside the region, or None;
    dL/dexposure (3, 4), or None)."""
    lib = _ffi.load()
    dev = frame.device
    a, b = region
    stride = int(frame.shape[1]) * 3
    out = torch.empty(4, dtype=torch.float32, device=dev)
    grad = grad_e = None
    if with_grad:
        whole = (a, b) == (int(frame.shape[0]), int(frame.shape[1]))
        grad = (torch.empty if whole else torch.zeros)(frame.shape, dtype=torch.float32, device=dev)
        if with_grad_exposure:
            grad_e = torch.empty((3, 4), dtype=torch.float32, device=dev)
    if exposure is not None:
        exposure = exposure.contiguous()
    with torch.cuda.device(dev):
        nbytes = lib.gsx_photometric_loss_weighted_workspace_bytes(a, b, 1 if with_grad else 0)
        if nbytes == 0:
            raise _ffi.GsxError(_ffi.GSX_ERR_INVALID_ARGUMENT,
                                "gsx_photometric_loss_weighted_workspace_bytes rejected the region %s" % (region,))
        ws = _WORKSPACE.get(dev, nbytes)
        rc = lib.gsx_photometric_loss_weighted(_ptr(frame), stride, _ptr(target), stride, _ptr(weight), int(frame.shape[1]),
                                               _ptr(exposure), a, b, lam, _ptr(out), _ptr(grad), stride, _ptr(grad_e),
                                               _ptr(ws), nbytes, _stream_handle(dev))
    _ffi.check(rc)
    return out, grad, grad_e


class _WeightedPhotometricLossFunction(torch.autograd.Function):
    """Forward: value, dL/dframe and dL/dexposure in the one library call, both saved; backward: grad_output times them."""

    @staticmethod
    def forward(ctx, frame, exposure, target, weight, lam, region):
        want_e = exposure is not None and exposure.requires_grad
        out, grad, grad_e = _call_weighted(frame.detach(), target, lam, region, True, weight,
                                           None if exposure is None else exposure.detach(), want_e)
        ctx.want_e = want_e
        ctx.save_for_backward(grad, *((grad_e,) if want_e else ()))
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms):
        saved = ctx.saved_tensors
        grad_frame = grad_loss * saved[0] if ctx.needs_input_grad[0] else None
        grad_e = grad_loss * saved[1] if ctx.want_e else None
        return grad_frame, grad_e, None, None, None, None


def photometric_loss(frame: torch.Tensor, target: torch.Tensor, lambda_dssim: float = 0.2,
                     region: Optional[Tuple[int, int]] = None, terms: Optional[dict] = None,
                     weight: Optional[torch.Tensor] = None, exposure: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The loss above as a 0-d float32 tensor on the GPU.  ``frame`` and ``target``: contiguous float32 (A, B, 3) tensors on
    the same GPU; ``region=(a, b)`` crops the two leading axes (None: the whole tensor); ``terms``: a dict that receives
    ``l1`` and ``ssim`` as 0-d tensors.  Nothing waits for the device.  When ``frame`` requires grad (and grad mode is on)
    the result carries dL/dframe -- computed in the same call, zero outside the region; ``target`` never gets one.

    ``weight``: a contiguous float32 (A, B) map on the frame's GPU, finite and >= 0 (not checked: that would read it back),
    not requiring grad: both means become weighted means, ``sum m (.) / (3 sum m)`` (gsx_photometric_loss_weighted,
    include/gsx.h).  The weight multiplies the SSIM MAP, not the images: a pixel with weight 0 still reaches the loss through
    the 11 x 11 windows of its neighbours within 5 pixels -- dilate the mask by 5 for a hard cut.  With every weight zero the
    loss and every gradient are exact zeros.  ``exposure``: a float32 (3, 4) tensor on the GPU, an affine colour transform
    ``x' = E[:, :3] x + E[:, 3]`` of the frame inside the region before it meets the target; when it requires grad the result
    carries dL/dexposure too, from the same call.  With either, ``terms`` also receives ``weight_sum``.  With both None every
    call and every bit is as without the two arguments."""
    _check_image("frame", frame)
    if weight is not None:
        _check_weight(weight, frame)
    if exposure is not None:
        _check_exposure(exposure, frame)
    if frame.device.type != "cuda":
        raise ValueError("frame is on %s: the loss runs only as HIP kernels on an AMD GPU (torch device 'cuda'); "
                         "there is no CPU fallback" % frame.device)
    _check_image("target", target, frame.device)
    if tuple(target.shape) != tuple(frame.shape):
        raise ValueError("target has shape %s, the frame %s" % (tuple(target.shape), tuple(frame.shape)))
    if target.requires_grad:
        raise ValueError("target requires grad: photometric_loss differentiates the frame alone (pass target.detach())")
    lam = float(lambda_dssim)
    if not 0.0 <= lam <= 1.0:
        raise ValueError("lambda_dssim = %r is outside [0, 1]" % (lambda_dssim,))
    if region is None:
        region = (int(frame.shape[0]), int(frame.shape[1]))
    else:
        region = (int(region[0]), int(region[1]))
        if not (1 <= region[0] <= frame.shape[0] and 1 <= region[1] <= frame.shape[1]):
            raise ValueError("region %s does not fit the leading axes %s" % (region, tuple(frame.shape[:2])))
    if weight is not None or exposure is not None:
        wants = frame.requires_grad or (exposure is not None and exposure.requires_grad)
        if wants and torch.is_grad_enabled():
            loss, out = _WeightedPhotometricLossFunction.apply(frame, exposure, target, weight, lam, region)
        else:
            out, _, _ = _call_weighted(frame.detach(), target, lam, region, False, weight,
                                       None if exposure is None else exposure.detach())
            loss = out[0]
        if terms is not None:
            terms["l1"], terms["ssim"], terms["weight_sum"] = out[1], out[2], out[3]
        return loss
    if frame.requires_grad and torch.is_grad_enabled():
        loss, out = _PhotometricLossFunction.apply(frame, target, lam, region)
    else:
        out, _ = _call(frame.detach(), target, lam, region, False)
        loss = out[0]
    if terms is not None:
        terms["l1"], terms["ssim"] = out[1], out[2]
    return loss


def depth_loss(depth: torch.Tensor, target: torch.Tensor, region: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """The mean of ``|D - A t|`` over the region's pixels with ``t > 0``, as a 0-d tensor: ``depth`` is the (A, B, 2) image
    of ``GaussianScene.render_image_depth_hip`` -- expected depth ``D`` and coverage ``A`` -- and ``target`` an (A, B) map of
    metric depths ``t`` in view space, 0 (or less, or NaN) where there is no measurement.  The form is linear in both maps
    and divides by nothing: where a pixel is half covered it compares ``D`` with half the target.  ``region=(a, b)`` crops
    the two leading axes (None: the whole image; a frame's last tile row and column are never rendered:
    ``GaussianScene.rendered_region``).  With no valid pixel the result is a zero that is still connected to ``depth``.
    Elementwise torch over one frame: there is no kernel behind it, and nothing waits for the device."""
    if not isinstance(depth, torch.Tensor) or depth.dim() != 3 or depth.shape[2] != 2:
        raise ValueError("depth must be an (A, B, 2) tensor (D, A), got %s" % (
            tuple(depth.shape) if isinstance(depth, torch.Tensor) else type(depth).__name__,))
    if not isinstance(target, torch.Tensor) or tuple(target.shape) != tuple(depth.shape[:2]):
        raise ValueError("target must be an %s tensor of depths, got %s" % (
            tuple(depth.shape[:2]), tuple(target.shape) if isinstance(target, torch.Tensor) else type(target).__name__))
    if target.device != depth.device:
        raise ValueError("target is on %s, depth on %s" % (target.device, depth.device))
    if target.requires_grad:
        raise ValueError("target requires grad: depth_loss differentiates the depth image alone (pass target.detach())")
    if region is not None:
        a, b = int(region[0]), int(region[1])
        if not (1 <= a <= depth.shape[0] and 1 <= b <= depth.shape[1]):
            raise ValueError("region %s does not fit the leading axes %s" % (region, tuple(depth.shape[:2])))
        depth, target = depth[:a, :b], target[:a, :b]
    valid = target > 0
    t = torch.where(valid, target, torch.zeros_like(target)).to(depth.dtype)
    residual = (depth[..., 0] - depth[..., 1] * t).abs() * valid.to(depth.dtype)
    return residual.sum() / valid.sum().clamp(min=1).to(depth.dtype)
