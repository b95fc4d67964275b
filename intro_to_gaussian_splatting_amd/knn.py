"""Exact three-nearest-neighbour distances on the GPU: ``nearest3`` (gsx_knn3, include/gsx.h), the call behind
``Gaussians.initialize_scale``.

For every point the distances to its three nearest OTHER points (a duplicate counts, at distance 0; a neighbour that does
not exist is +inf) and the initial scale made of them, in one library call.  The result is a pure float32 function of the
points -- the contract of include/gsx.h, restated in numpy in tests/knn_restatement.py -- whatever the search prunes.  There
is no torch composition behind it and no CPU path.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _ffi

RULES = {"reference": _ffi.GSX_KNN_RULE_REFERENCE, "published": _ffi.GSX_KNN_RULE_PUBLISHED}


def morton_permutation(p: torch.Tensor, bits: int) -> torch.Tensor:
    """int64 (n,): the rows of ``p`` (n, 3) along a 3D Morton (Z-order) curve of ``bits`` per axis over the cloud's bounding
    box, ties by row (``bits`` <= 21: the code is an int64).  Non-finite coordinates go to cell 0.  n > 0."""
    n = p.shape[0]
    lo, hi = p.min(dim=0).values, p.max(dim=0).values
    span = torch.clamp(hi - lo, min=1e-30)
    cells = float(1 << bits)
    q = torch.clamp(((p - lo) / span * cells).to(torch.int64), 0, (1 << bits) - 1)
    q = torch.where(torch.isfinite(p), q, torch.zeros_like(q))         # (NaN / inf means: cell 0)
    code = torch.zeros(n, dtype=torch.int64, device=p.device)
    for b in range(bits):
        for axis in range(3):
            code |= ((q[:, axis] >> b) & 1) << (3 * b + axis)
    return torch.argsort(code, stable=True)


def nearest3(points: torch.Tensor, order: Optional[torch.Tensor] = None, rule: str = "reference",
             stats: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(dist3, scale)`` of ``points`` (n, 3): ``dist3`` (n, 3) the three smallest distances to other rows, ascending;
    ``scale`` (n, 1) under ``rule``: "reference" max(mean(d0, d1, d2), 1e-5), what the reference's ``initialize_scale``
    computes, or "published" sqrt(max(mean(d0^2, d1^2, d2^2), 1e-7)), the published 3DGS initialisation.
    ``order``: an int32 (n,) permutation of the rows, the sequence in which they are blocked for the search (a Morton order:
    ``morton_permutation``); it changes the speed and never a bit of the result.  ``stats`` (a dict): receives
    ``candidates``, the (query, candidate) pairs evaluated -- asking makes the call synchronise."""
    if rule not in RULES:
        raise ValueError("rule = %r is neither 'reference' nor 'published'" % (rule,))
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be a tensor of shape (n, 3)")
    if points.dtype != torch.float32 or not points.is_contiguous():
        raise ValueError("points must be a contiguous float32 tensor")
    if points.device.type != "cuda":
        raise ValueError("points is on %s: nearest3 runs only as HIP kernels on an AMD GPU (torch device 'cuda'); "
                         "there is no CPU fallback" % points.device)
    n = int(points.shape[0])
    dev = points.device
    if order is not None:
        if order.device != dev or order.dtype != torch.int32 or not order.is_contiguous() or tuple(order.shape) != (n,):
            raise ValueError("order must be a contiguous int32 tensor of %d rows on %s" % (n, dev))
    if n and not bool(torch.isfinite(points).all()):
        raise ValueError("points holds a NaN or an infinity: finite coordinates are the precondition of gsx_knn3")
    lib = _ffi.load()
    need = int(lib.gsx_knn3_workspace_bytes(n))
    if need == 0:
        raise ValueError("%d points are more than nearest3 takes (2^30)" % n)
    dist3 = torch.empty((n, 3), dtype=torch.float32, device=dev)
    scale = torch.empty((n, 1), dtype=torch.float32, device=dev)
    if n == 0:                  # (an empty tensor has no address to hand over)
        if stats is not None:
            stats["candidates"] = 0
        return dist3, scale
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)         # (the caching allocator aligns to 512 bytes)
    counted = ctypes.c_int64(0)
    with torch.cuda.device(dev):
        rc = lib.gsx_knn3(points.data_ptr(), n, None if order is None else order.data_ptr(), RULES[rule], dist3.data_ptr(),
                          scale.data_ptr(), ctypes.byref(counted) if stats is not None else None, workspace.data_ptr(),
                          need, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _ffi.check(rc)
    if stats is not None:
        stats["candidates"] = int(counted.value)
    return dist3, scale
