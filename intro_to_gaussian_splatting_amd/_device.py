"""What every module that calls into libgsx needs from the device side and nothing else: pointers and stream handles as
ctypes values, the float32 / device check of an argument, the GPU requirement, and the caller-owned scratch (the library
never allocates).  A leaf: it imports torch, ctypes and the standard library only, so the loss, the optimiser and the
density control get a stream handle without the scene class and its COLMAP readers."""
from __future__ import annotations

import ctypes
from collections import OrderedDict
from typing import Optional

import torch


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _check_f32(name: str, t: torch.Tensor, device: torch.device) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    if t.device != device:
        raise ValueError("%s is on %s, expected %s" % (name, t.device, device))
    return t if t.is_contiguous() else t.contiguous()


def _stream_handle(device: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_gpu(device: torch.device) -> None:
    if device.type != "cuda":
        raise RuntimeError(
            "the Gaussian tensors are on %s: this renderer runs only as HIP kernels on an AMD GPU "
            "(torch device 'cuda'); there is no CPU fallback" % device)


class _Lru(OrderedDict):
    """A dict that forgets its least recently used entry beyond ``limit`` (device buffers keyed by stream handles or
    by views: a viewer that keeps creating streams, a sweep over hundreds of cameras or a strip plan that moves with
    every rebalance would otherwise grow them for the life of the process)."""

    def __init__(self, limit: int) -> None:
        super().__init__()
        self.limit = int(limit)

    def lookup(self, key):
        val = self.get(key)
        if val is not None:
            self.move_to_end(key)
        return val

    def store(self, key, val):
        self[key] = val
        self.move_to_end(key)
        while len(self) > self.limit:
            self.popitem(last=False)      # (freed on its own stream: torch's allocator orders the reuse behind its last kernel)
        return val


class _Workspace:
    """Caller-owned device scratch for libgsx (the library never allocates)."""

    def __init__(self, limit: int = 8) -> None:
        self.buffers = _Lru(limit)

    def get(self, device: torch.device, nbytes: int) -> torch.Tensor:
        # one buffer per (device, stream): frames in flight on different streams must not share scratch; the
        # buffers of the `limit` most recently used streams are kept (a C3 frame's is ~130 MB)
        key = (device, torch.cuda.current_stream(device).cuda_stream)
        buf = self.buffers.lookup(key)
        if buf is None or buf.numel() < nbytes:
            buf = self.buffers.store(key, torch.empty(nbytes, dtype=torch.uint8, device=device))
        return buf


_WORKSPACE = _Workspace()
