"""Photo rectification timing (gsx_rectify_photo): one 4000 x 3000 photo to 1600 wide under an OPENCV lens: one JSON line.

    timeout -k 10 600 python tools/bench_rectify.py [--steps 20] [--warmup 3] [--batch 5]

The photo is synthetic (seeded random blocks; no real photograph is part of the tree), the camera an OPENCV one with mild
barrel distortion and an off-centre principal point, the target ``rectified_camera(camera, "std_3dgs", width=1600)``,
``samples`` as ``pick_samples`` picks them (3: 2.5 photo pixels per output pixel).  Contenders take turns inside every step of
one session on the same photo, medians over the steps, each timed as `batch` back-to-back calls between two HIP events:
  call_ms        gsx_rectify_photo through ctypes with ready-made structs: the kernel
  method_ms      capture.rectify(photo, camera, target): the same plus its checks and two allocations
  torch_ms       the same resampling composed in torch from the uint8 photo with the sampling grid READY (it depends on the
                 camera alone): to float, F.grid_sample (bilinear, align_corners) of the photo at the S x S supersampled
                 positions, times the validity mask, F.avg_pool2d of both, the quotient, and the permute to (W', H', 3)
  torch_grid_ms  building that grid and mask (the lens model and the Jacobian on 17 M positions): once per camera
Bytes: what the algorithm has to move -- the photo once (3 W H) and both outputs once (16 W' H') -- over call_ms.
`torch_max_abs_diff`: how far the composition's image is from the kernel's (it rounds in another order).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, batch):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / batch


def run(steps, warmup, batch, src=(4000, 3000), width=1600):
    import numpy as np
    import torch
    import torch.nn.functional as F

    from intro_to_gaussian_splatting_amd import _ffi, capture, colmap

    if not torch.cuda.is_available():
        raise RuntimeError("bench_rectify needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    ws, hs = src
    camera = colmap.Camera(1, "OPENCV", ws, hs, np.array([0.8029 * ws, 0.8041 * ws, 0.5034 * ws, 0.4964 * hs,
                                                         -0.071, 0.012, 0.0007, -0.0011]))
    _, target = capture.rectified_camera(camera, "std_3dgs", width=width)
    S = capture.pick_samples(camera, target)
    tw, th = int(target.width), int(target.height)
    rs = np.random.default_rng(0)
    blocks = rs.integers(0, 256, (hs // 8 + 1, ws // 8 + 1, 3), dtype=np.uint8)
    photo = torch.from_numpy(np.ascontiguousarray(blocks.repeat(8, axis=0).repeat(8, axis=1)[:hs, :ws])).to(dev)
    lens = capture.gsx_lens(camera)
    image = torch.empty((tw, th, 3), dtype=torch.float32, device=dev)
    weight = torch.empty((tw, th), dtype=torch.float32, device=dev)
    lib, stream = _ffi.load(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call():
        _ffi.check(lib.gsx_rectify_photo(photo.data_ptr(), 3 * ws, ctypes.byref(lens), ctypes.byref(target), S,
                                         image.data_ptr(), weight.data_ptr(), stream))

    fxs, fys, cxs, cys, k1, k2, p1, p2 = [float(v) for v in camera.params]

    @torch.no_grad()
    def make_grid():
        off = (torch.arange(S, device=dev, dtype=torch.float32) + 0.5) / S - 0.5
        px = (torch.arange(tw, device=dev, dtype=torch.float32)[:, None] + off[None, :]).reshape(-1)
        py = (torch.arange(th, device=dev, dtype=torch.float32)[:, None] + off[None, :]).reshape(-1)
        x = ((px - float(target.cx)) / float(target.fx))[None, :]
        y = ((py - float(target.cy)) / float(target.fy))[:, None]
        r2 = x * x + y * y
        rho = (k1 + k2 * r2) * r2
        xd = x + x * rho + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y + y * rho + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        g, gp = 1 + rho, k1 + 2 * k2 * r2
        jxx = g + 2 * x * x * gp + 2 * p1 * y + 6 * p2 * x
        jyy = g + 2 * y * y * gp + 6 * p1 * y + 2 * p2 * x
        jxy = 2 * x * y * gp + 2 * p1 * x + 2 * p2 * y
        u, v = fxs * xd + (cxs - 0.5), fys * yd + (cys - 0.5)
        valid = (u >= 0) & (u <= ws - 1) & (v >= 0) & (v <= hs - 1) & (jxx * jyy - jxy * jxy > 0)
        grid = torch.stack([2 * u / (ws - 1) - 1, 2 * v / (hs - 1) - 1], dim=-1)[None]     # (1, H' S, W' S, 2)
        return grid.contiguous(), valid[None, None].to(torch.float32)

    grid, valid = make_grid()

    @torch.no_grad()
    def composed():
        src_f = photo.permute(2, 0, 1)[None].to(torch.float32)
        fine = F.grid_sample(src_f, grid, mode="bilinear", padding_mode="zeros", align_corners=True) * valid
        total, share = F.avg_pool2d(fine, S), F.avg_pool2d(valid, S)
        out = torch.where(share > 0, total / (255.0 * share.clamp_min(1e-12)), torch.zeros_like(total))
        return out[0].permute(2, 1, 0).contiguous(), share[0, 0].t().contiguous()

    call()
    theirs, their_w = composed()
    torch.cuda.synchronize()
    diff = float((theirs - image).abs().max())
    wdiff = float((their_w - weight).abs().max())
    del theirs, their_w

    contenders = {"call_ms": call, "method_ms": lambda: capture.rectify(photo, camera, target), "torch_ms": composed,
                  "torch_grid_ms": make_grid}
    samples = {k: [] for k in contenders}
    for step in range(warmup + steps):
        for name, fn in contenders.items():
            ms = _timed(fn, batch)
            if step >= warmup:
                samples[name].append(ms)
    med = {k: statistics.median(v) for k, v in samples.items()}
    nbytes = 3 * ws * hs + 16 * tw * th
    res = dict(workload="opencv_%dx%d_to_%dx%d" % (ws, hs, tw, th), samples=S, batch=batch, bytes=nbytes,
               torch_max_abs_diff=diff, torch_weight_max_abs_diff=wdiff, valid_share=round(float(weight.mean()), 4))
    res.update({k: round(v, 4) for k, v in med.items()})
    res.update({k.replace("_ms", "_min_ms"): round(min(v), 4) for k, v in samples.items()})
    res.update(call_gbps=round(nbytes / med["call_ms"] / 1e6, 1), torch_over_call=round(med["torch_ms"] / med["call_ms"], 2))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--lib", default=None, help="an experiment build of libgsx.so to time instead (another block shape, ...)")
    args = ap.parse_args()
    if args.lib:
        from intro_to_gaussian_splatting_amd import _ffi

        _ffi.LIB_PATH = os.path.abspath(args.lib)
    print(json.dumps(dict(metric="rectify_ms", results=run(args.steps, args.warmup, args.batch))))


if __name__ == "__main__":
    main()
