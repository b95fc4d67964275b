"""Scene transform timing (gsx_transform_gaussians) on the trained-like 1M scene at SH degree 3: one JSON line.

    timeout -k 10 600 python tools/bench_transform.py [--steps 20] [--warmup 3] [--batch 5]

bench.py's c3_trainedlike scene (1M Gaussians, seed 0, degree-3 coefficients): 3 + 3 + 4 + 48 = 58 floats per Gaussian are
read and written, 2 x 4 x (10 + 3 K) = 464 bytes per row.  Five contenders take turns inside every step of one session on
the same tensors, medians over the steps, each timed as `batch` back-to-back calls between two HIP events; after every
sample the arrays are put back, so no contender sees another's output:
  call_ms     gsx_transform_gaussians through ctypes with a ready-made GsxTransform: the kernel
  method_ms   Gaussians.transform(R, s, t) end to end: validation, quaternion and SH matrices in float64 on the host, the call
  torch_ms    the same transform composed in torch, in place on the same tensors: a matmul for the means, a product for
              the scales, the Hamilton product from eight slices, and per SH band one torch.einsum("ij,njc->nic") over a
              strided slice of sh (a GEMM on a contiguous copy) with a copy back -- the fastest spelling we found
  torch_bmm_ms  the same with the bands written the obvious way, torch.matmul(M_l, sh[:, band]): n small batched products
              (9 ms per band on an MI355X)
  adam_ms     GaussianAdam.step() over the same arrays and opacity (59 floats, 28 B each): the streaming yardstick
TB/s over the bytes above (adam: 28 x 59 B per row).  `torch_max_abs_diff`: how far the torch composition's arrays are from
the kernel's after one transform (it rounds in another order).
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

ARRAYS = ("points", "scales", "quaternions", "sh")
LR = {"points": 1.6e-6, "scales": 5e-5, "quaternions": 1e-5, "opacity": 5e-4, "sh": 2.5e-5}
S, T = 2.5, (1.5, -0.75, 2.0)


def _timed(fn, batch):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / batch


def _rotation(seed=0):
    import numpy as np

    q = np.random.RandomState(seed).normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def run(steps, warmup, batch, n=1_000_000):
    import torch

    from intro_to_gaussian_splatting_amd import GaussianAdam, Gaussians, _ffi
    from intro_to_gaussian_splatting_amd.synthetic import make_trained_like_scene
    from intro_to_gaussian_splatting_amd.transform import sh_rotation_matrices, similarity

    sc = make_trained_like_scene(n, 1920, 1080, seed=0)
    g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"], device="cuda:0")
    g.sh, g.sh_degree = torch.from_numpy(sc["sh"]).to(g.device).contiguous(), int(sc["sh_degree"])
    dev, degree = g.points.device, g.sh_degree
    sim = similarity(_rotation(), S, T)
    Ms = sh_rotation_matrices(sim.R)

    t = _ffi.GsxTransform()
    t.R[:] = [float(v) for v in sim.R.reshape(-1)]
    t.s = sim.s
    t.t[:] = [float(v) for v in sim.t]
    t.q_R[:] = [float(v) for v in sim.q]
    for field, M in zip(("M1", "M2", "M3"), Ms):
        getattr(t, field)[:] = [float(v) for v in M.reshape(-1)]
    lib, stream = _ffi.load(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call():
        _ffi.check(lib.gsx_transform_gaussians(g.points.data_ptr(), g.scales.data_ptr(), g.quaternions.data_ptr(),
                                               g.sh.data_ptr(), degree, n, ctypes.byref(t), stream))

    f32 = dict(dtype=torch.float32, device=dev)
    Rt, tt = torch.tensor(sim.R.T, **f32), torch.tensor(sim.t, **f32)
    qr = [float(v) for v in sim.q]
    Mt = [torch.tensor(M, **f32) for M in Ms]

    @torch.no_grad()
    def composed(gemm=True):
        g.points.copy_(sim.s * (g.points @ Rt) + tt)
        g.scales.mul_(sim.s)
        aw, ax, ay, az = qr
        bw, bx, by, bz = g.quaternions.unbind(dim=1)
        g.quaternions.copy_(torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                                         aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], dim=1))
        for l, M in enumerate(Mt[:degree], start=1):
            band = g.sh[:, l * l:(l + 1) ** 2, :]
            if gemm:        # einsum folds the band into one GEMM on a contiguous copy
                band.copy_(torch.einsum("ij,njc->nic", M, band))
            else:           # n batched (m, m) x (m, 3) products per band
                band.copy_(torch.matmul(M, band))

    names = ARRAYS + ("opacity",)
    begin = {k: getattr(g, k).detach().clone() for k in names}

    def restore():
        with torch.no_grad():
            for k in names:
                getattr(g, k).copy_(begin[k])

    # how far the composition is from the kernel (another rounding order), after one transform each
    call()
    mine = {k: getattr(g, k).detach().clone() for k in ARRAYS}
    restore()
    composed()
    diff = max(float((getattr(g, k) - mine[k]).abs().max()) for k in ARRAYS)
    restore()
    del mine

    gen = torch.Generator(device=dev).manual_seed(0)
    for k in names:
        p = getattr(g, k).requires_grad_(True)
        p.grad = 1e-3 * torch.randn(p.shape, device=dev, generator=gen)
    contenders = {
        "call_ms": call,
        "method_ms": lambda: g.transform(sim.R, sim.s, sim.t),
        "torch_ms": composed,
        "torch_bmm_ms": lambda: composed(gemm=False),
        "adam_ms": GaussianAdam(g, lr=LR).step,
    }
    samples = {k: [] for k in contenders}
    for step in range(warmup + steps):
        for name, fn in contenders.items():
            ms = _timed(fn, batch)
            if step >= warmup:
                samples[name].append(ms)
            restore()
    med = {k: statistics.median(v) for k, v in samples.items()}
    row_bytes = 2 * 4 * (10 + 3 * (degree + 1) ** 2)
    adam_bytes = 28 * 59
    tbps = lambda nbytes, ms: round(nbytes * n / ms / 1e9, 3)  # noqa: E731
    res = dict(workload="c3_trainedlike", n=n, sh_degree=degree, batch=batch, bytes_per_row=row_bytes,
               torch_max_abs_diff=diff)
    res.update({k: round(v, 4) for k, v in med.items()})
    res.update(call_tbps=tbps(row_bytes, med["call_ms"]), method_tbps=tbps(row_bytes, med["method_ms"]),
               torch_tbps=tbps(row_bytes, med["torch_ms"]), adam_tbps=tbps(adam_bytes, med["adam_ms"]),
               torch_over_call=round(med["torch_ms"] / med["call_ms"], 2),
               torch_bmm_over_call=round(med["torch_bmm_ms"] / med["call_ms"], 2),
               call_over_adam_per_byte=round((med["call_ms"] / row_bytes) / (med["adam_ms"] / adam_bytes), 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000)
    args = ap.parse_args()
    print(json.dumps(dict(metric="transform_ms", results=run(args.steps, args.warmup, args.batch, args.n))))


if __name__ == "__main__":
    main()
