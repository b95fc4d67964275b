"""Optimiser step timing (gsx_adam_step through GaussianAdam) on the trained-like 1M scene at SH degree 3: one JSON line.

    timeout -k 10 600 python tools/bench_adam.py [--steps 20] [--warmup 3] [--batch 5]

bench.py's c3_trainedlike scene (1M Gaussians, seed 0, 1920x1080, degree-3 coefficients) with points, scales, quaternions,
opacity and sh trained: 3 + 3 + 4 + 1 + 48 = 59 floats per Gaussian.  The gradients are those of ONE real
scene.photometric_loss(...).backward() on a frame rendered with geometry_gradients=True, against a target rendered from
perturbed coefficients and opacities.  Four contenders take turns inside every step of one session on the same tensors,
medians over the steps, each timed as `batch` back-to-back steps between two HIP events:
  dense_ms          GaussianAdam.step(), scales in log space
  skip_ms           the same with skip_zero_rows (GSX_ADAM_SKIP_ZERO_ROWS); `rows_skipped` is the share of Gaussians whose
                    59 gradient entries are all zero
  torch_foreach_ms  torch.optim.Adam(foreach=True) on the same tensors
  torch_fused_ms    torch.optim.Adam(fused=True)
GB/s: 28 B per element of an updated row (gradient read; parameter and two moments read and written) plus 4 B per element
of a skipped one (its gradient is read).  `step_share` sets the step beside the 5.19 ms SH backward it follows
(DESIGN.md section 8b); gsx_sh_backward streams at 3.9 - 4.05 TB/s.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SH_BACKWARD_MS = 5.19           # the SH scene's backward at c3_trainedlike
TRAINED = ("points", "scales", "quaternions", "opacity", "sh")
LR = {"points": 1.6e-6, "scales": 5e-5, "quaternions": 1e-5, "opacity": 5e-4, "sh": 2.5e-5}


def _timed(fn, batch):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / batch


def run(steps, warmup, batch, n=1_000_000):
    import torch

    from intro_to_gaussian_splatting_amd import GaussianAdam, GaussianScene, Gaussians
    from intro_to_gaussian_splatting_amd.synthetic import make_trained_like_scene, write_colmap_text

    sc = make_trained_like_scene(n, 1920, 1080, seed=0)
    with tempfile.TemporaryDirectory() as tmp:
        write_colmap_text(tmp, sc)
        g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"],
                                  device="cuda:0")
        g.sh, g.sh_degree = torch.from_numpy(sc["sh"]).to(g.device).contiguous(), int(sc["sh_degree"])
        scene = GaussianScene(tmp, g)
    with torch.no_grad():
        gen = torch.Generator(device=g.sh.device).manual_seed(0)
        keep = g.sh.clone(), g.opacity.clone()
        g.sh.add_(0.1 * torch.randn(g.sh.shape, device=g.sh.device, generator=gen))
        g.opacity.add_(0.3 * torch.randn(g.opacity.shape, device=g.sh.device, generator=gen))
        target = scene.render_image_hip(1).clone()
        g.sh.copy_(keep[0])
        g.opacity.copy_(keep[1])
        del keep
    for k in TRAINED:
        getattr(g, k).requires_grad_(True)
    loss = scene.photometric_loss(1, scene.render_image_hip(1, geometry_gradients=True), target)
    loss.backward()
    live = torch.zeros(n, dtype=torch.bool, device=g.sh.device)
    for k in TRAINED:
        live |= (getattr(g, k).grad.reshape(n, -1) != 0).any(dim=1)
    skipped = n - int(live.sum())
    width = sum(getattr(g, k).numel() // n for k in TRAINED)

    params = [getattr(g, k) for k in TRAINED]
    groups = lambda: [dict(params=[getattr(g, k)], lr=LR[k]) for k in TRAINED]  # noqa: E731
    contenders = {
        "dense_ms": GaussianAdam(g, lr=LR).step,
        "skip_ms": GaussianAdam(g, lr=LR, skip_zero_rows=True).step,
        "torch_foreach_ms": torch.optim.Adam(groups(), foreach=True).step,
        "torch_fused_ms": torch.optim.Adam(groups(), fused=True).step,
    }
    samples = {k: [] for k in contenders}
    begin = [p.detach().clone() for p in params]
    for step in range(warmup + steps):
        for name, fn in contenders.items():
            ms = _timed(fn, batch)
            if step >= warmup:
                samples[name].append(ms)
            assert all(bool(torch.isfinite(p).all()) for p in params), name
            with torch.no_grad():       # every sample starts from the scene: torch's linear steps would walk small scales below zero
                for p, b in zip(params, begin):
                    p.copy_(b)
    med = {k: statistics.median(v) for k, v in samples.items()}
    dense_bytes = 28 * width * n
    skip_bytes = 28 * width * (n - skipped) + 4 * width * skipped
    rate = lambda nbytes, ms: round(nbytes / ms / 1e6, 1)  # noqa: E731  (GB/s)
    res = dict(workload="c3_trainedlike", n=n, sh_degree=g.sh_degree, floats_per_row=width, batch=batch, loss=float(loss),
               rows_skipped=round(skipped / n, 4), dense_bytes=dense_bytes, skip_bytes=skip_bytes)
    res.update({k: round(v, 4) for k, v in med.items()})
    res.update(dense_gbps=rate(dense_bytes, med["dense_ms"]), skip_gbps=rate(skip_bytes, med["skip_ms"]),
               torch_foreach_gbps=rate(dense_bytes, med["torch_foreach_ms"]), torch_fused_gbps=rate(dense_bytes, med["torch_fused_ms"]),
               skip_over_dense=round(med["skip_ms"] / med["dense_ms"], 3),
               torch_fused_over_dense=round(med["torch_fused_ms"] / med["dense_ms"], 2),
               torch_foreach_over_dense=round(med["torch_foreach_ms"] / med["dense_ms"], 2),
               step_share=dict(sh_backward_ms=SH_BACKWARD_MS, dense_adds=round(med["dense_ms"] / SH_BACKWARD_MS, 3),
                               skip_adds=round(med["skip_ms"] / SH_BACKWARD_MS, 3)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000)
    args = ap.parse_args()
    print(json.dumps(dict(metric="adam_step_ms", results=run(args.steps, args.warmup, args.batch, args.n))))


if __name__ == "__main__":
    main()
