"""Scale initialisation timing (gsx_knn3 through knn.nearest3 and Gaussians.initialize_scale): one JSON line per run.

    timeout -k 10 900 python tools/bench_knn.py [--steps 20] [--warmup 3] [--sizes 100000,1000000]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_knn.py --trace      # the kernels' own times, a run of its own

10^5 and then 10^6 points of bench.py's C3 scene (synthetic.make_scene) and of the trained-like scene, seed 0.  Per run,
medians over the steps, each sample between two HIP events around the whole Python call:
  init_ms         Gaussians.initialize_scale(rule="published"): the Morton order in torch, gsx_knn3, the assignment
  morton_ms       knn.morton_permutation(points, 21) and its cast to int32 alone
  knn_ms          knn.nearest3(points, order) with the order at hand: two launches, allocations included
  knn_unordered_ms  the same call with order=None (rows as the generator left them), when --unordered
  torch_ms        the contender on the same GPU and tensor, taking turns with the HIP call in the same loop: brute force
                  composed in torch in chunks -- cdist of a chunk against the cloud, the chunk's own rows set to inf, then
                  topk(3, largest=False).  At 10^6 points one such pass evaluates 10^12 pairs, so it runs every
                  --torch-every-th step there (default: twice in all).
candidates_per_query: (query, candidate) pairs evaluated over n (n - 1 without pruning), from the call's own counter.
max_rel_diff: the contender's distances against the HIP call's (cdist goes through a matrix product: not bit for bit).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def torch_nearest3(p, chunk):
    """(n, 3) distances: brute force in chunks."""
    import torch

    n = p.shape[0]
    out = torch.empty((n, 3), dtype=torch.float32, device=p.device)
    for i0 in range(0, n, chunk):
        i1 = min(i0 + chunk, n)
        d = torch.cdist(p[i0:i1], p)
        r = torch.arange(i1 - i0, device=p.device)
        d[r, r + i0] = float("inf")
        out[i0:i1] = torch.topk(d, 3, dim=1, largest=False, sorted=True).values
    return out


def _points(scene, n):
    from intro_to_gaussian_splatting_amd.synthetic import make_scene, make_trained_like_scene

    make = make_scene if scene == "c3" else make_trained_like_scene
    return make(n, 1920, 1080, seed=0)["points"]


def run(scene, n, steps, warmup, torch_every, unordered, chunk):
    import numpy as np
    import torch

    from intro_to_gaussian_splatting_amd import Gaussians, nearest3
    from intro_to_gaussian_splatting_amd.knn import morton_permutation

    pts = np.ascontiguousarray(_points(scene, n), dtype=np.float32)
    g = Gaussians(torch.from_numpy(pts), torch.zeros((n, 3)), device="cuda:0")
    p = g.points
    order = morton_permutation(p, 21).to(torch.int32).contiguous()
    stats = {}
    dist3, _ = nearest3(p, order=order, stats=stats)
    names = ["init_ms", "morton_ms", "knn_ms"] + (["knn_unordered_ms"] if unordered else [])
    samples = {k: [] for k in names + ["torch_ms"]}
    max_rel = None
    for step in range(warmup + steps):
        took = {"init_ms": _timed(lambda: g.initialize_scale(rule="published"))[0],
                "morton_ms": _timed(lambda: morton_permutation(p, 21).to(torch.int32).contiguous())[0],
                "knn_ms": _timed(lambda: nearest3(p, order=order))[0]}
        if unordered:
            took["knn_unordered_ms"] = _timed(lambda: nearest3(p))[0]
        if torch_every > 0 and (step == 0 or (step >= warmup and (step - warmup) % torch_every == 0)):
            ms, ref = _timed(lambda: torch_nearest3(p, chunk))
            if step >= warmup:
                samples["torch_ms"].append(ms)
            rel = (ref - dist3).abs() / dist3.clamp(min=1e-30)
            max_rel = float(rel[dist3 > 0].max())
            del ref, rel
        if step >= warmup:
            for k in names:
                samples[k].append(took[k])
    res = dict(scene=scene, n=n, steps=steps, warmup=warmup, candidates=stats["candidates"],
               candidates_per_query=round(stats["candidates"] / n, 1), torch_samples=len(samples["torch_ms"]), max_rel_diff=max_rel)
    res.update({k: round(statistics.median(v), 4) for k, v in samples.items() if v})
    if samples["torch_ms"]:
        res["torch_over_hip"] = round(res["torch_ms"] / res["knn_ms"], 1)
    return res


def trace(sizes):
    """A few calls of each size, to be run under rocprofv3 --kernel-trace --stats."""
    import numpy as np
    import torch

    from intro_to_gaussian_splatting_amd import nearest3
    from intro_to_gaussian_splatting_amd.knn import morton_permutation

    for scene in ("c3", "trainedlike"):
        for n in sizes:
            p = torch.from_numpy(np.ascontiguousarray(_points(scene, n), dtype=np.float32)).to("cuda:0")
            order = morton_permutation(p, 21).to(torch.int32).contiguous()
            for _ in range(5):
                nearest3(p, order=order)
            torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--scenes", default="c3,trainedlike")
    ap.add_argument("--torch-every", type=int, default=-1, help="the contender runs every N-th step (0: never; default: every "
                    "step up to 10^5 points, every tenth above)")
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--unordered", action="store_true")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    if args.trace:
        trace(sizes)
        return
    for n in sizes:
        for scene in args.scenes.split(","):
            every = args.torch_every if args.torch_every >= 0 else (1 if n <= 100_000 else 10)
            print(json.dumps(dict(metric="knn_ms", results=run(scene, n, args.steps, args.warmup, every, args.unordered, args.chunk))),
                  flush=True)


if __name__ == "__main__":
    main()
