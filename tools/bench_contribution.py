"""Contribution pass timing (gsx_render_contribution) on C3 and on the trained-like scene: one JSON line.

    timeout -k 10 600 python tools/bench_contribution.py [--steps 20] [--warmup 3] [--std] [--workloads c3,c3_trainedlike]

Per workload (1920x1080, tile 16; c3: SURVEY.md section 8(d) generator, seed 0, 1M Gaussians; c3_trainedlike: bench.py's
trained-like 1M scene with degree-3 coefficients, whose colours both calls evaluate first): one contribution pass of one
view (``scene._render_contribution``: the library call alone, the view's counts taken from a frame rendered beforehand)
in turns, step by step in one session, with the colour-only backward entry of the same tree on the same view
(``scene._render_backward``: gsx_render_backward, with --std the std_3dgs pair, gsx_render_backward_std) and with the
forward frame -- whatever the clocks do, they do to all three.  Every median comes with its minimum and maximum;
"contribution_over_backward" is the ratio of the two medians.  Both calls run projection, depth order, binning and the
emission prefix again and synchronise once; the contribution pass loads no image and no gradient and stores the same 16
bytes per pair.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_backward import _in_turns  # noqa: E402

WORKLOADS = ("c3", "c3_trainedlike")


def run(name, steps, warmup, std=False, n=1_000_000):
    import torch

    from intro_to_gaussian_splatting_amd import GaussianScene, Gaussians
    from intro_to_gaussian_splatting_amd.synthetic import make_scene, make_trained_like_scene, write_colmap_text

    sc = make_scene(n, 1920, 1080, seed=0) if name == "c3" else make_trained_like_scene(n, 1920, 1080, seed=0)
    with tempfile.TemporaryDirectory() as tmp:
        write_colmap_text(tmp, sc)
        g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"],
                                  device="cuda:0")
        if "sh" in sc:
            g.sh, g.sh_degree = torch.from_numpy(sc["sh"]).to(g.device).contiguous(), int(sc["sh_degree"])
        scene = GaussianScene(tmp, g)
    semantics = "std_3dgs" if std else "ref_cpu"
    kw = dict(semantics=semantics) if std else {}
    with torch.no_grad():
        st = {}
        frame = scene.render_image_hip(1, stats=st, **kw).clone()
        ones = torch.ones_like(frame)
        counts = (st["n_instances"], st["n_visible"])
        contribution = lambda: scene._render_contribution(1, 16, semantics, *counts)  # noqa: E731
        backward = lambda: scene._render_backward(1, 16, "wh3", frame, ones, *counts,  # noqa: E731
                                                  std=((0.0, 0.0, 0.0), False) if std else None)
        # the design requirement, on the scene being timed: weight_sum is the backward's dL/dcolour[:, 0] under dL/dframe = 1
        con, grads = contribution(), backward()
        same_bits = bool(torch.equal(con.weight_sum.view(torch.int32), grads[0][:, 0].contiguous().view(torch.int32)))
        t = _in_turns(dict(contribution=contribution, backward_colour_only=backward,
                           frame=lambda: scene.render_image_hip(1, **kw)), steps, warmup)
        listed = int((con.views > 0).sum())
        out = dict(workload=name, n=n, semantics=semantics, n_instances=int(st["n_instances"]), listed=listed,
                   composited=int((con.pixels > 0).sum()),
                   below_0_01=int(((con.weight_max < 0.01) & (con.views > 0)).sum()),
                   weight_sum_equals_backward_bits=same_bits)
        out.update({k + "_ms": v[0] for k, v in t.items()})
        out.update({k + "_min_max": v[1] for k, v in t.items()})
        out["contribution_over_backward"] = round(t["contribution"][0] / t["backward_colour_only"][0], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--std", action="store_true", help="the std_3dgs pair: the pass and gsx_render_backward_std's colour-only call")
    ap.add_argument("--workloads", default=",".join(WORKLOADS), help="comma-separated: which of c3, c3_trainedlike to run")
    args = ap.parse_args()
    out = {name: run(name, args.steps, args.warmup, args.std) for name in WORKLOADS if name in args.workloads.split(",")}
    print(json.dumps(dict(metric="contribution_ms", results=out)))


if __name__ == "__main__":
    main()
