"""Backward pass timing (gsx_render_backward) at C2 and C3: one JSON line.

    timeout -k 10 600 python tools/bench_backward.py [--steps 20] [--warmup 3] [--geometry]

Per workload (SURVEY.md section 8(d) generator, seed 0, 1920x1080, tile 16): the forward frame (render_image_hip, no
gradients, median of HIP-event-bracketed frames), the whole backward call (median, host-synchronised as the call is) and
its stages from GSX_FLAG_TIMING (test library: gsx_debug_backward_stage_ms) -- the forward's stages run again, the
compositing backward (+ raw records and emission prefix), the per-Gaussian sums --, and the bytes stored into the
per-pair slots (16 per pair).  --geometry adds the same figures for gsx_render_backward_geometry (key "geometry": the
points, scales and quaternions too; 48 slot bytes per pair, the per-Gaussian chain counted with the sums).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"c2": 100_000, "c3": 1_000_000}


def _median_ms(fn, steps, warmup):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def run(name, n, steps, warmup, geometry=False):
    import torch

    from intro_to_gaussian_splatting_amd import GaussianScene, Gaussians, _ffi
    from intro_to_gaussian_splatting_amd.synthetic import make_scene, write_colmap_text

    sc = make_scene(n, 1920, 1080, seed=0)
    with tempfile.TemporaryDirectory() as tmp:
        write_colmap_text(tmp, sc)
        g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"],
                                  device="cuda:0")
        scene = GaussianScene(tmp, g)
    with torch.no_grad():
        st = {}
        frame = scene.render_image_hip(1, stats=st).clone()
        fwd_ms = _median_ms(lambda: scene.render_image_hip(1), steps, warmup)
        W = torch.randn(frame.shape, device=frame.device, generator=torch.Generator(device=frame.device).manual_seed(0))
        lib = _ffi.load()

        def leg(geo, slot_bytes):
            call = lambda **kw: scene._render_backward(1, 16, "wh3", frame, W, st["n_instances"], st["n_visible"],  # noqa: E731
                                                       geometry=geo, **kw)
            bwd_ms = _median_ms(call, steps, warmup)
            stages = []         # once per step, under GSX_FLAG_TIMING
            for _ in range(steps):
                call(flags=_ffi.GSX_FLAG_TIMING)
                ms = (ctypes.c_float * 3)()
                _ffi.check(lib.gsx_debug_backward_stage_ms(ms))
                stages.append(list(ms))
            med = [statistics.median(s[i] for s in stages) for i in range(3)]
            return dict(backward_ms=round(bwd_ms, 4), backward_over_forward=round(bwd_ms / fwd_ms, 3),
                        stage_rerun_ms=round(med[0], 4), compositing_backward_ms=round(med[1], 4), sums_ms=round(med[2], 4),
                        slot_bytes=int(st["n_instances"]) * slot_bytes)

        out = dict(workload=name, n=n, n_instances=int(st["n_instances"]), forward_frame_ms=round(fwd_ms, 4), **leg(False, 16))
        if geometry:
            out["geometry"] = leg(True, 48)
            out["geometry_over_colour_only"] = round(out["geometry"]["backward_ms"] / out["backward_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--geometry", action="store_true", help="also time gsx_render_backward_geometry")
    args = ap.parse_args()
    from intro_to_gaussian_splatting_amd import _ffi

    _ffi.use_test_library()     # gsx_debug_backward_stage_ms
    out = {name: run(name, n, args.steps, args.warmup, args.geometry) for name, n in WORKLOADS.items()}
    print(json.dumps(dict(metric="backward_ms", results=out)))


if __name__ == "__main__":
    main()
