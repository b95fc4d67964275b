"""Backward pass timing (gsx_render_backward) at C2 and C3: one JSON line.

    timeout -k 10 600 python tools/bench_backward.py [--steps 20] [--warmup 3] [--geometry] [--screen] [--camera] [--depth] [--screen-abs] [--std [--antialiased]]
                                                     [--workloads c3] [--sh [--active-degree A]]

Per workload (SURVEY.md section 8(d) generator, seed 0, 1920x1080, tile 16): the forward frame (render_image_hip, no
gradients, median of HIP-event-bracketed frames), the whole backward call (median, host-synchronised as the call is) and
its stages from GSX_FLAG_TIMING (test library: gsx_debug_backward_stage_ms) -- the forward's stages run again, the
compositing backward (+ raw records and emission prefix), the per-Gaussian sums --, and the bytes stored into the
per-pair slots (16 per pair).  --geometry adds the same figures for gsx_render_backward_geometry (key "geometry": the
points, scales and quaternions too; 48 slot bytes per pair, the per-Gaussian chain counted with the sums).  --screen adds
them for gsx_render_backward_screen (key "screen": the same work plus 12 bytes stored per Gaussian, dL/d(NDC mean) and the
radius), its steps taking turns with the geometry entry's so that both see the same clocks ("screen_over_geometry").
--camera takes gsx_render_backward_camera (24 more sums per Gaussian in the chain kernel, one small reduction launch, 32
floats out) in turns with the geometry and the screen entry, three ways ("alternating_camera", "camera_over_screen");
with --sh it takes the SH scene's whole camera-gradient backward (the camera entry, then gsx_sh_backward with the view
direction's share) in turns with the same two calls through the screen entry.  --workloads picks among c2 and c3.
--screen-abs (key "screen_abs") takes gsx_render_backward_screen_abs (the tile kernel's abs instance: two more sums per record
and pixel, 8 more bytes stored per pair, two more sums in the per-Gaussian sum kernel, 8 more bytes stored per Gaussian) in turns with
the screen entry in one session: both medians with their minimum and maximum ("screen_abs_over_screen"), and the
GSX_FLAG_TIMING stages of both, medians of `steps` calls.
--depth (key "depth") takes, in turns in one session: gsx_render_backward_depth for a random dL/dframe and dL/ddepth
("fused"), the screen entry for the same dL/dframe ("screen"), gsx_render_depth alone ("depth_forward"), the frame
("frame") and the two calls the composed path adds, the frame over colours (z, 1, 0) ("frame_z") and its geometry
backward ("backward_z").  "fused_render_side_ms" = frame + depth_forward + fused against "composed_render_side_ms" =
frame + frame_z + screen + backward_z, the medians added; "stages" holds the GSX_FLAG_TIMING stages of the screen and the
fused backward (stage chain again; raw records, prefix and the tile kernel; sums and chain), medians of `steps` calls.

--std (key "std") takes gsx_render_backward_std -- the std_3dgs frame of the same scene (black background, tight
rectangles), its colour-only call ("std_colour_only") and its geometry call ("std_geometry") -- in turns with the ref_cpu
geometry entry ("geometry") and the two forward frames ("frame", "std_frame") in one session: every median with its
minimum and maximum, "std_geometry_over_geometry", and both frames' pair counts (the std lists are the shorter ones).
--antialiased (with --std) adds the anti-aliased frame and its two backward calls to the same turns ("std_aa_frame",
"std_aa_geometry", "std_aa_colour_only"; GSX_FLAG_ANTIALIASED: the same pairs, opacity times rho) and
"std_aa_geometry_over_std_geometry", "std_aa_frame_over_std_frame".

--sh times the differentiable SH scene INSTEAD: the trained-like 1M scene with degree-3 coefficients (bench.py's
c3_trainedlike).  Its backward is gsx_render_backward on this camera's evaluated colours (gsx_sh_to_rgb runs again) and
then gsx_sh_backward: the whole backward, the share of gsx_sh_backward in it, and the kernel alone -- time per launch
over batches of back-to-back launches, bytes = n (24 + 24 K) (+ 12 n with the mean gradient), GB/s -- beside the forward
kernel gsx_sh_to_rgb (n (24 + 12 K) bytes) timed the same way in the same run as the yardstick.  Both kernels alternate
between two copies of the coefficients, so that no launch finds its 192 MB in the 256 MB last-level cache.
--active-degree A (with --sh) sets Gaussians.active_sh_degree: the frame, the backward and the two kernels run on the first
A bands of the degree-3 rows (gsx_sh_to_rgb_active / gsx_sh_backward_active; bytes = n (24 + 12 K_A + 12 K) and
n (24 + 12 K_A)), and "in_turns" holds three rounds of the degree-3 kernels in turns with them, per launch.
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


def _in_turns(calls, steps, warmup):
    """{name: (median ms, [min, max])} of the calls taken in turns, step by step: whatever the clocks do, they do to all."""
    names = list(calls)
    turns = {k: [] for k in names}
    for i in range(len(names) * (warmup + steps)):
        k = names[i % len(names)]
        ms = _median_ms(calls[k], 1, 0)
        if i >= len(names) * warmup:
            turns[k].append(ms)
    return {k: (round(statistics.median(v), 4), [round(min(v), 4), round(max(v), 4)]) for k, v in turns.items()}


def run(name, n, steps, warmup, geometry=False, screen=False, camera=False, depth=False, screen_abs=False, std=False,
        antialiased=False):
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

        def leg(geo, slot_bytes, scr=False):
            call = lambda **kw: scene._render_backward(1, 16, "wh3", frame, W, st["n_instances"], st["n_visible"],  # noqa: E731
                                                       geometry=geo, screen=scr, **kw)
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
        if screen:
            out["screen"] = leg(True, 48, scr=True)
            # the two entries step by step in turn: whatever the clocks do, they do to both
            calls = [lambda scr=scr: scene._render_backward(1, 16, "wh3", frame, W, st["n_instances"], st["n_visible"],
                                                            geometry=True, screen=scr) for scr in (False, True)]
            turns = [[], []]
            for i in range(2 * (warmup + steps)):
                ms = _median_ms(calls[i & 1], 1, 0)
                if i >= 2 * warmup:
                    turns[i & 1].append(ms)
            geo_ms, scr_ms = statistics.median(turns[0]), statistics.median(turns[1])
            out["alternating"] = dict(geometry_ms=round(geo_ms, 4), screen_ms=round(scr_ms, 4),
                                      geometry_min_max=[round(min(turns[0]), 4), round(max(turns[0]), 4)],
                                      screen_min_max=[round(min(turns[1]), 4), round(max(turns[1]), 4)])
            out["screen_over_geometry"] = round(scr_ms / geo_ms, 4)
        if camera:
            back = lambda **kw: scene._render_backward(1, 16, "wh3", frame, W, st["n_instances"], st["n_visible"],  # noqa: E731
                                                       geometry=True, **kw)
            t = _in_turns(dict(geometry=back, screen=lambda: back(screen=True), camera=lambda: back(screen=True, camera=True)),
                          steps, warmup)
            out["alternating_camera"] = {k + "_ms": v[0] for k, v in t.items()}
            out["alternating_camera"].update({k + "_min_max": v[1] for k, v in t.items()})
            out["camera_over_screen"] = round(t["camera"][0] / t["screen"][0], 4)
        if screen_abs:
            back = lambda **kw: scene._render_backward(1, 16, "wh3", frame, W, st["n_instances"], st["n_visible"],  # noqa: E731
                                                       geometry=True, screen=True, **kw)
            calls = dict(screen=back, screen_abs=lambda **kw: back(screen_abs=True, **kw))
            t = _in_turns(calls, steps, warmup)
            d = {k + "_ms": v[0] for k, v in t.items()}
            d.update({k + "_min_max": v[1] for k, v in t.items()})
            d["screen_abs_over_screen"] = round(t["screen_abs"][0] / t["screen"][0], 4)
            d["stages"] = {}
            for key, call in calls.items():
                stages = []
                for _ in range(steps):
                    call(flags=_ffi.GSX_FLAG_TIMING)
                    ms = (ctypes.c_float * 3)()
                    _ffi.check(lib.gsx_debug_backward_stage_ms(ms))
                    stages.append(list(ms))
                d["stages"][key] = [round(statistics.median(s[i] for s in stages), 4) for i in range(3)]
            out["screen_abs"] = d
        if std:
            st_std = {}
            render_std = lambda **kw: scene.render_image_hip(1, semantics="std_3dgs", **kw)  # noqa: E731
            frame_std = render_std(stats=st_std).clone()
            back_std = lambda geo: scene._render_backward(1, 16, "wh3", frame_std, W, st_std["n_instances"],  # noqa: E731
                                                          st_std["n_visible"], geometry=geo, std=((0.0, 0.0, 0.0), False))
            calls = dict(geometry=lambda: scene._render_backward(1, 16, "wh3", frame, W, st["n_instances"],
                                                                 st["n_visible"], geometry=True),
                         std_geometry=lambda: back_std(True), std_colour_only=lambda: back_std(False),
                         frame=lambda: scene.render_image_hip(1), std_frame=render_std)
            if antialiased:
                st_aa = {}
                frame_aa = render_std(stats=st_aa, antialiased=True).clone()
                back_aa = lambda geo: scene._render_backward(1, 16, "wh3", frame_aa, W, st_aa["n_instances"],  # noqa: E731
                                                             st_aa["n_visible"], geometry=geo, std=((0.0, 0.0, 0.0), False, True))
                calls.update(std_aa_geometry=lambda: back_aa(True), std_aa_colour_only=lambda: back_aa(False),
                             std_aa_frame=lambda: render_std(antialiased=True))
            t = _in_turns(calls, steps, warmup)
            d = {k + "_ms": v[0] for k, v in t.items()}
            d.update({k + "_min_max": v[1] for k, v in t.items()})
            d["std_geometry_over_geometry"] = round(t["std_geometry"][0] / t["geometry"][0], 4)
            d["n_instances"] = int(st["n_instances"])
            d["std_n_instances"] = int(st_std["n_instances"])
            if antialiased:
                d["std_aa_geometry_over_std_geometry"] = round(t["std_aa_geometry"][0] / t["std_geometry"][0], 4)
                d["std_aa_frame_over_std_frame"] = round(t["std_aa_frame"][0] / t["std_frame"][0], 4)
                d["std_aa_n_instances"] = int(st_aa["n_instances"])
            out["std"] = d
        if depth:
            back = lambda **kw: scene._render_backward(1, 16, "wh3", frame, W, st["n_instances"], st["n_visible"],  # noqa: E731
                                                       geometry=True, **kw)
            dimg = scene._render_depth(1, 16, "wh3", st["n_instances"], st["n_visible"])
            gen = torch.Generator(device=frame.device).manual_seed(1)
            Wd = torch.randn(dimg.shape, device=frame.device, generator=gen)
            # the composed path: the frame over colours (z, 1, 0) and its geometry backward for dL/dframe = (gD, gA, 0)
            pre = scene.preprocess(1)
            z = torch.zeros(n, dtype=torch.float32, device=frame.device)
            z[scene.last_order.long()] = pre.depths
            del pre
            colors, zcolors = g.colors, torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], 1).contiguous()
            W2 = torch.cat([Wd, torch.zeros_like(Wd[..., :1])], -1).contiguous()

            def over_z(fn):
                def call():
                    g.colors = zcolors
                    try:
                        return fn()
                    finally:
                        g.colors = colors
                return call

            frame_z = over_z(lambda: scene.render_image_hip(1))().clone()
            back_z = over_z(lambda **kw: scene._render_backward(1, 16, "wh3", frame_z, W2, st["n_instances"], st["n_visible"],
                                                                geometry=True))
            fused = lambda **kw: back(screen=True, depth=dimg, grad_depth=Wd, **kw)  # noqa: E731
            t = _in_turns(dict(screen=lambda: back(screen=True), fused=fused,
                               depth_forward=lambda: scene._render_depth(1, 16, "wh3", st["n_instances"], st["n_visible"]),
                               frame=lambda: scene.render_image_hip(1), frame_z=over_z(lambda: scene.render_image_hip(1)),
                               backward_z=back_z), steps, warmup)
            d = {k + "_ms": v[0] for k, v in t.items()}
            d.update({k + "_min_max": v[1] for k, v in t.items()})
            d["fused_over_screen"] = round(t["fused"][0] / t["screen"][0], 4)
            d["fused_render_side_ms"] = round(t["frame"][0] + t["depth_forward"][0] + t["fused"][0], 4)
            d["composed_render_side_ms"] = round(t["frame"][0] + t["frame_z"][0] + t["screen"][0] + t["backward_z"][0], 4)
            d["fused_over_composed"] = round(d["fused_render_side_ms"] / d["composed_render_side_ms"], 4)
            stages = {}
            for key, call in (("screen", lambda **kw: back(screen=True, **kw)), ("fused", fused)):
                rows = []
                for _ in range(steps):
                    call(flags=_ffi.GSX_FLAG_TIMING)
                    ms = (ctypes.c_float * 3)()
                    _ffi.check(lib.gsx_debug_backward_stage_ms(ms))
                    rows.append(list(ms))
                stages[key] = [round(statistics.median(r[i] for r in rows), 4) for i in range(3)]
            d["stages"] = stages
            out["depth"] = d
    return out


def run_sh(steps, warmup, geometry=False, n=1_000_000, batch=10, active=None, camera=False):
    import torch

    from intro_to_gaussian_splatting_amd import GaussianScene, Gaussians, _ffi
    from intro_to_gaussian_splatting_amd.synthetic import make_trained_like_scene, write_colmap_text

    sc = make_trained_like_scene(n, 1920, 1080, seed=0)
    with tempfile.TemporaryDirectory() as tmp:
        write_colmap_text(tmp, sc)
        g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"],
                                  device="cuda:0")
        g.sh, g.sh_degree = torch.from_numpy(sc["sh"]).to(g.device).contiguous(), int(sc["sh_degree"])
        scene = GaussianScene(tmp, g)
    lib = _ffi.load()
    deg, k = g.sh_degree, (g.sh_degree + 1) ** 2
    if active is not None:      # the SH degree schedule: frames, backward and the kernels below on the first `active` bands
        g.active_sh_degree = active
    act = g.active_sh_degree
    ka = (act + 1) ** 2
    with torch.no_grad():
        st = {}
        frame = scene.render_image_hip(1, stats=st).clone()
        fwd_ms = _median_ms(lambda: scene.render_image_hip(1), steps, warmup)
        W = torch.randn(frame.shape, device=frame.device, generator=torch.Generator(device=frame.device).manual_seed(0))

        def whole(geo):
            def call():
                grads = scene._render_backward(1, 16, "wh3", frame, W, st["n_instances"], st["n_visible"], geometry=geo)
                return scene._sh_backward(1, grads[0], with_points=geo)
            return _median_ms(call, steps, warmup)

        # the two kernels alone, on the gradient the frame really produces
        gc = scene._render_backward(1, 16, "wh3", frame, W, st["n_instances"], st["n_visible"])[0]
        pts = g.points.reshape(n, 3).contiguous()
        shs = [g.sh.reshape(n, k, 3).contiguous(), g.sh.reshape(n, k, 3).clone()]
        gsh, gview, cols = torch.empty((n, k, 3), device=pts.device), torch.empty((n, 3), device=pts.device), \
            torch.empty((n, 3), device=pts.device)
        center = (ctypes.c_float * 3)(*scene.images[1].camera_center_host)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731

        def kernel_ms(launch):
            def burst():
                for i in range(batch):
                    _ffi.check(launch(shs[i & 1]))
            return _median_ms(burst, steps, warmup) / batch

        stored = dict(
            bwd=lambda sh: lib.gsx_sh_backward(p(pts), p(sh), deg, n, center, p(gc), p(gsh), None, stream),
            bwd_pts=lambda sh: lib.gsx_sh_backward(p(pts), p(sh), deg, n, center, p(gc), p(gsh), p(gview), stream),
            fwd=lambda sh: lib.gsx_sh_to_rgb(p(pts), p(sh), deg, n, center, p(cols), stream))
        launches = stored if active is None else dict(
            bwd=lambda sh: lib.gsx_sh_backward_active(p(pts), p(sh), deg, act, n, center, p(gc), p(gsh), None, stream),
            bwd_pts=lambda sh: lib.gsx_sh_backward_active(p(pts), p(sh), deg, act, n, center, p(gc), p(gsh), p(gview), stream),
            fwd=lambda sh: lib.gsx_sh_to_rgb_active(p(pts), p(sh), deg, act, n, center, p(cols), stream))
        bwd, bwd_pts, fwd = (kernel_ms(launches[key]) for key in ("bwd", "bwd_pts", "fwd"))
        rate = lambda nbytes, ms: round(nbytes / ms / 1e6, 1)  # noqa: E731  (GB/s)
        b_bwd, b_fwd = n * (24 + 12 * ka + 12 * k), n * (24 + 12 * ka)
        whole_ms = whole(False)
        out = dict(workload="c3_trainedlike", n=n, sh_degree=deg, n_instances=int(st["n_instances"]),
                   forward_frame_ms=round(fwd_ms, 4), backward_ms=round(whole_ms, 4),
                   backward_over_forward=round(whole_ms / fwd_ms, 3),
                   sh_backward_ms=round(bwd, 4), sh_backward_share=round(bwd / whole_ms, 4), sh_backward_bytes=b_bwd,
                   sh_backward_gbps=rate(b_bwd, bwd),
                   sh_backward_with_points_ms=round(bwd_pts, 4), sh_backward_with_points_bytes=b_bwd + 12 * n,
                   sh_backward_with_points_gbps=rate(b_bwd + 12 * n, bwd_pts),
                   sh_to_rgb_ms=round(fwd, 4), sh_to_rgb_bytes=b_fwd, sh_to_rgb_gbps=rate(b_fwd, fwd))
        if active is not None:
            # the degree-`deg` kernels the strided instances stand in for, in turns with them: three rounds each, all kept
            turns = {key: ([], []) for key in ("bwd", "bwd_pts", "fwd")}
            for _ in range(3):
                for key in turns:
                    turns[key][0].append(round(kernel_ms(stored[key]), 4))
                    turns[key][1].append(round(kernel_ms(launches[key]), 4))
            out["active_degree"] = act
            out["in_turns"] = {key: dict(stored_ms=v[0], active_ms=v[1]) for key, v in turns.items()}
        if geometry:
            geo_ms = whole(True)
            out["geometry"] = dict(backward_ms=round(geo_ms, 4), sh_backward_share=round(bwd_pts / geo_ms, 4))
        if camera:
            def through(cam):
                grads = scene._render_backward(1, 16, "wh3", frame, W, st["n_instances"], st["n_visible"], geometry=True,
                                               screen=True, camera=cam)
                return scene._sh_backward(1, grads[0], with_points=True)
            t = _in_turns(dict(screen=lambda: through(False), camera=lambda: through(True)), steps, warmup)
            out["alternating_camera"] = {k + "_ms": v[0] for k, v in t.items()}
            out["alternating_camera"].update({k + "_min_max": v[1] for k, v in t.items()})
            out["camera_over_screen"] = round(t["camera"][0] / t["screen"][0], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--geometry", action="store_true", help="also time gsx_render_backward_geometry")
    ap.add_argument("--screen", action="store_true", help="also time gsx_render_backward_screen, in turns with the geometry entry")
    ap.add_argument("--camera", action="store_true", help="also time gsx_render_backward_camera, in turns with the geometry "
                    "and the screen entry")
    ap.add_argument("--depth", action="store_true", help="also time gsx_render_backward_depth and gsx_render_depth in turns "
                    "with the screen entry and with the composed path's two frames and two backwards")
    ap.add_argument("--screen-abs", action="store_true", help="also time gsx_render_backward_screen_abs, in turns with the "
                    "screen entry")
    ap.add_argument("--std", action="store_true", help="also time gsx_render_backward_std (colour-only and geometry), in turns "
                    "with the ref_cpu geometry entry and the two forward frames")
    ap.add_argument("--antialiased", action="store_true", help="with --std: also the anti-aliased frame and its backward "
                    "(GSX_FLAG_ANTIALIASED), in the same turns")
    ap.add_argument("--workloads", default="c2,c3", help="comma-separated: which of c2, c3 to run (not with --sh)")
    ap.add_argument("--sh", action="store_true", help="the differentiable SH scene instead: trained-like 1M, degree 3")
    ap.add_argument("--active-degree", type=int, default=None, help="with --sh: Gaussians.active_sh_degree (0..3), the "
                    "gsx_sh_*_active entries, and the degree-3 kernels timed in turns with them")
    args = ap.parse_args()
    if args.antialiased and not args.std:
        ap.error("--antialiased goes with --std: the opacity compensation belongs to the std_3dgs frame")
    from intro_to_gaussian_splatting_amd import _ffi

    if args.sh:
        print(json.dumps(dict(metric="sh_backward_ms", results=run_sh(args.steps, args.warmup, args.geometry,
                                                                       active=args.active_degree, camera=args.camera))))
        return
    _ffi.use_test_library()     # gsx_debug_backward_stage_ms
    out = {name: run(name, n, args.steps, args.warmup, args.geometry, args.screen, args.camera, args.depth, args.screen_abs,
                     args.std, args.antialiased)
           for name, n in WORKLOADS.items() if name in args.workloads.split(",")}
    print(json.dumps(dict(metric="backward_ms", results=out)))


if __name__ == "__main__":
    main()
