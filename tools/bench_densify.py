"""Density control timing (gsx_density_* through DensityControl) on the trained-like 1M scene at SH degree 3: one JSON line.

    timeout -k 10 600 python tools/bench_densify.py [--steps 20] [--warmup 3] [--screen]

bench.py's c3_trainedlike scene (1M Gaussians, seed 0, 1920x1080, degree-3 coefficients) with points, scales, quaternions,
opacity and sh trained and two Adam steps taken: 59 floats per Gaussian x 3 arrays (parameter, exp_avg, exp_avg_sq), plus the
untrained colours.  The statistic is that of real scene.photometric_loss(...).backward() calls; the thresholds are
quantiles of the scene itself (`--prune`, `--densify`: the shares of rows pruned and densified, the latter split above the
median size).  Two contenders per operation take turns inside every step of one session on the same tensors, medians over
the steps, each timed between two HIP events around the whole Python call (the round's includes its one host
synchronisation, its noise draw and its allocations):
  accumulate_ms / torch_accumulate_ms   DensityControl.accumulate() | grad_sum += grad.norm(dim=1) where the row is non-zero
  round_ms / torch_round_ms             DensityControl.densify_and_prune() | the same rules as boolean masks, and per array
                                        mask indexing plus cat (survivors, clones, split children), moments zero-filled
--screen adds a third contender to the first line, taking its turn inside the same steps:
  screen_accumulate_ms                  DensityControl(statistic="screen").accumulate() on the statistic one real
                                        backward with screen_statistics=True left (gsx_density_accumulate_screen: 12 B read
                                        per row, 12 B more read and 12 B written per LISTED row)
Both rounds start from the same container every time (the rewrite is out of place: the sources are re-installed).
Bytes: 4 B read and 4 B written per element of an output row (a new row's moments are not read), 28 B per row for the plan
(statistic, scales, opacity in; action and prefix out and in again); the same model for both contenders.
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

TRAINED = ("points", "scales", "quaternions", "opacity", "sh")
LR = {"points": 1.6e-6, "scales": 5e-5, "quaternions": 1e-5, "opacity": 5e-4, "sh": 2.5e-5}
ARRAYS = ("points", "scales", "quaternions", "opacity", "colors", "sh")


def _timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _rotation(q):
    import torch

    nrm = q.norm(dim=1, keepdim=True)
    w, x, y, z = torch.where(nrm > 0, q / nrm, torch.tensor([1.0, 0.0, 0.0, 0.0], device=q.device)).unbind(dim=1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def torch_round(g, opt, grad_sum, seen, knobs, generator):
    """The round composed in torch: ({name: tensor}, {key: {name: tensor}}, n_out).  New rows are appended."""
    import torch

    n = len(g)
    smax = g.scales.detach().amax(dim=1)
    prune = (g.opacity.detach().reshape(-1) < knobs["prune_logit"]) | (smax > knobs["prune_scale"])
    hot = (seen > 0) & (grad_sum / seen.clamp(min=1).float() >= knobs["grad_threshold"])
    split = ~prune & hot & (smax > knobs["dense_scale"])
    clone = ~prune & hot & ~(smax > knobs["dense_scale"])
    stay = ~prune & ~split
    noise = torch.randn((n, 2, 3), generator=generator, device=smax.device)
    out = {}
    for name in ARRAYS:
        a = getattr(g, name)
        if a is None:
            continue
        a = a.detach()
        kids = a[split]
        if name == "points":
            d = g.scales.detach()[split][:, None, :] * noise[split]
            kids = kids[:, None, :] + torch.einsum("mkj,mcj->mck", _rotation(g.quaternions.detach()[split]), d)
        elif name == "scales":
            kids = (kids / knobs["split_shrink"])[:, None, :].expand(-1, 2, -1)
        else:
            kids = kids[:, None].expand(-1, 2, *a.shape[1:])
        out[name] = torch.cat([a[stay], a[clone], kids.reshape(-1, *a.shape[1:])])
    moments = {}
    for key in ("exp_avg", "exp_avg_sq"):
        moments[key] = {}
        for name in opt.names:
            m = getattr(opt, key)[name]
            fresh = torch.zeros((int(out[name].shape[0]) - int(stay.sum()),) + tuple(m.shape[1:]), device=m.device)
            moments[key][name] = torch.cat([m[stay], fresh])
    return out, moments, int(out["points"].shape[0])


def run(steps, warmup, prune_share, densify_share, n=1_000_000, screen=False):
    import torch

    from intro_to_gaussian_splatting_amd import DensityControl, GaussianAdam, GaussianScene, Gaussians
    from intro_to_gaussian_splatting_amd.synthetic import make_trained_like_scene, write_colmap_text

    sc = make_trained_like_scene(n, 1920, 1080, seed=0)
    with tempfile.TemporaryDirectory() as tmp:
        write_colmap_text(tmp, sc)
        g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"],
                                  device="cuda:0")
        g.sh, g.sh_degree = torch.from_numpy(sc["sh"]).to(g.device).contiguous(), int(sc["sh_degree"])
        scene = GaussianScene(tmp, g)
    dev = g.sh.device
    with torch.no_grad():
        gen = torch.Generator(device=dev).manual_seed(0)
        keep = g.sh.clone(), g.opacity.clone()
        g.sh.add_(0.1 * torch.randn(g.sh.shape, device=dev, generator=gen))
        g.opacity.add_(0.3 * torch.randn(g.opacity.shape, device=dev, generator=gen))
        target = scene.render_image_hip(1).clone()
        g.sh.copy_(keep[0])
        g.opacity.copy_(keep[1])
        del keep
    for k in TRAINED:
        getattr(g, k).requires_grad_(True)
    opt = GaussianAdam(g, lr=LR)
    dc = DensityControl(g, optimizer=opt, scene=scene)
    for _ in range(2):
        opt.zero_grad()
        scene.photometric_loss(1, scene.render_image_hip(1, geometry_gradients=True), target).backward()
        dc.accumulate()
        opt.step()
    screen_stat, dcs = None, None
    if screen:      # one more backward, through gsx_render_backward_screen: the statistic the third contender consumes every step
        opt.zero_grad()
        scene.photometric_loss(1, scene.render_image_hip(1, geometry_gradients=True, screen_statistics=True), target).backward()
        screen_stat = scene.screen_statistics
        dcs = DensityControl(g, scene=scene, statistic="screen")
    mean = dc.grad_sum / dc.seen.clamp(min=1).float()
    n_seen = max(1, int((dc.seen > 0).sum()))
    dc.grad_threshold = float(torch.quantile(mean[dc.seen > 0], max(0.0, 1.0 - densify_share * n / n_seen)))
    hot = (dc.seen > 0) & (mean >= dc.grad_threshold)
    dc.dense_scale = float(g.scales.detach().amax(dim=1)[hot].median())      # half of the densified rows split, half clone
    dc.prune_logit = float(torch.quantile(g.opacity.detach().reshape(-1), prune_share))
    dc.prune_scale = float("inf")
    knobs = dict(grad_threshold=dc.grad_threshold, dense_scale=dc.dense_scale, prune_logit=dc.prune_logit,
                 prune_scale=dc.prune_scale, split_shrink=dc.split_shrink)

    start = {name: getattr(g, name) for name in ARRAYS}
    start_m = {key: dict(getattr(opt, key)) for key in ("exp_avg", "exp_avg_sq")}
    stat = dc.grad_sum.clone(), dc.seen.clone()
    grad = g.points.grad
    t_sum, t_seen = torch.zeros_like(dc.grad_sum), torch.zeros_like(dc.seen)

    def restore():
        for name, t in start.items():
            setattr(g, name, t)
        opt.exp_avg, opt.exp_avg_sq = dict(start_m["exp_avg"]), dict(start_m["exp_avg_sq"])
        dc.grad_sum, dc.seen = stat[0].clone(), stat[1].clone()
        g.points.grad = grad

    def torch_accumulate():
        live = (grad != 0).any(dim=1)
        t_sum.add_(torch.where(live, grad.norm(dim=1), torch.zeros_like(t_sum)))
        t_seen.add_(live.to(t_seen.dtype))

    def screen_accumulate():
        scene.screen_statistics = screen_stat       # (accumulate() consumes it)
        dcs.accumulate()

    samples = {k: [] for k in ("accumulate_ms", "torch_accumulate_ms", "round_ms", "torch_round_ms") +
               (("screen_accumulate_ms",) if screen else ())}
    counts, torch_n_out = None, None
    for step in range(warmup + steps):
        restore()
        took = {"accumulate_ms": _timed(dc.accumulate)[0], "torch_accumulate_ms": _timed(torch_accumulate)[0]}
        if screen:
            took["screen_accumulate_ms"] = _timed(screen_accumulate)[0]
        restore()
        took["round_ms"], counts = _timed(lambda: dc.densify_and_prune(generator=torch.Generator(device=dev).manual_seed(step)))
        restore()
        took["torch_round_ms"], composed = _timed(lambda: torch_round(g, opt, stat[0], stat[1], knobs,
                                                                      torch.Generator(device=dev).manual_seed(step)))
        torch_n_out = composed[2]
        del composed
        if step >= warmup:
            for k, v in took.items():
                samples[k].append(v)
    restore()
    med = {k: statistics.median(v) for k, v in samples.items()}
    n_out, new = counts["n_out"], counts["n_cloned"] + 2 * counts["n_split"]
    widths = {name: start[name].numel() // n for name in ARRAYS}
    param_floats = sum(widths.values())
    moment_floats = 2 * sum(widths[name] for name in opt.names)
    round_bytes = 8 * param_floats * n_out + (4 * (n_out - new) + 4 * n_out) * moment_floats + 28 * n + 24 * counts["n_split"]
    acc_bytes = 12 * n + 8 * int((stat[1] > 0).sum())
    rate = lambda nbytes, ms: round(nbytes / ms / 1e6, 1)  # noqa: E731  (GB/s)
    res = dict(workload="c3_trainedlike", n=n, sh_degree=g.sh_degree, floats_per_row=param_floats + moment_floats,
               counts=counts, torch_n_out=torch_n_out, round_bytes=round_bytes, accumulate_bytes=acc_bytes)
    res.update({k: round(v, 4) for k, v in med.items()})
    res.update(round_gbps=rate(round_bytes, med["round_ms"]), torch_round_gbps=rate(round_bytes, med["torch_round_ms"]),
               accumulate_gbps=rate(acc_bytes, med["accumulate_ms"]), torch_accumulate_gbps=rate(acc_bytes, med["torch_accumulate_ms"]),
               torch_round_over_hip=round(med["torch_round_ms"] / med["round_ms"], 2),
               torch_accumulate_over_hip=round(med["torch_accumulate_ms"] / med["accumulate_ms"], 2))
    if screen:
        listed = int((screen_stat[2] > 0).sum())
        sbytes = 12 * n + 24 * listed
        res.update(screen_listed=listed, screen_accumulate_bytes=sbytes, screen_accumulate_gbps=rate(sbytes, med["screen_accumulate_ms"]),
                   screen_accumulate_over_points=round(med["screen_accumulate_ms"] / med["accumulate_ms"], 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prune", type=float, default=0.05)
    ap.add_argument("--densify", type=float, default=0.10)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--screen", action="store_true", help="also time accumulate() under statistic='screen'")
    args = ap.parse_args()
    print(json.dumps(dict(metric="densify_round_ms",
                          results=run(args.steps, args.warmup, args.prune, args.densify, args.n, args.screen))))


if __name__ == "__main__":
    main()
