"""Fixed-budget densification timing (gsx_mcmc_* through MCMCControl) on the trained-like 1M scene at SH degree 3: one JSON line.

    timeout -k 10 600 python tools/bench_mcmc.py [--steps 20] [--warmup 3]

The scene of tools/bench_densify.py: bench.py's c3_trainedlike (1M Gaussians, seed 0, 1920x1080, degree-3 coefficients) with
points, scales, quaternions, opacity and sh trained and two Adam steps taken, so that gradients and moments are those of
real scene.photometric_loss(...).backward() calls.  Two contenders per operation take turns inside every step of one session
on the same tensors, medians over the steps, each timed between two HIP events around the whole Python call (so a call's
noise draw, its allocations and a round's one host synchronisation are inside):
  regularize_ms / torch_regularize_ms   MCMCControl.regularize() | grad.add_ of the same two terms composed in torch
  perturb_ms / torch_perturb_ms         MCMCControl.perturb() | the gate, the rotation and the two products composed in torch
  perturb_kernel_ms                     gsx_mcmc_perturb alone, on a noise array drawn before: 68 B per row; one call between
                                        two events, so the launch latency of a single small kernel is inside
  perturb_stream_ms                     the same call ten times in a row between two events, divided by ten: the streaming
                                        rate (perturb_gbps) is read from this one
  relocate_ms / torch_relocate_ms       MCMCControl.relocate() at `--dead` dead rows and `--growth` growth | multinomial +
                                        bincount + the relocation from a (51, 51) coefficient table + indexing + cat over the
                                        same arrays and moments
  adam_ms                               GaussianAdam.step() in the same session: 28 B per trained element, the streaming
                                        rate perturb_gbps is read against
Every round starts from the same container (the rewrite is out of place: the sources are re-installed); the points are put
back after every perturbation.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRAINED = ("points", "scales", "quaternions", "opacity", "sh")
LR = {"points": 1.6e-6, "scales": 5e-5, "quaternions": 1e-5, "opacity": 5e-4, "sh": 2.5e-5}
ARRAYS = ("points", "scales", "quaternions", "opacity", "colors", "sh")
N_MAX = 51


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

    w, x, y, z = (q / q.norm(dim=1, keepdim=True)).unbind(dim=1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def torch_regularize(g, mc):
    import torch

    n = len(g)
    sg = torch.sigmoid(g.opacity.detach())
    g.opacity.grad.add_((mc.lambda_opacity / n) * sg * (1 - sg))
    g.scales.grad.add_((mc.lambda_scale / (3 * n)) * torch.sign(g.scales.detach()))


def torch_perturb(g, mc, rate, generator):
    import torch

    n = len(g)
    noise = torch.randn((n, 3), generator=generator, device=g.points.device)
    gate = torch.sigmoid(mc.gate_k * ((1 - torch.sigmoid(g.opacity.detach().reshape(-1))) - mc.gate_x0))
    R = _rotation(g.quaternions.detach())
    s = g.scales.detach()
    d = torch.einsum("nkc,nc->nk", R, s * s * torch.einsum("nkc,nk->nc", R, noise))
    d = (rate * gate)[:, None] * d
    g.points.detach().add_(torch.where(torch.isfinite(d).all(dim=1, keepdim=True), d, torch.zeros_like(d)))


def _table(dev):
    """T[N][k] = sum_{i=k+1..N} C(i-1, k) (-1)^k / sqrt(k+1) in float64: D = sum_k T[N][k] x^(k+1)."""
    import torch

    T = [[0.0] * N_MAX for _ in range(N_MAX + 1)]
    for N in range(1, N_MAX + 1):
        for k in range(N):
            T[N][k] = sum(math.comb(i - 1, k) for i in range(k + 1, N + 1)) * (-1) ** k / math.sqrt(k + 1)
    return torch.tensor(T, dtype=torch.float64, device=dev)


def torch_relocate(g, opt, mc, n_out, table, generator):
    """The round composed in torch: ({name: tensor}, {key: {name: tensor}})."""
    import torch

    n = len(g)
    o = g.opacity.detach().reshape(-1)
    p = torch.sigmoid(o.double())
    dead = o <= mc.dead_logit
    dead_rows = dead.nonzero().reshape(-1)
    draws = torch.multinomial(torch.where(dead, torch.zeros_like(p), p), int(dead_rows.numel()) + n_out - n, replacement=True,
                              generator=generator)
    count = torch.bincount(draws, minlength=n)
    source = torch.arange(n_out, device=o.device)
    source[dead_rows] = draws[:dead_rows.numel()]
    source[n:] = draws[dead_rows.numel():]
    hit = (count > 0).nonzero().reshape(-1)
    N = (count[hit] + 1).clamp(max=N_MAX)
    a = p[hit].clamp(max=1 - 2.0 ** -24)
    x = -torch.expm1(torch.log1p(-a) / N)
    powers = x[:, None] ** torch.arange(1, N_MAX + 1, device=o.device, dtype=torch.float64)[None, :]
    coeff = a / (table[N] * powers).sum(dim=1)
    new_p = x.clamp(mc.min_opacity, 1 - 2.0 ** -24)
    opacity = g.opacity.detach().clone()
    opacity.reshape(-1)[hit] = torch.log(new_p / (1 - new_p)).float()
    scales = g.scales.detach().clone()
    scales[hit] = (coeff[:, None] * scales[hit].double()).float()
    moved = (count > 0)[source]
    out = {}
    for name in ARRAYS:
        t = getattr(g, name)
        if t is None:
            continue
        t = opacity if name == "opacity" else (scales if name == "scales" else t.detach())
        out[name] = torch.cat([t[source[:n]], t[source[n:]]])
    moments = {}
    for key in ("exp_avg", "exp_avg_sq"):
        moments[key] = {}
        for name in opt.names:
            m = getattr(opt, key)[name][source]
            m[moved] = 0
            moments[key][name] = m
    return out, moments


def run(steps, warmup, dead_share, growth, n=1_000_000):
    import torch

    from intro_to_gaussian_splatting_amd import GaussianAdam, GaussianScene, Gaussians, MCMCControl, _ffi
    from intro_to_gaussian_splatting_amd._device import _stream_handle
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
    min_opacity = float(torch.sigmoid(torch.quantile(g.opacity.detach().reshape(-1).double(), dead_share)))
    mc = MCMCControl(g, optimizer=opt, scene=scene, cap_max=2 * n, min_opacity=min_opacity, growth=growth)
    for _ in range(2):
        opt.zero_grad()
        scene.photometric_loss(1, scene.render_image_hip(1, geometry_gradients=True), target).backward()
        opt.step()
    n_out = mc.n_out_for(n)
    table = _table(dev)
    rate = mc.noise_lr * mc.point_rate()

    start = {name: getattr(g, name) for name in ARRAYS}
    start_m = {key: dict(getattr(opt, key)) for key in ("exp_avg", "exp_avg_sq")}
    grads = {name: getattr(g, name).grad for name in TRAINED}
    grad_copy = {name: grads[name].clone() for name in ("opacity", "scales")}
    points_copy = g.points.detach().clone()
    noise = torch.randn((n, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(1))

    def restore():
        for name, t in start.items():
            setattr(g, name, t)
        opt.exp_avg, opt.exp_avg_sq = dict(start_m["exp_avg"]), dict(start_m["exp_avg_sq"])
        for name in TRAINED:
            getattr(g, name).grad = grads[name]
        with torch.no_grad():
            for name, t in grad_copy.items():
                grads[name].copy_(t)
            g.points.detach().copy_(points_copy)

    def perturb_kernel():
        _ffi.check(_ffi.load().gsx_mcmc_perturb(g.points.data_ptr(), g.scales.data_ptr(), g.quaternions.data_ptr(),
                                                g.opacity.data_ptr(), noise.data_ptr(), n, rate, mc.gate_k, mc.gate_x0,
                                                _stream_handle(dev)))

    names = ("regularize_ms", "torch_regularize_ms", "perturb_ms", "torch_perturb_ms", "perturb_kernel_ms", "perturb_stream_ms", "relocate_ms",
             "torch_relocate_ms", "adam_ms")
    samples = {k: [] for k in names}
    counts = None
    for step in range(warmup + steps):
        seeded = lambda: torch.Generator(device=dev).manual_seed(step)  # noqa: E731
        restore()
        took = {"regularize_ms": _timed(mc.regularize)[0]}
        restore()
        took["torch_regularize_ms"] = _timed(lambda: torch_regularize(g, mc))[0]
        restore()
        took["perturb_ms"] = _timed(lambda: mc.perturb(generator=seeded()))[0]
        restore()
        took["torch_perturb_ms"] = _timed(lambda: torch_perturb(g, mc, rate, seeded()))[0]
        restore()
        took["perturb_kernel_ms"] = _timed(perturb_kernel)[0]
        restore()
        took["perturb_stream_ms"] = _timed(lambda: [perturb_kernel() for _ in range(10)])[0] / 10.0
        restore()
        took["relocate_ms"], counts = _timed(lambda: mc.relocate(generator=seeded()))
        restore()
        took["torch_relocate_ms"], composed = _timed(lambda: torch_relocate(g, opt, mc, n_out, table, seeded()))
        del composed
        restore()
        state = {key: {k: v.clone() for k, v in getattr(opt, key).items()} for key in ("exp_avg", "exp_avg_sq")}
        params = {name: getattr(g, name).detach().clone() for name in TRAINED}
        took["adam_ms"] = _timed(opt.step)[0]
        with torch.no_grad():                   # the step is undone: every turn sees the same container
            for name in TRAINED:
                getattr(g, name).detach().copy_(params[name])
                opt.exp_avg[name].copy_(state["exp_avg"][name])
                opt.exp_avg_sq[name].copy_(state["exp_avg_sq"][name])
        opt.step_count -= 1
        del state, params
        if step >= warmup:
            for k, v in took.items():
                samples[k].append(v)
    restore()
    med = {k: statistics.median(v) for k, v in samples.items()}
    widths = {name: start[name].numel() // n for name in ARRAYS}
    trained_floats = sum(widths[name] for name in opt.names)
    perturb_bytes, adam_bytes = 68 * n, 28 * trained_floats * n
    reg_bytes = (4 + 8 + 12 + 24) * n
    round_bytes = 8 * (sum(widths.values()) + 2 * trained_floats) * n_out + 20 * n + 12 * n_out
    rate_of = lambda nbytes, ms: round(nbytes / ms / 1e6, 1)  # noqa: E731  (GB/s)
    res = dict(workload="c3_trainedlike", n=n, sh_degree=g.sh_degree, counts=counts, min_opacity=min_opacity, growth=growth,
               perturb_bytes=perturb_bytes, adam_bytes=adam_bytes, regularize_bytes=reg_bytes, relocate_bytes=round_bytes)
    res.update({k: round(v, 4) for k, v in med.items()})
    res.update(perturb_gbps=rate_of(perturb_bytes, med["perturb_stream_ms"]),
               perturb_single_call_gbps=rate_of(perturb_bytes, med["perturb_kernel_ms"]), adam_gbps=rate_of(adam_bytes, med["adam_ms"]),
               regularize_gbps=rate_of(reg_bytes, med["regularize_ms"]), relocate_gbps=rate_of(round_bytes, med["relocate_ms"]),
               torch_regularize_over_hip=round(med["torch_regularize_ms"] / med["regularize_ms"], 2),
               torch_perturb_over_hip=round(med["torch_perturb_ms"] / med["perturb_ms"], 2),
               torch_relocate_over_hip=round(med["torch_relocate_ms"] / med["relocate_ms"], 2),
               per_step_pair_ms=round(med["regularize_ms"] + med["perturb_ms"], 4),
               per_step_pair_over_adam=round((med["regularize_ms"] + med["perturb_ms"]) / med["adam_ms"], 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dead", type=float, default=0.05)
    ap.add_argument("--growth", type=float, default=1.05)
    ap.add_argument("--n", type=int, default=1_000_000)
    args = ap.parse_args()
    print(json.dumps(dict(metric="mcmc_ms", results=run(args.steps, args.warmup, args.dead, args.growth, args.n))))


if __name__ == "__main__":
    main()
