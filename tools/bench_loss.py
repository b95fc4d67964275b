"""Photometric loss timing (gsx_photometric_loss) on the C3 frame at 1920x1080: one JSON line.

    timeout -k 10 600 python tools/bench_loss.py [--steps 20] [--warmup 3] [--batch 5] [--weighted]

The C3 frame (SURVEY.md section 8(d) generator, 1M Gaussians, seed 0, tile 16, wh3) against a target rendered from
perturbed colours and opacities, over the frame's rendered region (1904 x 1072 of 1920 x 1080).  Three contenders take turns
inside every step of one session, medians over the steps, each timed as `batch` back-to-back calls between two HIP events:
  library_grad_ms    gsx_photometric_loss with grad_image: value and dL/dframe
  library_value_ms   the value-only call
  torch_ms           the same loss composed in torch on the same GPU (five depthwise 11 x 11 conv2d, the elementwise
                     chain, autograd's backward): the yardstick -- the parent commit has no loss to compare with
and, through the test library's GSX_LOSS_KERNELS knob (one launch of the three at a time), the kernels one by one, with the
algorithmic bytes of the call -- two images read by each of the two tile kernels, three maps written and read again, the
gradient written -- and the GB/s they amount to (gsx_sh_backward streams at 4.0 TB/s).  `step_share` sets the call beside
the 2.46 ms colour-only backward of the same frame.

``--weighted`` adds a second leg on the same frame, its figures under ``weighted`` in the JSON line: the plain entry again
(the yardstick of this leg, taking turns with the others in the same session), gsx_photometric_loss_weighted with a weight
only, with an exposure only, and with both plus grad_exposure, the same weighted loss composed in torch (the restatement's
``torch_loss`` extended: the exposure as a matmul, the weighted means, autograd down to the frame and the exposure), and
the kernels of the call with both, one launch at a time.  Against the plain entry the weighted call reads 4 more bytes per
pixel where that reads about 60, and sums fifteen more numbers per workgroup.
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

COLOUR_BACKWARD_MS = 2.46       # gsx_render_backward at C3
C1, C2 = 0.01 ** 2, 0.03 ** 2


def _timed(fn, batch):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / batch


def _torch_loss(x, y, lam, kernel):
    import torch.nn.functional as F

    conv = lambda z: F.conv2d(z.permute(2, 0, 1)[None], kernel, padding=5, groups=3)  # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return (1 - lam) * (x - y).abs().mean() + lam * (1 - m.mean())


def _c3_frame_and_target(n):
    """(frame, target, rendered region) of the C3 scene."""
    import torch

    from intro_to_gaussian_splatting_amd import GaussianScene, Gaussians
    from intro_to_gaussian_splatting_amd.synthetic import make_scene, write_colmap_text

    sc = make_scene(n, 1920, 1080, seed=0)
    with tempfile.TemporaryDirectory() as tmp:
        write_colmap_text(tmp, sc)
        g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"],
                                  device="cuda:0")
        scene = GaussianScene(tmp, g)
    with torch.no_grad():
        frame = scene.render_image_hip(1).clone()
        gen = torch.Generator(device=frame.device).manual_seed(0)
        keep = g.colors.clone(), g.opacity.clone()
        g.colors.add_(0.1 * torch.randn(g.colors.shape, device=frame.device, generator=gen)).clamp_(0, 1)
        g.opacity.add_(0.3 * torch.randn(g.opacity.shape, device=frame.device, generator=gen))
        target = scene.render_image_hip(1).clone()
        g.colors.copy_(keep[0])
        g.opacity.copy_(keep[1])
    return frame, target, scene.rendered_region(1)


def _window_kernel(device):
    import torch

    win = torch.exp(-((torch.arange(11, dtype=torch.float64) - 5) ** 2) / (2 * 1.5 ** 2))
    win = (win / win.sum()).float().to(device)
    return (win[:, None] * win[None, :]).expand(3, 1, 11, 11).contiguous()


def run(steps, warmup, batch, n=1_000_000, lam=0.2, scene=None):
    from intro_to_gaussian_splatting_amd.loss import _call

    frame, target, (a, b) = scene if scene is not None else _c3_frame_and_target(n)
    kernel = _window_kernel(frame.device)
    leaf = frame.clone().requires_grad_(True)

    def composed():
        leaf.grad = None
        _torch_loss(leaf[:a, :b], target[:a, :b], lam, kernel).backward()

    contenders = {
        "library_grad_ms": lambda: _call(frame, target, lam, (a, b), True),
        "library_value_ms": lambda: _call(frame, target, lam, (a, b), False),
        "torch_ms": composed,
    }
    # the kernels one by one (test library: GSX_LOSS_KERNELS selects the launches of a call)
    kernels = {"loss_maps_kernel_ms": ("1", True), "loss_reduce_kernel_ms": ("2", True), "loss_grad_kernel_ms": ("4", True),
               "loss_maps_kernel_value_only_ms": ("1", False)}

    def one(name):
        mask, with_grad = kernels[name]
        os.environ["GSX_LOSS_KERNELS"] = mask
        try:
            return _timed(lambda: _call(frame, target, lam, (a, b), with_grad), batch)
        finally:
            del os.environ["GSX_LOSS_KERNELS"]

    samples = {k: [] for k in list(contenders) + list(kernels)}
    for step in range(warmup + steps):
        for name, fn in contenders.items():
            ms = _timed(fn, batch)
            if step >= warmup:
                samples[name].append(ms)
        for name in kernels:
            ms = one(name)
            if step >= warmup:
                samples[name].append(ms)
    med = {k: statistics.median(v) for k, v in samples.items()}
    # the library's figures against the composition's
    out, grad = _call(frame, target, lam, (a, b), True)
    composed()
    ref = _torch_loss(leaf.detach()[:a, :b], target[:a, :b], lam, kernel)
    image_bytes = a * b * 3 * 4
    # maps kernel: 2 images in, 3 maps out; grad kernel: 3 maps + 2 images in, 1 gradient out
    nbytes = {"loss_maps_kernel_ms": 5 * image_bytes, "loss_grad_kernel_ms": 6 * image_bytes,
              "loss_maps_kernel_value_only_ms": 2 * image_bytes}
    res = dict(workload="c3", n=n, region=[a, b], lambda_dssim=lam, batch=batch,
               loss=float(out[0]), l1=float(out[1]), ssim=float(out[2]), torch_loss=float(ref),
               grad_max_abs_difference_over_max=float((grad[:a, :b] - leaf.grad[:a, :b]).abs().max() / leaf.grad.abs().max()))
    res.update({k: round(v, 4) for k, v in med.items()})
    res["torch_over_library"] = round(med["torch_ms"] / med["library_grad_ms"], 2)
    res["algorithmic_bytes"] = 11 * image_bytes
    res["library_grad_gbps"] = round(11 * image_bytes / med["library_grad_ms"] / 1e6, 1)
    for k, v in nbytes.items():
        res[k.replace("_ms", "_gbps")] = round(v / med[k] / 1e6, 1)
    res["step_share"] = dict(colour_backward_ms=COLOUR_BACKWARD_MS,
                             library_adds=round(med["library_grad_ms"] / COLOUR_BACKWARD_MS, 3),
                             torch_adds=round(med["torch_ms"] / COLOUR_BACKWARD_MS, 3))
    return res


def _torch_loss_weighted(x, y, lam, kernel, m, E):
    import torch.nn.functional as F

    if E is not None:
        x = x @ E[:, :3].t() + E[:, 3]
    conv = lambda z: F.conv2d(z.permute(2, 0, 1)[None], kernel, padding=5, groups=3)  # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    smap = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    if m is None:
        return (1 - lam) * (x - y).abs().mean() + lam * (1 - smap.mean())
    n3 = 3 * m.sum()
    return (1 - lam) * (m[..., None] * (x - y).abs()).sum() / n3 + lam * (1 - (m[None, None] * smap).sum() / n3)


def run_weighted(steps, warmup, batch, scene, lam=0.2):
    """The --weighted leg: the plain entry and the weighted entry's three uses in turns, the torch composition, the kernels."""
    import torch

    from intro_to_gaussian_splatting_amd.loss import _call, _call_weighted

    frame, target, (a, b) = scene
    dev = frame.device
    kernel = _window_kernel(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    weight = torch.rand(frame.shape[:2], device=dev, generator=gen)
    weight[200:500, 300:700] = 0.0                        # a masked-out rectangle in a soft weight
    E = (torch.eye(3, 4, device=dev) + 0.05 * torch.randn((3, 4), device=dev, generator=gen)).contiguous()
    leaf = frame.clone().requires_grad_(True)
    leaf_e = E.clone().requires_grad_(True)

    def composed():
        leaf.grad = leaf_e.grad = None
        _torch_loss_weighted(leaf[:a, :b], target[:a, :b], lam, kernel, weight[:a, :b], leaf_e).backward()

    contenders = {
        "plain_ms": lambda: _call(frame, target, lam, (a, b), True),
        "weight_only_ms": lambda: _call_weighted(frame, target, lam, (a, b), True, weight, None),
        "exposure_only_ms": lambda: _call_weighted(frame, target, lam, (a, b), True, None, E),
        "both_with_grad_exposure_ms": lambda: _call_weighted(frame, target, lam, (a, b), True, weight, E, True),
        "both_value_only_ms": lambda: _call_weighted(frame, target, lam, (a, b), False, weight, E),
        "torch_ms": composed,
    }
    kernels = {"wloss_maps_kernel_ms": "1", "wloss_reduce_kernel_ms": "2", "wloss_grad_and_exposure_reduce_ms": "4"}

    def one(name):
        os.environ["GSX_LOSS_KERNELS"] = kernels[name]
        try:
            return _timed(contenders["both_with_grad_exposure_ms"], batch)
        finally:
            del os.environ["GSX_LOSS_KERNELS"]

    samples = {k: [] for k in list(contenders) + list(kernels)}
    for step in range(warmup + steps):
        for name, fn in contenders.items():
            ms = _timed(fn, batch)
            if step >= warmup:
                samples[name].append(ms)
        contenders["both_with_grad_exposure_ms"]()        # leaves the sums and the scale slot the kernels read when run alone
        for name in kernels:
            ms = one(name)
            if step >= warmup:
                samples[name].append(ms)
    med = {k: statistics.median(v) for k, v in samples.items()}
    out, grad, grad_e = _call_weighted(frame, target, lam, (a, b), True, weight, E, True)
    composed()
    ref = _torch_loss_weighted(leaf.detach()[:a, :b], target[:a, :b], lam, kernel, weight[:a, :b], E)
    res = dict(lambda_dssim=lam, loss=float(out[0]), l1=float(out[1]), ssim=float(out[2]), weight_sum=float(out[3]),
               torch_loss=float(ref),
               grad_max_abs_difference_over_max=float((grad[:a, :b] - leaf.grad[:a, :b]).abs().max() / leaf.grad.abs().max()),
               grad_exposure_max_abs_difference_over_max=float((grad_e - leaf_e.grad).abs().max() / leaf_e.grad.abs().max()))
    res.update({k: round(v, 4) for k, v in med.items()})
    for k in ("weight_only_ms", "exposure_only_ms", "both_with_grad_exposure_ms"):
        res[k.replace("_ms", "_over_plain")] = round(med[k] / med["plain_ms"], 3)
    res["torch_over_both"] = round(med["torch_ms"] / med["both_with_grad_exposure_ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--weighted", action="store_true", help="also time gsx_photometric_loss_weighted (module docstring)")
    args = ap.parse_args()
    from intro_to_gaussian_splatting_amd import _ffi

    _ffi.use_test_library()     # the GSX_LOSS_KERNELS knob
    scene = _c3_frame_and_target(1_000_000)
    results = run(args.steps, args.warmup, args.batch, scene=scene)
    if args.weighted:
        results["weighted"] = run_weighted(args.steps, args.warmup, args.batch, scene)
    print(json.dumps(dict(metric="photometric_loss_ms", results=results)))


if __name__ == "__main__":
    main()
