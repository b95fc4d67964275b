"""Backward pass on the GPU (gsx_render_backward through torch.autograd): gradients of the ref_cpu frame with respect to
the colours and the opacity logits, held against the reference's own autograd (tests/golden/grad_*.npz) and the float64
restatement (tests/backward_restatement.py); exact linearity in the colours at C3; determinism; refused options."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

import backward_restatement
from test_backward_host import GRAD_SCENES, REL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _scene(tmp_path, sc, colors=None):
    from intro_to_gaussian_splatting_amd import GaussianScene, Gaussians
    from intro_to_gaussian_splatting_amd.synthetic import write_colmap_text

    write_colmap_text(str(tmp_path), sc)
    g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"], device=DEV)
    if colors is not None:
        g.colors = torch.from_numpy(np.ascontiguousarray(colors, np.float32)).to(DEV)
    return GaussianScene(str(tmp_path), g)


def _golden_scene(tmp_path, gg):
    sc = {k: gg[k] for k in ("points", "colors_0_255", "scales", "quaternions", "opacity", "qvec", "tvec", "fx", "fy",
                             "cx", "cy", "width", "height")}
    return _scene(tmp_path, sc, colors=gg["colors"])


def _grads(scene, W, tile=16, **kw):
    g = scene.gaussians
    g.colors.requires_grad_(True)
    g.opacity.requires_grad_(True)
    g.colors.grad = g.opacity.grad = None
    frame = scene.render_image_hip(1, tile_size=tile, **kw)
    (frame * W).sum().backward()
    return frame.detach(), g.colors.grad.detach().clone(), g.opacity.grad.detach().clone()


def _oracle_pre(scene, sc, idx=1):
    from oracle import c_oracle, cpu_ref

    im = scene.images[idx]
    c = im.gsx_camera()
    cam = cpu_ref.Camera(im.world2view.cpu().numpy(), im.full_proj_transform.cpu().numpy(), np.float32(c.tan_fovx),
                         np.float32(c.tan_fovy), np.float32(c.fx), np.float32(c.fy), c.width, c.height)
    return c_oracle.preprocess(sc["points"], scene.gaussians.colors.detach().cpu().numpy(), sc["scales"],
                               sc["quaternions"], sc["opacity"], cam)


def test_render_image_has_grad_fn_and_backward_fills_grads(tmp_path):
    gg = load_golden("grad_small_64x48_n300")
    scene = _golden_scene(tmp_path, gg)
    scene.gaussians.colors.requires_grad_(True)
    img = scene.render_image(1, tile_size=16)
    assert img.grad_fn is not None and img.device.type == "cpu"
    (img * torch.from_numpy(gg["W"])).sum().backward()
    g = scene.gaussians
    assert g.colors.grad is not None and g.colors.grad.shape == (300, 3) and g.colors.grad.abs().max() > 0
    assert g.opacity.grad is None          # it did not require grad
    g.opacity.requires_grad_(True)
    g.colors.grad = None
    scene.render_image(1, tile_size=16).sum().backward()
    assert g.opacity.grad is not None and g.opacity.grad.shape == (300, 1) and g.opacity.grad.abs().max() > 0


@pytest.mark.parametrize("name", GRAD_SCENES)
def test_hip_gradients_match_reference_autograd(tmp_path, name):
    gg = load_golden("grad_" + name)
    scene = _golden_scene(tmp_path, gg)
    W = torch.from_numpy(gg["W"]).to(DEV)
    frame, gc, go = _grads(scene, W, tile=int(gg["tile"]))
    ref_c, ref_o = gg["grad_colors"].astype(np.float64), gg["grad_opacity"].astype(np.float64)
    gc, go = gc.cpu().numpy().astype(np.float64), go.cpu().numpy().astype(np.float64)
    ec = np.abs(gc - ref_c).max() / np.abs(ref_c).max()
    eo = np.abs(go - ref_o).max() / np.abs(ref_o).max()
    print("%s: max|dgrad| / max|grad|: colours %.3g, opacity logits %.3g" % (name, ec, eo))
    assert ec <= REL and eo <= REL, (ec, eo)


def test_grad_path_frame_equals_no_grad_frame(tmp_path):
    gg = load_golden("grad_trainedlike_128x128_n3000")
    scene = _golden_scene(tmp_path, gg)
    with torch.no_grad():
        plain = scene.render_image_hip(1, tile_size=16).clone()
    scene.gaussians.colors.requires_grad_(True)
    graded = scene.render_image_hip(1, tile_size=16)
    assert graded.grad_fn is not None
    assert torch.equal(plain, graded.detach())


def _c3(tmp_path):
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    sc = make_scene(1_000_000, 1920, 1080, seed=0)
    return sc, _scene(tmp_path, sc)


def test_colour_gradient_is_exact_at_c3(tmp_path):
    """The frame is linear in the colours: L(c + V) - L(c) == <dL/dc, V> (float64 sums of float32 frames)."""
    sc, scene = _c3(tmp_path)
    gen = torch.Generator(device="cpu").manual_seed(5)
    W = torch.randn((1920, 1080, 3), generator=gen).to(DEV)
    V = (0.1 * torch.randn((1_000_000, 3), generator=gen)).to(DEV)
    frame, gc, go = _grads(scene, W)
    g = scene.gaussians
    with torch.no_grad():
        L0 = (frame.double() * W.double()).sum()
        c0 = g.colors.detach().clone()
        g.colors.data.add_(V)
        L1 = (scene.render_image_hip(1, tile_size=16).double() * W.double()).sum()
        g.colors.data.copy_(c0)
    lhs, rhs = float(L1 - L0), float((gc.double() * V.double()).sum())
    print("C3: L(c+V) - L(c) = %.9g, <grad, V> = %.9g" % (lhs, rhs))
    assert abs(lhs - rhs) <= 1e-5 * abs(rhs), (lhs, rhs)


def test_opacity_gradients_match_restatement_at_c1(tmp_path):
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    sc = make_scene(2000, 256, 256, seed=0)
    scene = _scene(tmp_path, sc)
    W = torch.from_numpy(np.random.default_rng(3).standard_normal((256, 256, 3)).astype(np.float32)).to(DEV)
    frame, gc, go = _grads(scene, W)
    pre = _oracle_pre(scene, sc)
    rc, ro = backward_restatement.backward(pre, frame.cpu().numpy(), W.cpu().numpy(), 256, 256, 16, 2000)
    assert np.abs(go.cpu().numpy() - ro).max() <= REL * np.abs(ro).max()
    assert np.abs(gc.cpu().numpy() - rc).max() <= REL * np.abs(rc).max()


def test_opacity_gradients_match_restatement_at_c3_on_eight_tiles(tmp_path):
    sc, scene = _c3(tmp_path)
    rng = np.random.default_rng(11)
    tiles = [(int(x) * 16, int(y) * 16) for x, y in zip(rng.integers(0, 119, 8), rng.integers(0, 66, 8))]
    Wn = np.zeros((1920, 1080, 3), np.float32)
    for x0, y0 in tiles:
        Wn[x0:x0 + 16, y0:y0 + 16] = rng.standard_normal((16, 16, 3))
    W = torch.from_numpy(Wn).to(DEV)
    frame, gc, go = _grads(scene, W)
    pre = _oracle_pre(scene, sc)
    rc, ro = backward_restatement.backward(pre, frame.cpu().numpy(), Wn, 1920, 1080, 16, 1_000_000, tiles=tiles)
    assert np.abs(ro).max() > 0
    assert np.abs(go.cpu().numpy() - ro).max() <= REL * np.abs(ro).max()
    assert np.abs(gc.cpu().numpy() - rc).max() <= REL * np.abs(rc).max()


def test_backward_is_deterministic_and_follows_spatial_order(tmp_path):
    gg = load_golden("grad_trainedlike_128x128_n3000")
    scene = _golden_scene(tmp_path, gg)
    W = torch.from_numpy(gg["W"]).to(DEV)
    _, c1, o1 = _grads(scene, W)
    _, c2, o2 = _grads(scene, W)
    _, c3, o3 = _grads(scene, W, use_hints=False)
    assert torch.equal(c1, c2) and torch.equal(o1, o2)
    assert torch.equal(c1, c3) and torch.equal(o1, o3)
    g = scene.gaussians
    with torch.no_grad():
        g.colors.requires_grad_(False)
        g.opacity.requires_grad_(False)
        ordered = g.spatially_ordered()
    from intro_to_gaussian_splatting_amd import GaussianScene

    scene2 = GaussianScene(str(tmp_path), ordered)
    _, c4, o4 = _grads(scene2, W)
    oi = ordered.original_index.long()
    assert torch.equal(c4, c1[oi]) and torch.equal(o4, o1[oi])


def test_points_scales_quaternions_get_no_gradient(tmp_path):
    gg = load_golden("grad_small_64x48_n300")
    scene = _golden_scene(tmp_path, gg)
    g = scene.gaussians
    for t in (g.points, g.scales, g.quaternions, g.colors, g.opacity):
        t.requires_grad_(True)
    frame = scene.render_image_hip(1, tile_size=16)
    gp, gs, gq, gc, go = torch.autograd.grad((frame * torch.from_numpy(gg["W"]).to(DEV)).sum(),
                                             [g.points, g.scales, g.quaternions, g.colors, g.opacity], allow_unused=True)
    assert gp is None and gs is None and gq is None
    assert gc is not None and go is not None


def test_refused_combinations_raise_and_run_without_grad(tmp_path):
    gg = load_golden("grad_small_64x48_n300")
    scene = _golden_scene(tmp_path, gg)
    g = scene.gaussians
    out = torch.empty((64, 48, 3), device=DEV)
    calls = {
        "semantics": lambda: scene.render_image_hip(1, semantics="ref_cuda"),
        "tile_window": lambda: scene.render_image_hip(1, tile_window=(0, 1, 0, 1)),
        "out": lambda: scene.render_image_hip(1, out=out),
        "substrips": lambda: scene.render_image_hip(1, substrips=[0, 1, 3]),
        "no_sync": lambda: scene.render_image_hip(1, no_sync=True),
        "capture_frame": lambda: scene.capture_frame(1),
        "render_images": lambda: next(iter(scene.render_images([1]))),
    }
    g.colors.requires_grad_(True)
    for what, call in calls.items():
        with pytest.raises(ValueError, match=what):
            call()
    with torch.no_grad():
        for what, call in calls.items():
            call()
        scene.confirm_frames()
    g.colors.requires_grad_(False)
    for what, call in calls.items():
        call()
    scene.confirm_frames()
    # an SH scene
    g.sh = torch.zeros((64 * 0 + g.points.shape[0], 1, 3), device=DEV)
    g.sh_degree = 0
    g.colors.requires_grad_(True)
    with pytest.raises(ValueError, match="SH"):
        scene.render_image_hip(1)
    with torch.no_grad():
        scene.render_image_hip(1)
