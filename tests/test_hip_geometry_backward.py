"""Geometry gradients on the GPU (gsx_render_backward_geometry through ``geometry_gradients=True``): dL/dpoints,
dL/dscales and dL/dquaternions of the ref_cpu frame, held Gaussian by Gaussian against the reference's own autograd with
its graph cut mended (tests/golden/geomgrad_*.npz, tools/capture_geometry_grad_golden.py) and against the float64
restatement (tests/geometry_backward_restatement.py).

Bounds (test_geometry_backward_host.py): E_REF is the worst per-Gaussian scaled error of the reference's own float32
autograd against the restatement over all fixtures, per output.  The kernel is held to 12 E_REF against the restatement
and to 13 E_REF against the fixtures (the reference's own share added).  What the kernel measured on an MI355X is recorded below.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden

import geometry_backward_restatement as gbr
from test_geometry_backward_host import BOUND_FIXTURE, BOUND_RESTATEMENT, GEOM_SCENES, fixture_inputs
from test_hip_backward import DEV, _golden_scene, _oracle_pre, _scene

pytestmark = pytest.mark.gpu

# Worst error / scale measured on an MI355X over every test of this file that calls _check:
#                 against the restatement                against the reference's autograd
#   points        6.13e-08  (tiny_48x48_n600)            1.03e-07  (tiny_48x48_n600)
#   scales        4.69e-07  (needle_160x160_n110)        1.18e-07  (tiny_48x48_n600)
#   quaternions   3.54e-09  (needle_160x160_n110)        1.06e-08  (tiny_48x48_n600)
# (bounds: 12 E_REF = 2.61e-07, 5.62e-06, 4.55e-08 and 13 E_REF = 2.82e-07, 6.09e-06, 4.93e-08.)
GEOMETRY = ("points", "scales", "quaternions")


def _W(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).to(DEV)


def _all_grads(scene, W, tile=16, geometry=True, only=None, idx=1, **kw):
    """(frame, {name: gradient}) of L = <W, frame> of view `idx` for the five tensors (only: those named)."""
    g = scene.gaussians
    names = GEOMETRY + ("colors", "opacity")
    for name in names:
        t = getattr(g, name)
        t.requires_grad_(only is None or name in only)
        t.grad = None
    frame = scene.render_image_hip(idx, tile_size=tile, geometry_gradients=geometry, **kw)
    (frame * W).sum().backward()
    out = {name: (None if getattr(g, name).grad is None else getattr(g, name).grad.detach().clone()) for name in names}
    for name in names:
        getattr(g, name).requires_grad_(False)
        getattr(g, name).grad = None
    return frame.detach(), out


def _camera(scene, idx=1):
    from oracle import cpu_ref

    im = scene.images[idx]
    c = im.gsx_camera()
    return cpu_ref.Camera(im.world2view.cpu().numpy(), im.full_proj_transform.cpu().numpy(), np.float32(c.tan_fovx),
                          np.float32(c.tan_fovy), np.float32(c.fx), np.float32(c.fy), c.width, c.height)


def _check(scene, sc, frame, W, tile, grads, tag, tiles=None, fixture=None, idx=1):
    """The three geometry gradients against the restatement (12 E_REF per output) and, with `fixture`, against the
    reference's autograd (13 E_REF), per Gaussian.  Returns the restatement's gradients."""
    pre = _oracle_pre(scene, sc, idx)
    w, h = int(sc["width"]), int(sc["height"])
    as_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)  # noqa: E731
    out = gbr.geometry_backward(pre, sc["points"], sc["scales"], sc["quaternions"], _camera(scene, idx), as_np(frame), as_np(W),
                                w, h, tile, tiles=tiles, with_scale=True)
    for k, name in enumerate(GEOMETRY):
        got = as_np(grads[name]).astype(np.float64)
        e = gbr.per_gaussian_error(got, out[k], out[3 + k])
        line = "%s: %s: kernel vs restatement, max error / scale %.4g (bound %.3g)" % (tag, name, e, BOUND_RESTATEMENT[name])
        if fixture is not None:
            ef = gbr.per_gaussian_error(got, fixture["grad_" + name], out[3 + k])
            line += "; vs reference autograd %.4g (bound %.3g)" % (ef, BOUND_FIXTURE[name])
        print(line)
        assert np.isfinite(got).all(), (tag, name)
        assert e <= BOUND_RESTATEMENT[name], (tag, name, e)
        if fixture is not None:
            assert ef <= BOUND_FIXTURE[name], (tag, name, ef)
    return out


@pytest.mark.parametrize("name", GEOM_SCENES)
def test_geometry_gradients_match_reference_and_restatement(tmp_path, name):
    gg, base = fixture_inputs(name)
    scene = _golden_scene(tmp_path, base)
    W = torch.from_numpy(base["W"]).to(DEV)
    tile = int(base["tile"])
    frame, grads = _all_grads(scene, W, tile=tile)
    assert np.array_equal(frame.cpu().numpy(), base["image"]) or np.abs(frame.cpu().numpy() - base["image"]).max() <= 1e-4
    sc = {k: base[k] for k in ("points", "scales", "quaternions", "opacity", "width", "height")}
    out = _check(scene, sc, frame, W, tile, grads, name, fixture=gg)
    # a culled Gaussian, and one on no composited pixel, gets exact zeros in all three
    dead = (np.abs(base["grad_colors"]).sum(1) == 0) & (np.abs(out[0]).sum(1) == 0)
    for key in GEOMETRY:
        assert not grads[key].cpu().numpy()[dead].any(), key
    if int(gg["n_culled"]):
        assert dead.sum() >= int(gg["n_culled"])


def test_colour_and_opacity_gradients_are_the_default_call_s_bits(tmp_path):
    gg = load_golden("grad_trainedlike_128x128_n3000")
    scene = _golden_scene(tmp_path, gg)
    W = torch.from_numpy(gg["W"]).to(DEV)
    f0, plain = _all_grads(scene, W, geometry=False, only=("colors", "opacity"))
    f1, geo = _all_grads(scene, W)
    assert torch.equal(f0, f1)
    assert torch.equal(plain["colors"], geo["colors"]) and torch.equal(plain["opacity"], geo["opacity"])
    assert all(plain[k] is None for k in GEOMETRY) and all(geo[k] is not None and geo[k].abs().max() > 0 for k in GEOMETRY)
    with torch.no_grad():
        assert torch.equal(scene.render_image_hip(1, geometry_gradients=True), f0)


def test_deterministic_and_follows_spatial_order(tmp_path):
    gg = load_golden("grad_trainedlike_128x128_n3000")
    scene = _golden_scene(tmp_path, gg)
    W = torch.from_numpy(gg["W"]).to(DEV)
    _, a = _all_grads(scene, W)
    _, b = _all_grads(scene, W)
    _, c = _all_grads(scene, W, use_hints=False)
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    from intro_to_gaussian_splatting_amd import GaussianScene

    with torch.no_grad():
        ordered = scene.gaussians.spatially_ordered()
    scene2 = GaussianScene(str(tmp_path), ordered)
    _, d = _all_grads(scene2, W)
    oi = ordered.original_index.long()
    for k in a:
        assert torch.equal(d[k], a[k][oi]), k


@pytest.mark.parametrize("tile,w,h", [(16, 96, 80), (32, 96, 96)])
def test_hw3_layout_gradients_equal_wh3(tmp_path, tile, w, h):
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    sc = make_scene(400, w, h, seed=7)
    scene = _scene(tmp_path, sc)
    W = _W((w, h, 3), 5)
    f0, a = _all_grads(scene, W, tile=tile)
    f1, b = _all_grads(scene, W.permute(1, 0, 2).contiguous(), tile=tile, layout="hw3")
    assert torch.equal(f0, f1.permute(1, 0, 2))
    for k in a:
        assert a[k].abs().max() > 0 and torch.equal(a[k], b[k]), k


# the edges file's list (tests/test_hip_backward_edges.py: TILE_SCENES)
TILE_SCENES = {1: (24, 20, 120), 3: (40, 32, 200), 12: (64, 52, 900), 20: (84, 64, 400), 24: (80, 80, 400),
               32: (112, 100, 500), 64: (160, 140, 600)}


@pytest.mark.parametrize("tile", sorted(TILE_SCENES))
def test_tile_sizes_match_restatement(tmp_path, tile):
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    w, h, n = TILE_SCENES[tile]
    sc = make_scene(n, w, h, seed=100 + tile)
    scene = _scene(tmp_path, sc)
    W = _W((w, h, 3), tile)
    frame, grads = _all_grads(scene, W, tile=tile)
    out = _check(scene, sc, frame, W, tile, grads, "tile %d" % tile)
    assert (np.abs(out[0]).sum(1) > 0).sum() >= n // 4


def test_only_points_requiring_grad_returns_only_that_gradient(tmp_path):
    gg = load_golden("grad_small_64x48_n300")
    scene = _golden_scene(tmp_path, gg)
    W = torch.from_numpy(gg["W"]).to(DEV)
    _, full = _all_grads(scene, W)
    g = scene.gaussians
    g.points.requires_grad_(True)
    # without the keyword such a scene renders on the plain path, as it always has
    assert scene.render_image_hip(1).grad_fn is None
    frame = scene.render_image_hip(1, geometry_gradients=True)
    assert frame.grad_fn is not None
    (frame * W).sum().backward()
    assert all(getattr(g, name).grad is None for name in ("scales", "quaternions", "colors", "opacity"))
    assert torch.equal(g.points.grad, full["points"])
    g.points.grad = None
    g.points.requires_grad_(False)


def test_refusals_hold_with_geometry_gradients_and_default_stays_none(tmp_path):
    gg = load_golden("grad_small_64x48_n300")
    scene = _golden_scene(tmp_path, gg)
    g = scene.gaussians
    out = torch.empty((64, 48, 3), device=DEV)
    calls = {
        "semantics": lambda: scene.render_image_hip(1, semantics="ref_cuda", geometry_gradients=True),
        "tile_window": lambda: scene.render_image_hip(1, tile_window=(0, 1, 0, 1), geometry_gradients=True),
        "out": lambda: scene.render_image_hip(1, out=out, geometry_gradients=True),
        "substrips": lambda: scene.render_image_hip(1, substrips=[0, 1, 3], geometry_gradients=True),
        "no_sync": lambda: scene.render_image_hip(1, no_sync=True, geometry_gradients=True),
        "camera_buffer": lambda: scene.render_image_hip(1, camera_buffer=torch.zeros(64, device=DEV), geometry_gradients=True),
    }
    for tensor in (g.points, g.colors):         # a geometry tensor alone, a colour tensor alone
        tensor.requires_grad_(True)
        for what, call in calls.items():
            with pytest.raises(ValueError, match=what):
                call()
        tensor.requires_grad_(False)
    g.colors.requires_grad_(True)
    for what, call in (("capture_frame", lambda: scene.capture_frame(1)),
                       ("render_images", lambda: next(iter(scene.render_images([1]))))):
        with pytest.raises(ValueError, match=what):
            call()
    g.sh = torch.zeros((g.points.shape[0], 1, 3), device=DEV)
    g.sh_degree = 0
    with pytest.raises(ValueError, match="SH"):
        scene.render_image_hip(1, geometry_gradients=True)
    g.sh = None
    for t in (g.points, g.scales, g.quaternions, g.colors, g.opacity):
        t.requires_grad_(True)
    frame = scene.render_image_hip(1)
    gp, gs, gq, gc, go = torch.autograd.grad(frame.sum(), [g.points, g.scales, g.quaternions, g.colors, g.opacity],
                                             allow_unused=True)
    assert gp is None and gs is None and gq is None and gc is not None and go is not None


# Central difference of L(theta) = <W, frame(theta)> along a seeded direction V of one parameter group, all Gaussians at
# once.  Moving a Gaussian also moves its rectangle and can reorder depths: every such flip is a jump of L that the
# difference quotient divides by 2h.  Calibrated on the CPU as the opacity test of tests/test_hip_backward_edges.py was:
# c_oracle.render at C1 (2000 Gaussians, 256x256, W seed 3) against the restatement's gradient, V ~ N(0, 1) seeds 1..3,
# relative error |fd - <grad, V>| / |<grad, V>| per seed:
#   scales       h=1e-1: 1.1 1.0 1.3       1e-2: .31 .27 .21       1e-3: 6.4e-3 3.6e-3 1.9e-2    1e-4: 7.5e-4 2.1e-4 6.9e-4
#                1e-5: 5.3e-4 1.5e-4 3.1e-4     -> h = 1e-4 (1e-5 is as flat on the CPU but nearer float32's noise), 3 x 7.5e-4
#   quaternions  h=1e-1: .76 3.0 .65       1e-2: 4.0e-2 .12 7.2e-2   1e-3: 4.1e-4 3.1e-3 6.1e-4  1e-4: 8.3e-4 3.5e-3 1.1e-3
#                1e-5: 1.0e-6 1.2e-2 5.5e-3     -> h = 1e-3, 3 x 3.1e-3
#   points       h=1e-1: .93 .48 .79       1e-2: .32 .51 .54       1e-3: 1.4e-2 5.1e-2 9.6e-2   1e-4: 1.1e-3 2.3e-3 .93
#                1e-5: 9.8e-4 3.6e-2 1.5e-2; half decades 3e-4: 3.6e-4 .15 .31, 3e-5: 2.4e-4 2.9e-3 3.1, 3e-6: 3.7e-4 2.4e-2 2.8e-2
#     no h below 2e-2 for all three seeds (<grad, V> is -2740, 1006, -505: random directions cancel, single flips do not),
#     so V is scaled by each Gaussian's view depth, as the plan for this case was:
#                h=1e-3: 4.7e-2 5.0e-2 2.0e-3   1e-4: 4.8e-2 8.7e-2 9.3e-2   1e-5: 7.8e-5 1.0e-3 .93
#                3e-4: 1.2e-2 9.2e-2 3.3e-2     3e-5: 4.4e-4 .29 .31         3e-6: 2.7e-3 7.7e-3 1.9e-2
#     -> h = 3e-6 (the only h below 2e-2 on all seeds; a flip's share grows like 1 / h relative to curvature's, so the
#     smallest h the float32 frames carry is the flattest), 3 x 1.92e-2.  The scales did not need their own-size scaling.
# group -> (h, tolerance, how V is scaled)
FD = {"points": (3e-6, 5.8e-2, "depth"), "scales": (1e-4, 2.3e-3, None), "quaternions": (1e-3, 9.3e-3, None)}


def _fd_direction(group, sc, scene, seed=1):
    n = sc["points"].shape[0]
    V = np.random.default_rng(seed).standard_normal((n, 4 if group == "quaternions" else 3)).astype(np.float32)
    how = FD[group][2]
    if how == "size":
        V = V * sc["scales"]
    elif how == "depth":
        cam = _camera(scene)
        V = V * (np.concatenate([sc["points"], np.ones((n, 1), np.float32)], 1) @ cam.world2view)[:, 2:3]
    return torch.from_numpy(np.ascontiguousarray(V, np.float32)).to(DEV)


@pytest.mark.parametrize("group", GEOMETRY)
def test_geometry_gradient_matches_central_difference(tmp_path, group):
    """(L(theta + hV) - L(theta - hV)) / 2h == <dL/dtheta, V> end to end on the GPU at C1, one parameter group at a
    time, without the restatement; the perturbation actually applied (float32) is used for the inner product."""
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    n, w, h = 2000, 256, 256
    sc = make_scene(n, w, h, seed=0)
    scene = _scene(tmp_path, sc)
    W = _W((w, h, 3), 3)
    _, grads = _all_grads(scene, W)
    fd_h, tol, _ = FD[group]
    V = _fd_direction(group, sc, scene)
    t = getattr(scene.gaussians, group)
    with torch.no_grad():
        t0 = t.clone()
        tp, tm = t0 + fd_h * V, t0 - fd_h * V
        t.copy_(tp)
        Lp = float((scene.render_image_hip(1).double() * W.double()).sum())
        t.copy_(tm)
        Lm = float((scene.render_image_hip(1).double() * W.double()).sum())
        t.copy_(t0)
    fd = (Lp - Lm) / (2 * fd_h)
    dot = float((grads[group].double() * (tp.double() - tm.double())).sum()) / (2 * fd_h)
    print("%s: finite difference %.9g, <grad, V> %.9g, relative %.3g" % (group, fd, dot, abs(fd - dot) / abs(dot)))
    assert abs(fd - dot) <= tol * abs(dot), (fd, dot)


def test_c3_gradients_are_finite_zero_where_culled_and_homogeneous(tmp_path):
    """1M Gaussians at 1080p: all five gradients finite, exact zeros on every row the forward culls, and the frame's
    homogeneity in the colours, sum_k <dL/dc_k, c_k> = <W, F>, on the geometry entry point (it walks the same lists)."""
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    sc = make_scene(1_000_000, 1920, 1080, seed=0, behind_fraction=0.05)       # C3 with rows behind the cull plane
    scene = _scene(tmp_path, sc)
    W = _W((1920, 1080, 3), 5)
    frame, grads = _all_grads(scene, W)
    for k, v in grads.items():
        assert torch.isfinite(v).all(), k
        assert v.abs().max() > 0, k
    cam = _camera(scene)
    z = (np.concatenate([sc["points"], np.ones((sc["points"].shape[0], 1), np.float32)], 1) @ cam.world2view)[:, 2]
    culled = torch.from_numpy(z < np.float32(0.19)).to(DEV)       # safely behind the z >= 0.2 plane
    print("C3: %d rows behind the cull plane" % int(culled.sum()))
    assert int(culled.sum()) >= 10_000
    for k, v in grads.items():
        assert not v[culled].any(), k
    lhs = float((grads["colors"].double() * scene.gaussians.colors.double()).sum())
    rhs = float((W.double() * frame.double()).sum())
    print("C3: sum <grad c, c> = %.10g, <W, F> = %.10g" % (lhs, rhs))
    assert abs(lhs - rhs) <= 1e-5 * abs(rhs), (lhs, rhs)
