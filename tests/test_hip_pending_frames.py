"""Several differentiable frames pending at once, and a backward whose scene changed under it, on the GPU.

The backward of a frame recomputes projection, depth order and binning from the LIVE scene and trusts only the forward's
counts (gaussian_scene._RenderImageFunction), so it owes nothing to the order forward -> backward -> next forward that every
other gradient test keeps.  Here two or three frames are pending before the first backward runs: other views, other tile
sizes, another scene on the same workspace, the depth function beside the plain one, pose gradients, the screen statistic,
the loss.  The scenes: grad_small_64x48_n300 with two more poses (views 2 and 3, orbit_poses(2, step_deg=STEP_DEG): 5 degrees
to either side of view 1), and the same with SH coefficients built as test_hip_sh_backward._sh_scene builds them.

"Alone" is forward then backward of ONE view with nothing else pending.  Each view's alone gradient is held to the float64
restatements at the bounds of the suites they come from (test_hip_geometry_backward._check, test_hip_backward_edges._check,
test_hip_depth._check, test_hip_camera_gradient._check, sh_backward_restatement at test_sh_backward_host.BOUND).  Every
comparison of a pending-frames result with an alone result is torch.equal.  A sum over two views is a two-term float32
addition, which is commutative: autograd's accumulation order cannot matter.

STEP_DEG was chosen on the CPU (c_oracle.render + backward_restatement on the three poses): at 2 .. 30 degrees every view
has 223 .. 230 Gaussians with a non-zero colour gradient and every pair of frames differs in all 48 x 32 rendered pixels;
10 leaves the culled sets of the three views different.  Both conditions are asserted on the GPU's own frames below.

Worst error / scale of the alone gradients on an MI355X, over views 1, 2 and 3 (test_alone_*):
    geometry entry     points 1.157e-08 (bound 2.61e-07)   scales 2.313e-08 (5.62e-06)   quaternions 3.005e-09 (4.55e-08)
                       (all three: the SH scene with every band active, view 3)
    colour, opacity    colours 5.010e-07 (8e-06; view 2)   opacity logits 2.240e-07 (8e-06; SH scene, active degree 1, view 2)
    depth entry        points 5.479e-09 (1.84e-07; view 2)   scales 2.555e-09 (4.33e-07; view 1)
                       quaternions 2.766e-10 (5.07e-08; view 3)   colors 5.012e-07 (2.33e-06; view 2)
                       opacity 5.342e-08 (5.83e-07; view 2)
    camera entry       world2view 2.800e-11 (3.49e-08; view 2)   full_proj 3.444e-10 (6.64e-08; view 2)
    gsx_sh_backward    sh 6.017e-07 (8.31e-06; every band active, view 1)
                       points through the view direction 2.169e-07 (4.61e-06; active degree 1, view 2)
The whole file takes under five seconds.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden

import sh_backward_restatement as shr
import test_hip_backward_edges as colour_suite
import test_hip_camera_gradient as camera_suite
import test_hip_depth as depth_suite
import test_hip_geometry_backward as geometry_suite
from test_hip_backward import DEV, _golden_scene
from test_hip_geometry_backward import GEOMETRY, _all_grads
from test_hip_sh_backward import _grads as _sh_grads
from test_hip_sh_backward import _rgb_copy, _sh_for
from test_sh_backward_host import BOUND as SH_BOUND

pytestmark = pytest.mark.gpu

STEP_DEG = 10.0
VIEWS = (1, 2, 3)
TILE = 16
FIVE = GEOMETRY + ("colors", "opacity")
FIVE_SH = GEOMETRY + ("opacity", "sh")
SH_DEGREE = 3
MIN_LIVE, MIN_DIFFERENT = 50, 0.10


def _base():
    gg = load_golden("grad_small_64x48_n300")
    return gg, {k: gg[k] for k in ("points", "colors_0_255", "scales", "quaternions", "opacity", "qvec", "tvec", "fx", "fy",
                                   "cx", "cy", "width", "height")}


def _scene(path, sh=False, active=None):
    """grad_small_64x48_n300 with views 1, 2 and 3; ``sh``: SH coefficients of degree 3 (``active``: the active degree)."""
    from intro_to_gaussian_splatting_amd import GaussianScene, Gaussians
    from intro_to_gaussian_splatting_amd.synthetic import orbit_poses, write_colmap_text

    gg, sc = _base()
    write_colmap_text(str(path), sc, extra_poses=orbit_poses(2, step_deg=STEP_DEG))
    g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"], device=DEV)
    g.colors = torch.from_numpy(np.ascontiguousarray(gg["colors"], np.float32)).to(DEV)
    if sh:
        g.sh = torch.from_numpy(_sh_for(np.asarray(gg["colors"], np.float32), SH_DEGREE, 11)).to(DEV).contiguous()
        g.sh_degree = SH_DEGREE
        if active is not None:
            g.active_sh_degree = active
    scene = GaussianScene(str(path), g)
    assert sorted(scene.images) == list(VIEWS)
    return scene


def _weights(idx, last=3):
    return geometry_suite._W((64, 48, last), 100 * last + idx)


W = {}


def _w(idx, last=3):
    if (idx, last) not in W:
        W[(idx, last)] = _weights(idx, last)
    return W[(idx, last)]


def _names(scene):
    return FIVE_SH if getattr(scene.gaussians, "sh", None) is not None else FIVE


def _arm(scene, names=None):
    g = scene.gaussians
    for name in ("points", "scales", "quaternions", "opacity", "colors", "sh"):
        t = getattr(g, name, None)
        if t is not None:
            t.requires_grad_(name in (names or _names(scene)))
            t.grad = None
    return [getattr(g, name) for name in (names or _names(scene))]


def _collect(scene, names=None):
    g = scene.gaussians
    return {name: (None if getattr(g, name).grad is None else getattr(g, name).grad.detach().clone())
            for name in (names or _names(scene))}


def _alone(scene, idx, **kw):
    """(frame, {name: gradient}) of L = <W_idx, frame of view idx>, nothing else pending."""
    if getattr(scene.gaussians, "sh", None) is not None:
        frame, grads = _sh_grads(scene, _w(idx), FIVE_SH, True, idx=idx)
        return frame, {k: grads[k] for k in FIVE_SH}
    return _all_grads(scene, _w(idx), tile=TILE, idx=idx, **kw)


def _views_show_something_and_differ(scene, frames, colour_grads, tag):
    """No view may pass vacuously: >= 50 Gaussians with a colour gradient per view, any two frames differ in > 10 % of the
    rendered pixels."""
    for idx in VIEWS:
        live = int((colour_grads[idx].reshape(colour_grads[idx].shape[0], -1).abs().sum(1) > 0).sum())
        print("%s: view %d: %d Gaussians with a non-zero colour gradient" % (tag, idx, live))
        assert live >= MIN_LIVE, (tag, idx, live)
    a, b = scene.rendered_region(1, TILE)
    for i, j in ((1, 2), (1, 3), (2, 3)):
        share = float((frames[i][:a, :b] != frames[j][:a, :b]).any(-1).float().mean())
        print("%s: views %d and %d differ in %.1f %% of the rendered pixels" % (tag, i, j, 100 * share))
        assert share > MIN_DIFFERENT, (tag, i, j, share)


_ALONE = {}


def _reference(tmp_path_factory, kind):
    """{view: (frame, gradients)} of a fresh scene of this kind, computed once per session and left unchanged.
    kind: "rgb", or ("sh", active degree)."""
    if kind not in _ALONE:
        path = tmp_path_factory.mktemp("alone")
        scene = _scene(path) if kind == "rgb" else _scene(path, sh=True, active=kind[1])
        _ALONE[kind] = {idx: _alone(scene, idx) for idx in VIEWS}
    return _ALONE[kind]


@pytest.fixture
def alone_rgb(tmp_path_factory):
    return _reference(tmp_path_factory, "rgb")


def _equal(got, want, tag):
    for name in want:
        assert got[name] is not None and want[name].abs().max() > 0, (tag, name)
        assert torch.equal(got[name], want[name]), (tag, name)


def _sum(a, b):
    return {name: a[name] + b[name] for name in a}


# ---- the alone gradients of every view against the float64 restatements
def test_alone_rgb_gradients_of_every_view_meet_the_restatement_bounds(tmp_path, alone_rgb):
    scene = _scene(tmp_path)
    _, sc = _base()
    _views_show_something_and_differ(scene, {i: alone_rgb[i][0] for i in VIEWS}, {i: alone_rgb[i][1]["colors"] for i in VIEWS},
                                     "rgb")
    for idx in VIEWS:
        frame, grads = alone_rgb[idx]
        tag = "alone, view %d" % idx
        geometry_suite._check(scene, sc, frame, _w(idx), TILE, grads, tag, idx=idx)
        colour_suite._check(scene, sc, frame, _w(idx), TILE, grads["colors"], grads["opacity"], tag, idx=idx)


def test_alone_depth_gradients_of_every_view_meet_the_restatement_bounds(tmp_path):
    scene = _scene(tmp_path)
    _, sc = _base()
    for idx in VIEWS:
        frame, depth, grads = depth_suite._depth_grads(scene, _w(idx), _w(idx, 2), tile=TILE, idx=idx)
        depth_suite._check(scene, sc, frame, depth, _w(idx), _w(idx, 2), TILE, grads, "alone depth, view %d" % idx, idx=idx)


def test_alone_camera_gradients_of_every_view_meet_the_restatement_bounds(tmp_path):
    scene = _scene(tmp_path)
    _, sc = _base()
    for idx in VIEWS:
        frame, outs, _ = camera_suite._entry(scene, _w(idx), TILE, screen=False, idx=idx)
        camera_suite._check("alone camera, view %d" % idx, outs[-2], outs[-1],
                            camera_suite._restate(scene, sc, frame, _w(idx), TILE, idx=idx))
        # the leaf's gradient is these two matrices composed (full_proj = world2view @ projection_matrix)
        im = scene.images[idx]
        im.world2view.requires_grad_(True)
        f = scene.render_image_hip(idx, camera_gradients=True)
        (f * _w(idx)).sum().backward()
        assert torch.equal(f.detach(), frame) and torch.equal(im.world2view.grad, outs[-2] + outs[-1] @ im.projection_matrix.t())
        im.world2view.grad = None
        im.world2view.requires_grad_(False)


@pytest.mark.parametrize("active", [SH_DEGREE, 1])
def test_alone_sh_gradients_of_every_view_meet_the_restatement_bounds(tmp_path, tmp_path_factory, active):
    """An SH frame's gradients are the RGB scene's of this view's evaluated colours -- held to the geometry and colour
    restatements -- carried through gsx_sh_backward_active, which is held to sh_backward_restatement at this view's
    camera centre on the active bands; the inactive bands are exact zeros."""
    from intro_to_gaussian_splatting_amd import GaussianScene

    alone = _reference(tmp_path_factory, ("sh", active))
    scene = _scene(tmp_path, sh=True, active=active)
    g = scene.gaussians
    _, sc = _base()
    n, ka = g.points.shape[0], (active + 1) ** 2
    frames, colour_grads = {}, {}
    for idx in VIEWS:
        frame, grads = alone[idx]
        tag = "alone sh (active %d), view %d" % (active, idx)
        with torch.no_grad():
            colors = scene._colors(idx).clone()
        rgb = GaussianScene(str(tmp_path), _rgb_copy(g, colors))
        rgb_frame, rgb_grads = _all_grads(rgb, _w(idx), tile=TILE, idx=idx)
        assert torch.equal(rgb_frame, frame)
        geometry_suite._check(rgb, sc, rgb_frame, _w(idx), TILE, rgb_grads, tag, idx=idx)
        colour_suite._check(rgb, sc, rgb_frame, _w(idx), TILE, rgb_grads["colors"], rgb_grads["opacity"], tag, idx=idx)
        for name in ("opacity", "scales", "quaternions"):
            assert torch.equal(grads[name], rgb_grads[name]), (tag, name)
        gsh, gview = scene._sh_backward(idx, rgb_grads["colors"], with_points=True)
        assert torch.equal(grads["sh"], gsh.view(g.sh.shape)) and torch.equal(grads["points"], rgb_grads["points"] + gview)
        assert gview.abs().max() > 0 and not grads["sh"][:, ka:].any()         # the view direction's share; inactive bands
        centre = np.asarray(scene.images[idx].camera_center_host, np.float64)
        pts, sh = g.points.detach().cpu().numpy(), g.sh.detach().cpu().numpy()[:, :ka]
        gc = rgb_grads["colors"].cpu().numpy()
        pre, mask = shr.forward(pts, sh, active, centre)[:2]
        sure = np.abs(pre) >= shr.NEAR_ZERO
        assert (~sure).mean() <= 0.01 and 0.01 <= (~mask).mean() <= 0.5
        ref_sh, ref_mean, scale_sh, scale_mean = shr.backward(pts, sh, active, centre, gc)
        # (a Gaussian on no composited pixel has dL/dcolour = 0: its scale is 0 and its rows must be exact zeros)
        e_sh = shr.scaled_error(gsh.cpu().numpy().reshape(n, -1, 3)[:, :ka], ref_sh, scale_sh, keep=sure[:, None, :])
        e_mean = shr.scaled_error(gview.cpu().numpy(), ref_mean, scale_mean, keep=sure.all(1)[:, None])
        print("%s: kernel vs restatement, max error / scale: sh %.4g (bound %.3g), points %.4g (bound %.3g)" % (
            tag, e_sh, SH_BOUND["sh"], e_mean, SH_BOUND["points"]))
        assert e_sh <= SH_BOUND["sh"] and e_mean <= SH_BOUND["points"], (tag, e_sh, e_mean)
        frames[idx], colour_grads[idx] = frame, rgb_grads["colors"]
    _views_show_something_and_differ(scene, frames, colour_grads, "sh (active %d)" % active)
    with torch.no_grad():       # the camera centre differs per view: so do the colours
        assert not torch.equal(scene._colors(1), scene._colors(2))


# ---- 1, 2: two views pending
def _two_forwards(scene, **kw):
    f1 = scene.render_image_hip(1, geometry_gradients=True, **kw)
    f2 = scene.render_image_hip(2, geometry_gradients=True, **kw)
    return f1, f2, (f1 * _w(1)).sum(), (f2 * _w(2)).sum()


def _two_views_one_backward(scene, alone):
    leaves = _arm(scene)
    f1, f2, L1, L2 = _two_forwards(scene)
    assert torch.equal(f1.detach(), alone[1][0]) and torch.equal(f2.detach(), alone[2][0])      # f1 read after f2 was rendered
    (L1 + L2).backward()
    _equal(_collect(scene), _sum(alone[1][1], alone[2][1]), "one backward")
    assert all(t.grad is not None for t in leaves)


def _either_order(scene, alone):
    names = _names(scene)
    for first in (1, 2):
        leaves = _arm(scene)
        _, _, L1, L2 = _two_forwards(scene)
        losses = {1: L1, 2: L2}
        got = {first: torch.autograd.grad(losses[first], leaves, retain_graph=True)}
        got[3 - first] = torch.autograd.grad(losses[3 - first], leaves)
        for idx in (1, 2):
            _equal(dict(zip(names, got[idx])), alone[idx][1], "view %d, view %d's backward first" % (idx, first))
        assert all(t.grad is None for t in leaves)


def test_two_views_one_backward_is_the_sum_of_the_alone_gradients(tmp_path, alone_rgb):
    _two_views_one_backward(_scene(tmp_path), alone_rgb)


def test_two_backwards_in_either_order_give_each_view_its_alone_gradient(tmp_path, alone_rgb):
    _either_order(_scene(tmp_path), alone_rgb)


# ---- 3: frames of other views, tile sizes and scenes between a forward and its backward
def test_frames_rendered_between_forward_and_backward_change_nothing(tmp_path, alone_rgb):
    scene = _scene(tmp_path / "small")
    big = _golden_scene(tmp_path / "big", load_golden("grad_trainedlike_128x128_n3000"))
    assert len(big.gaussians) == 3000
    _arm(scene)
    frame = scene.render_image_hip(1, geometry_gradients=True)
    with torch.no_grad():
        other = scene.render_image_hip(3, tile_size=8)
        again = scene.render_image_hip(1, use_hints=False)
        large = big.render_image_hip(1)
        assert other.abs().max() > 0 and large.shape == (128, 128, 3) and large.abs().max() > 0
        assert torch.equal(again, alone_rgb[1][0])
    assert torch.equal(frame.detach(), alone_rgb[1][0])
    (frame * _w(1)).sum().backward()
    _equal(_collect(scene), alone_rgb[1][1], "view 1 after three other frames")


# ---- 4: SH scenes, the inline path (every stored band active) and the _colors path (a degree below the stored one)
@pytest.mark.parametrize("active", [SH_DEGREE, 1])
def test_sh_scene_two_views_pending(tmp_path, tmp_path_factory, active):
    alone = _reference(tmp_path_factory, ("sh", active))
    scene = _scene(tmp_path, sh=True, active=active)
    assert scene._sh_truncated() == (active < SH_DEGREE)
    _two_views_one_backward(scene, alone)
    ka = (active + 1) ** 2
    assert not scene.gaussians.sh.grad[:, ka:].any() and scene.gaussians.sh.grad[:, :ka].abs().max() > 0
    assert scene.gaussians.colors.grad is None
    _either_order(scene, alone)


# ---- 5: the depth function beside the plain one
def _depth_loss(scene, f1, d1, f2, which):
    if which == "all":
        return (f1 * _w(1)).sum() + (d1 * _w(1, 2)).sum() + (f2 * _w(2)).sum()
    return (d1[..., 0] * _w(1, 2)[..., 0]).sum() + (f2 * _w(2)).sum()


@pytest.mark.parametrize("which", ["all", "depth channel only"])
def test_depth_function_and_plain_function_in_one_graph(tmp_path, alone_rgb, which):
    scene = _scene(tmp_path)
    _arm(scene)                 # view 1 alone, through the depth function
    f1, d1 = scene.render_image_depth_hip(1, tile_size=TILE)
    _depth_loss(scene, f1, d1, torch.zeros_like(f1), which).backward()
    alone_depth = _collect(scene)
    assert torch.equal(f1.detach(), alone_rgb[1][0])
    _arm(scene)
    f1, d1b = scene.render_image_depth_hip(1, tile_size=TILE)
    f2 = scene.render_image_hip(2, geometry_gradients=True)
    assert torch.equal(d1b.detach(), d1.detach()) and torch.equal(f2.detach(), alone_rgb[2][0])
    _depth_loss(scene, f1, d1b, f2, which).backward()
    _equal(_collect(scene), _sum(alone_depth, alone_rgb[2][1]), which)


# ---- 6: pose gradients of two views
def _camera_alone(scene, idx):
    _arm(scene)
    im = scene.images[idx]
    im.world2view.requires_grad_(True)
    im.world2view.grad = None
    frame = scene.render_image_hip(idx, geometry_gradients=True, camera_gradients=True)
    (frame * _w(idx)).sum().backward()
    out = im.world2view.grad.detach().clone()
    im.world2view.grad = None
    return out, _collect(scene)


def test_camera_gradients_of_two_pending_views_are_each_view_s_own(tmp_path, alone_rgb):
    scene = _scene(tmp_path)
    pose1, five1 = _camera_alone(scene, 1)
    pose2, five2 = _camera_alone(scene, 2)
    _equal(five1, alone_rgb[1][1], "camera entry, view 1")          # the Gaussians' gradients are the geometry entry's bits
    assert pose1.abs().max() > 0 and pose2.abs().max() > 0 and not torch.equal(pose1, pose2)
    _arm(scene)
    f1 = scene.render_image_hip(1, geometry_gradients=True, camera_gradients=True)
    f2 = scene.render_image_hip(2, geometry_gradients=True, camera_gradients=True)
    ((f1 * _w(1)).sum() + (f2 * _w(2)).sum()).backward()
    assert torch.equal(scene.images[1].world2view.grad, pose1) and torch.equal(scene.images[2].world2view.grad, pose2)
    assert scene.images[3].world2view.grad is None
    _equal(_collect(scene), _sum(five1, five2), "camera entry, two views")


# ---- 7: the screen statistic, one slot for two backwards
@pytest.mark.parametrize("mode", [True, "abs"])
def test_screen_statistic_after_two_pending_backwards_is_one_view_s_alone_statistic(tmp_path, alone_rgb, mode):
    scene = _scene(tmp_path)
    stat = {}
    for idx in (1, 2):
        scene.screen_statistics = None
        _, grads = _all_grads(scene, _w(idx), tile=TILE, idx=idx, screen_statistics=mode)
        _equal(grads, alone_rgb[idx][1], "screen entry, view %d" % idx)
        stat[idx] = scene.screen_statistics
        assert stat[idx][0] == idx and len(stat[idx]) == (4 if mode == "abs" else 3)
        assert all(t.abs().max() > 0 for t in stat[idx][1:])
    assert not torch.equal(stat[1][1], stat[2][1])
    scene.screen_statistics = None
    _arm(scene)
    f1, f2, L1, L2 = _two_forwards(scene, screen_statistics=mode)
    assert scene.screen_statistics is None
    (L1 + L2).backward()
    got = scene.screen_statistics
    assert got[0] in (1, 2) and len(got) == len(stat[got[0]])       # the view whose backward ran last: autograd's choice
    for a, b in zip(got[1:], stat[got[0]][1:]):
        assert torch.equal(a, b)
    _equal(_collect(scene), _sum(alone_rgb[1][1], alone_rgb[2][1]), "screen entry, two views")


# ---- 8: through the photometric loss
def test_two_views_through_the_photometric_loss(tmp_path):
    scene = _scene(tmp_path)
    with torch.no_grad():
        targets = {idx: (scene.render_image_hip(idx) * 0.5 + 0.1).clone() for idx in (1, 2)}
    alone = {}
    for idx in (1, 2):
        _arm(scene)
        scene.photometric_loss(idx, scene.render_image_hip(idx, geometry_gradients=True), targets[idx]).backward()
        alone[idx] = _collect(scene)
    _arm(scene)
    f1 = scene.render_image_hip(1, geometry_gradients=True)
    f2 = scene.render_image_hip(2, geometry_gradients=True)
    (scene.photometric_loss(1, f1, targets[1]) + scene.photometric_loss(2, f2, targets[2])).backward()
    _equal(_collect(scene), _sum(alone[1], alone[2]), "photometric loss")


# ---- 9: what changed under a pending frame is refused by name before anything is launched; the rest is not
def _refused(scene, loss, what, idx=1):
    before = scene.screen_statistics
    with pytest.raises(RuntimeError, match="render the frame again") as err:
        loss.backward()
    assert what in str(err.value) and "view %d" % idx in str(err.value), str(err.value)
    g = scene.gaussians
    for name in ("points", "scales", "quaternions", "opacity", "colors", "sh"):
        assert getattr(g, name, None) is None or getattr(g, name).grad is None, name
    assert scene.screen_statistics is before


def _pending(scene, idx=1):
    """A screen-statistics backward that fills the slot, then a frame of view idx left pending."""
    _arm(scene)
    (scene.render_image_hip(idx, geometry_gradients=True, screen_statistics=True) * _w(idx)).sum().backward()
    assert scene.screen_statistics is not None and scene.screen_statistics[0] == idx
    _arm(scene)
    return (scene.render_image_hip(idx, geometry_gradients=True, screen_statistics=True) * _w(idx)).sum()


def _fresh_alone(path, g, idx):
    """The alone result of a NEW scene holding copies of g's arrays as they are now."""
    from intro_to_gaussian_splatting_amd import GaussianScene, Gaussians

    fresh = Gaussians.from_arrays(g.points.detach().cpu(), g.colors.detach().cpu() * 256, g.scales.detach().cpu(),
                                  g.quaternions.detach().cpu(), g.opacity.detach().cpu(), device=DEV)
    fresh.colors = g.colors.detach().clone()
    return _alone(GaussianScene(str(path), fresh), idx)


def test_a_pose_set_under_a_pending_frame_is_refused_and_another_view_s_is_not(tmp_path, alone_rgb):
    scene = _scene(tmp_path)
    loss = _pending(scene)
    scene.images[3].set_world2view(scene.images[3].world2view.detach())         # another view: not this frame's business
    loss.backward()
    _equal(_collect(scene), alone_rgb[1][1], "view 1, view 3's pose set")
    loss = _pending(scene)
    scene.images[1].set_world2view(scene.images[2].world2view.detach())
    _refused(scene, loss, "pose")
    # view 1 now stands where view 2 stands: a fresh forward and backward give view 2's alone result
    frame, grads = _all_grads(scene, _w(2), tile=TILE, idx=1)
    assert torch.equal(frame, alone_rgb[2][0])
    _equal(grads, alone_rgb[2][1], "view 1 at view 2's pose")


def test_points_replaced_under_a_pending_frame_are_refused(tmp_path, alone_rgb):
    scene = _scene(tmp_path)
    g = scene.gaussians
    loss = _pending(scene)
    g.points = g.points.detach().clone().requires_grad_()
    _refused(scene, loss, "gaussians.points ")
    frame, grads = _alone(scene, 1)
    assert torch.equal(frame, alone_rgb[1][0])
    _equal(grads, alone_rgb[1][1], "after the refusal")


def test_an_sh_degree_raised_under_a_pending_frame_is_refused_and_the_same_value_is_not(tmp_path, tmp_path_factory):
    scene = _scene(tmp_path, sh=True, active=1)
    g = scene.gaussians
    loss = _pending(scene)
    g.active_sh_degree = 1
    loss.backward()
    _equal(_collect(scene), _reference(tmp_path_factory, ("sh", 1))[1][1], "the same degree assigned again")
    loss = _pending(scene)
    assert g.oneup_sh_degree() == 2
    _refused(scene, loss, "active_sh_degree")
    frame, grads = _alone(scene, 1)
    want = _reference(tmp_path_factory, ("sh", 2))[1]
    assert torch.equal(frame, want[0])
    _equal(grads, want[1], "after the refusal, at degree 2")


def test_a_densify_round_under_a_pending_frame_is_refused_and_another_scene_s_round_is_not(tmp_path, alone_rgb):
    from intro_to_gaussian_splatting_amd import DensityControl

    scene, other = _scene(tmp_path / "a"), _scene(tmp_path / "b")
    g = scene.gaussians
    _arm(other)
    loss = _pending(scene)
    knob = float(torch.quantile(other.gaussians.opacity.detach().reshape(-1), 0.1))
    counts = DensityControl(other.gaussians, scene=other, prune_logit=knob).densify_and_prune(
        generator=torch.Generator(device=DEV).manual_seed(1))
    assert counts["n_pruned"] > 0 and len(other.gaussians) == counts["n_out"] < len(g)
    loss.backward()             # the other scene's rows are not this frame's business
    _equal(_collect(scene), alone_rgb[1][1], "another scene densified")
    loss = _pending(scene)
    counts = DensityControl(g, scene=scene, prune_logit=knob).densify_and_prune(generator=torch.Generator(device=DEV).manual_seed(1))
    assert counts["n_pruned"] > 0 and len(g) == counts["n_out"] < 300 and scene.screen_statistics is None
    _refused(scene, loss, "gaussians.points ")
    frame, grads = _alone(scene, 1)
    want = _fresh_alone(tmp_path / "a", g, 1)
    assert torch.equal(frame, want[0]) and grads["points"].shape == (counts["n_out"], 3)
    _equal(grads, want[1], "after the round")


def test_a_relocation_at_the_cap_keeps_the_row_count_and_is_refused_all_the_same(tmp_path):
    from intro_to_gaussian_splatting_amd import MCMCControl

    scene = _scene(tmp_path)
    g = scene.gaussians
    n = len(g)
    with torch.no_grad():       # a third of the rows dead: something to relocate
        g.opacity[::3] = -12.0
    loss = _pending(scene)
    counts = MCMCControl(g, scene=scene, cap_max=n).relocate(generator=torch.Generator(device=DEV).manual_seed(2))
    assert counts["n_out"] == n == len(g) and counts["n_dead"] >= n // 3 and counts["n_live"] > 0, counts
    _refused(scene, loss, "gaussians.points ")         # the same count: nothing else would have objected
    frame, grads = _alone(scene, 1)
    want = _fresh_alone(tmp_path, g, 1)
    assert torch.equal(frame, want[0])
    _equal(grads, want[1], "after the relocation")
