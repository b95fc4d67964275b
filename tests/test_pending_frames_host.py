"""Frames whose backward is still pending, host side.  The backward of a differentiable frame reads the live scene again --
the arrays, the row order, the view's camera, the active SH degree -- and trusts the forward's counts, so a change autograd
cannot see between forward and backward has to be refused: ``gaussian_scene._pending_snapshot`` (forward) and
``_check_pending`` (backward, before any library call), held here on CPU scenes, alone and through the two autograd functions
with the library calls stubbed.  Without the check the stubbed backwards below run on the changed scene and raise nothing.
tests/test_hip_pending_frames.py holds the same end to end on the GPU."""
import numpy as np
import pytest
import torch

FIVE = ("points", "scales", "quaternions", "opacity", "colors")
FIVE_SH = ("points", "scales", "quaternions", "opacity", "sh")
N, W, H = 40, 32, 24


def _scene(path, sh_degree=None, active=None):
    """A CPU scene of N Gaussians with views 1, 2 and 3; with ``sh_degree`` an SH scene stored at that degree."""
    from intro_to_gaussian_splatting_amd import Gaussians, GaussianScene
    from intro_to_gaussian_splatting_amd.synthetic import make_scene, orbit_poses, write_colmap_text

    sc = make_scene(N, W, H, seed=4)
    write_colmap_text(str(path), sc, extra_poses=orbit_poses(2, step_deg=8.0))
    g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"], device="cpu")
    if sh_degree is not None:
        g.sh = torch.from_numpy(np.random.default_rng(1).standard_normal((N, (sh_degree + 1) ** 2, 3)).astype(np.float32))
        g.sh_degree = sh_degree
        if active is not None:
            g.active_sh_degree = active
    scene = GaussianScene(str(path), g)
    assert sorted(scene.images) == [1, 2, 3]
    return scene


def _snap(scene, idx=1):
    from intro_to_gaussian_splatting_amd.gaussian_scene import _pending_snapshot

    g = scene.gaussians
    return _pending_snapshot(scene, idx, g.points, g.scales, g.quaternions, g.opacity, g.colors, getattr(g, "sh", None))


def _check(state):
    from intro_to_gaussian_splatting_amd.gaussian_scene import _check_pending

    _check_pending(state)


def _refused(state, idx, what):
    with pytest.raises(RuntimeError) as err:
        _check(state)
    text = str(err.value)
    assert "view %r" % idx in text and what in text and "render the frame again" in text, text
    return text


def test_an_unchanged_scene_passes_and_the_snapshot_holds_host_values_only(tmp_path):
    scene = _scene(tmp_path)
    state = _snap(scene)
    _check(state)
    _check(state)           # the comparison changes nothing
    assert [a[0] for a in state.arrays] == list(FIVE)
    for name, address, shape in state.arrays:
        assert isinstance(address, int) and shape == tuple(getattr(scene.gaussians, name).shape)
    assert state.bands is None and state.pose_version == 0
    sh_state = _snap(_scene(tmp_path / "sh", sh_degree=2, active=1))
    assert [a[0] for a in sh_state.arrays] == list(FIVE_SH) and sh_state.bands == (2, 1)


def test_the_same_pose_set_again_is_a_new_pose_and_another_view_s_pose_is_not_this_one_s(tmp_path):
    scene = _scene(tmp_path)
    state1, state2 = _snap(scene, 1), _snap(scene, 2)
    before = scene.images[1].world2view.detach().clone()
    scene.images[1].set_world2view(before)
    assert torch.equal(scene.images[1].world2view.detach(), before) and scene.images[1].pose_version == 1
    _refused(state1, 1, "pose")
    _check(state2)          # view 2 did not move
    fresh = _snap(scene, 1)
    _check(fresh)
    scene.images[3].set_world2view(scene.images[2].world2view.detach())
    _check(fresh)
    _check(state2)
    # the view's image replaced by another object at the same pose version
    scene.images[2] = scene.images[3]
    _refused(state2, 2, "pose")


def test_active_sh_degree_same_value_passes_another_is_refused_and_an_rgb_scene_ignores_it(tmp_path):
    scene = _scene(tmp_path, sh_degree=3, active=1)
    g = scene.gaussians
    state = _snap(scene)
    g.active_sh_degree = 1
    _check(state)
    assert g.oneup_sh_degree() == 2
    text = _refused(state, 1, "active_sh_degree")
    assert "1 at the forward, 2 now" in text
    g.active_sh_degree = 1
    _check(state)
    g.active_sh_degree = 0
    _refused(state, 1, "active_sh_degree")
    g.active_sh_degree = 1
    g.sh_degree = 2         # the stored layout reinterpreted
    _refused(state, 1, "sh_degree")
    g.sh_degree = 3
    _check(state)
    # every stored band active: one step down is refused too
    full = _scene(tmp_path / "full", sh_degree=2)
    state = _snap(full)
    assert state.bands == (2, 2)
    full.gaussians.active_sh_degree = 1
    _refused(state, 1, "active_sh_degree")
    # an RGB scene: the attribute is not read by its frames
    rgb = _scene(tmp_path / "rgb")
    state = _snap(rgb)
    rgb.gaussians._active_sh_degree = 0
    rgb.gaussians.sh_degree = 0
    _check(state)
    rgb.gaussians.sh = torch.zeros((N, 1, 3))        # ... but turning into an SH scene is a change
    _refused(state, 1, "gaussians.sh")


@pytest.mark.parametrize("sh", [False, True])
def test_each_array_replaced_by_a_clone_or_by_another_length_is_refused_by_name(tmp_path, sh):
    scene = _scene(tmp_path, sh_degree=1 if sh else None)
    g = scene.gaussians
    for name in FIVE_SH if sh else FIVE:
        state = _snap(scene)
        old = getattr(g, name)          # (kept alive, as save_for_backward keeps it: its address is not handed out again)
        setattr(g, name, old.detach().clone())
        assert getattr(g, name).shape == old.shape
        text = _refused(state, 1, "gaussians.%s " % name)
        assert sum(("gaussians.%s " % other) in text for other in FIVE + ("sh",)) == 1, text
        setattr(g, name, torch.cat([old, old[:3]]))         # N + 3 rows
        text = _refused(state, 1, "gaussians.%s " % name)
        assert str(tuple(old.shape)) in text and str((N + 3,) + tuple(old.shape[1:])) in text
        setattr(g, name, old[: N - 1])                      # N - 1 rows at the SAME address
        assert getattr(g, name).data_ptr() == old.data_ptr()
        _refused(state, 1, "gaussians.%s " % name)
        setattr(g, name, old)
        _check(state)
    # on an SH scene the frame does not read gaussians.colors: replacing it is nobody's business
    if sh:
        state = _snap(scene)
        g.colors = g.colors.clone()
        _check(state)


def test_the_container_replaced_is_refused(tmp_path):
    scene = _scene(tmp_path)
    state = _snap(scene)
    old = scene.gaussians
    other = _scene(tmp_path / "other").gaussians
    scene.gaussians = other
    _refused(state, 1, "scene.gaussians")
    scene.gaussians = old
    _check(state)


def test_the_row_order_appearing_disappearing_or_replaced_is_refused(tmp_path):
    scene = _scene(tmp_path)
    g = scene.gaussians
    oi = torch.arange(N, dtype=torch.int32)
    ro = torch.arange(N, dtype=torch.int32)
    state = _snap(scene)
    g.original_index = oi                   # appearing
    _refused(state, 1, "original_index")
    g.original_index = None
    g.row_of_index = ro
    _refused(state, 1, "row_of_index")
    g.original_index = oi
    ordered = _snap(scene)
    _check(ordered)
    g.original_index = oi.clone()           # replaced by an equal tensor
    _refused(ordered, 1, "original_index")
    g.original_index = oi
    g.row_of_index = ro.clone()
    _refused(ordered, 1, "row_of_index")
    g.row_of_index = ro
    _check(ordered)
    g.original_index = g.row_of_index = None        # disappearing
    _refused(ordered, 1, "original_index")
    _check(state)


def test_an_edit_in_place_is_left_to_autograd(tmp_path):
    scene = _scene(tmp_path, sh_degree=1)
    g = scene.gaussians
    state = _snap(scene)
    with torch.no_grad():
        for name in FIVE_SH:
            getattr(g, name).add_(1.0)
    _check(state)


# ---- through the autograd functions, the library calls stubbed
class _Stubbed:
    """A GaussianScene whose library calls are replaced by zeros of the right shapes, counting the backward's calls."""

    def __init__(self, scene):
        self.scene, self.backward_calls = scene, []
        scene.render_image_hip = self.render_image_hip
        scene._render_backward = self._render_backward
        scene._render_depth = self._render_depth
        scene._sh_backward = self._sh_backward

    def render_image_hip(self, image_idx, tile_size=16, layout="wh3", stats=None, **kw):
        if stats is not None:
            stats.update(n_instances=7, n_visible=N)
        return torch.zeros((W, H, 3))

    def _render_depth(self, image_idx, tile_size, layout, n_instances, n_visible):
        return torch.zeros((W, H, 2))

    def _render_backward(self, image_idx, *args, geometry=False, **kw):
        n = int(self.scene.gaussians.points.shape[0])
        self.backward_calls.append(image_idx)
        return tuple(torch.zeros((n, k)) for k in ((3, 1, 3, 3, 4) if geometry else (3, 1)))

    def _sh_backward(self, image_idx, grad_colors, with_points=False):
        g = self.scene.gaussians
        return torch.zeros(g.sh.shape), (torch.zeros((g.points.shape[0], 3)) if with_points else None)


def _apply(scene, idx, depth=False):
    from intro_to_gaussian_splatting_amd.gaussian_scene import _RenderImageDepthFunction, _RenderImageFunction

    g = scene.gaussians
    args = (g.points, g.scales, g.quaternions, g.opacity, g.colors, getattr(g, "sh", None))
    if depth:
        frame, d = _RenderImageDepthFunction.apply(scene, idx, 16, "wh3", {}, *args)
        return frame.sum() + d.sum()
    return _RenderImageFunction.apply(scene, idx, 16, "wh3", dict(geometry_gradients=True), *args).sum()


def _grads_none(g):
    return all(getattr(g, name).grad is None for name in FIVE + ("sh",) if getattr(g, name, None) is not None)


@pytest.mark.parametrize("depth", [False, True])
def test_both_functions_refuse_a_stale_backward_before_any_library_call(tmp_path, depth):
    scene = _scene(tmp_path)
    stub = _Stubbed(scene)
    g = scene.gaussians
    for name in FIVE:
        getattr(g, name).requires_grad_(True)
    # undisturbed, with a frame of another view pending and that view's pose set between: both run
    loss1, loss2 = _apply(scene, 1, depth), _apply(scene, 2, depth)
    scene.images[3].set_world2view(scene.images[3].world2view.detach())
    (loss1 + loss2).backward()
    assert sorted(stub.backward_calls) == [1, 2] and g.points.grad is not None
    for name in FIVE:
        getattr(g, name).grad = None
    stub.backward_calls.clear()

    def replace_points():
        g.points = g.points.detach().clone().requires_grad_()

    def reorder_rows():        # the same count: nothing else would object
        g.opacity = g.opacity.detach().flip(0).requires_grad_()

    changes = [("pose", lambda: scene.images[1].set_world2view(scene.images[1].world2view.detach())),
               ("gaussians.points ", replace_points), ("gaussians.opacity ", reorder_rows)]
    for what, change in changes:
        loss1, loss2 = _apply(scene, 1, depth), _apply(scene, 2, depth)
        change()
        with pytest.raises(RuntimeError, match="render the frame again") as err:
            loss1.backward()
        assert what in str(err.value) and "view 1" in str(err.value)
        assert stub.backward_calls == [] and _grads_none(g)
        if what == "pose":      # view 2's frame is still good
            loss2.backward()
            assert stub.backward_calls == [2]
            for name in FIVE:
                getattr(g, name).grad = None
            stub.backward_calls.clear()
        else:                   # its arrays are gone too
            with pytest.raises(RuntimeError, match="view 2"):
                loss2.backward()
            assert stub.backward_calls == []
    # an edit in place: autograd's own error, not this check's
    loss1 = _apply(scene, 1, depth)
    with torch.no_grad():
        g.scales.mul_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss1.backward()
    assert stub.backward_calls == []


def test_an_sh_frame_refuses_a_degree_raised_between_forward_and_backward(tmp_path):
    scene = _scene(tmp_path, sh_degree=2, active=0)
    stub = _Stubbed(scene)
    g = scene.gaussians
    g.sh.requires_grad_(True)
    loss = _apply(scene, 1)
    g.active_sh_degree = 0          # the same value
    loss.backward()
    assert stub.backward_calls == [1] and g.sh.grad is not None
    g.sh.grad = None
    stub.backward_calls.clear()
    loss = _apply(scene, 1)
    g.oneup_sh_degree()
    with pytest.raises(RuntimeError, match="active_sh_degree") as err:
        loss.backward()
    assert "view 1" in str(err.value) and "render the frame again" in str(err.value)
    assert stub.backward_calls == [] and g.sh.grad is None


def test_the_docstrings_say_who_checks_what():
    from intro_to_gaussian_splatting_amd import GaussianScene
    from intro_to_gaussian_splatting_amd.gaussian_scene import _RenderImageDepthFunction, _RenderImageFunction

    for fn in (_RenderImageFunction, _RenderImageDepthFunction):
        assert "_check_pending" in fn.__doc__ and "in place" in fn.__doc__.lower()
    assert "backward ran LAST" in GaussianScene.render_image_hip.__doc__
