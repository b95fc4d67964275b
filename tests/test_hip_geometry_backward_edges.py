"""Geometry gradients on the GPU (gsx_render_backward_geometry) at the edges the colour and opacity gradients are held to
(tests/test_hip_backward_edges.py): Gaussians that must get exactly zero, the row classes of one to three visible
Gaussians, faint records, runs of equal depth, the ways autograd hands over dL/dframe, quaternions far from unit length
and of either sign, a workspace another scene has used, and the whole training step through the photometric loss.

Every comparison with the float64 restatement (tests/geometry_backward_restatement.py) is test_hip_geometry_backward's
_check: 12 E_REF per output and Gaussian (test_geometry_backward_host.py), per_gaussian_error's SUBNORMAL floor,
finiteness.  The scenes are the colour suite's own, same seeds.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden

import backward_restatement
import geometry_backward_restatement as gbr
from test_geometry_backward_host import BOUND_RESTATEMENT
from test_hip_backward import DEV, _golden_scene, _oracle_pre, _scene
from test_hip_backward_edges import _duplicated_scene
from test_hip_geometry_backward import GEOMETRY, _all_grads, _camera, _check, _W
from test_hip_sh_backward import _sh_scene

pytestmark = pytest.mark.gpu

# Worst error / scale against the restatement that each test printed on an MI355X (bounds: 12 E_REF = 2.61e-07, 5.62e-06,
# 4.55e-08):
#                                                   points      scales      quaternions
#   three tiles                                     1.22e-08    1.38e-08    3.83e-10
#   last row / column                               6.60e-09    8.41e-09    4.06e-10
#   n=1 visible=1                                   1.61e-09    2.29e-09    6.70e-11
#   n=3 visible=3                                   6.27e-10    7.55e-10    1.06e-10
#   n=500 visible=1                                 4.07e-10    1.26e-10    3.95e-11
#   n=500 visible=3                                 7.16e-10    4.91e-10    5.36e-11
#   faint (rows above the moment floor)             1.73e-07    1.63e-07    6.11e-09
#   ties n=6000                                     1.15e-08    5.56e-09    2.68e-10
#   ties n=200000, eight tiles                      9.11e-08    3.29e-08    1.88e-09
#   (the same scene, unscaled)                      4.55e-09    3.95e-09    2.16e-10
#   quaternions rescaled                            4.19e-09    3.44e-09    1.86e-10
#   rescaled against unscaled (bound 2 x 12 E_REF)  6.89e-09    6.59e-09
# The training step: photometric loss 0.060862 -> 0.0117001 in thirty Adam steps.
ALL = GEOMETRY + ("colors", "opacity")
# float32's smallest normal is 1.2e-38.  Below it a term of a moment has lost its relative precision, or is flushed; a
# tile sums at most a few thousand such terms, so a moment's absolute error can reach about 1e-35.  Held to 1e-8 of the
# moment (the order of 12 E_REF), that needs the moment at or above 1e-27.  per_gaussian_error's SUBNORMAL floor is on
# the OUTPUT and does not cover this: the chain multiplies the moments by about 1e3 on the faint scene.
MOMENT_FLOOR = 1e-27


def _np(grads):
    return {k: v.cpu().numpy() for k, v in grads.items()}


def _on_lists(pre, n, tiles, tile=16):
    """Rows (original index) that are on the list of at least one of `tiles`."""
    from oracle import cpu_ref

    on = np.zeros(n, bool)
    for x0, y0 in tiles:
        on[np.asarray(pre.order)[cpu_ref.tile_list(pre, x0, y0, tile)]] = True
    return on


def _poison(n):
    """NaN in what the caching allocator hands out next: a large block, and freed blocks of exactly the five outputs'
    sizes (a free block of the requested size is the allocator's best fit), each between two live spacers so that they
    do not merge into one large block.  Returns the spacers: keep them until the gradients exist.  The zeros must be
    written, not inherited."""
    torch.full((1 << 20,), float("nan"), device=DEV).sum()
    spacers, poisoned = [], []
    for k in (3, 3, 4, 3, 1) * 8:
        poisoned.append(torch.full((n, k), float("nan"), device=DEV))
        spacers.append(torch.empty((n, k), device=DEV))
    poisoned[0].sum()
    del poisoned
    return spacers


def test_gaussians_off_the_graded_tiles_get_exact_zeros(tmp_path):
    """W non-zero on three tiles: every Gaussian on none of their lists gets exactly 0.0 in all three outputs (a slot pair
    that went to the wrong Gaussian would not be hidden by a tolerance); the others match the restatement.

    Graded on three tiles only, five Gaussians of this scene reach a graded tile with nothing but the far tail of their
    footprint (absolute moments 1.6e-41 .. 7.3e-30, gradients 1e-38 .. 1e-32): rows that v_exp_f32's flush of alpha
    below 2^-126 once left at zero (5.85e-03, 1.78e-02, 8.19e-07 of their scale) and alpha_ref_tail now carries."""
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    sc = make_scene(3000, 128, 128, seed=12)
    scene = _scene(tmp_path, sc)
    rng = np.random.default_rng(12)
    tiles = [(16, 32), (64, 0), (96, 96)]
    Wn = np.zeros((128, 128, 3), np.float32)
    for x0, y0 in tiles:
        Wn[x0:x0 + 16, y0:y0 + 16] = rng.standard_normal((16, 16, 3))
    W = torch.from_numpy(Wn).to(DEV)
    spacers = _poison(3000)
    frame, grads = _all_grads(scene, W)
    del spacers
    on = _on_lists(_oracle_pre(scene, sc), 3000, tiles)
    assert on.sum() > 50 and (~on).sum() > 1000
    for key, got in _np(grads).items():
        assert not got[~on].any(), key
        assert (np.abs(got[on]).sum(1) > 0).sum() >= 50, key
    _check(scene, sc, frame, Wn, 16, grads, "three tiles", tiles=tiles)


def test_gaussians_only_on_the_unrendered_last_tiles_get_exact_zeros(tmp_path):
    """REF_CPU never renders the last tile row and column: a visible Gaussian whose rectangle reaches only those gets
    exactly 0.0 in all three outputs, with W non-zero there too."""
    from intro_to_gaussian_splatting_amd.synthetic import make_scene
    from oracle import cpu_ref

    sc = make_scene(2000, 96, 80, seed=21)
    scene = _scene(tmp_path, sc)
    W = _W((96, 80, 3), 21)
    spacers = _poison(2000)
    frame, grads = _all_grads(scene, W)
    del spacers
    _check(scene, sc, frame, W, 16, grads, "last row / column")
    pre = _oracle_pre(scene, sc)
    on = _on_lists(pre, 2000, [(x0, y0) for x0 in cpu_ref.tile_origins(96, 16) for y0 in cpu_ref.tile_origins(80, 16)])
    visible = np.zeros(2000, bool)
    visible[np.asarray(pre.order)] = True
    edge_only = visible & ~on
    print("last row / column: %d visible Gaussians on no rendered tile" % edge_only.sum())
    assert edge_only.sum() >= 10
    for key, got in _np(grads).items():
        assert not got[~on].any(), key
        assert got[on].any(), key


def test_no_visible_gaussian_gives_all_zero_gradients(tmp_path):
    """The m == 0 return: the five outputs come from torch.empty, and the zeros must be written, not inherited."""
    from intro_to_gaussian_splatting_amd.synthetic import make_few_visible_scene

    sc = make_few_visible_scene(64, 48, 48, seed=5, visible=0)
    scene = _scene(tmp_path, sc)
    W = _W((48, 48, 3), 5)
    spacers = _poison(64)
    frame, grads = _all_grads(scene, W)
    del spacers
    assert not frame.any()
    for key, width in (("points", 3), ("scales", 3), ("quaternions", 4), ("colors", 3), ("opacity", 1)):
        assert grads[key].shape == (64, width), key
        assert torch.isfinite(grads[key]).all() and not grads[key].any(), key


@pytest.mark.parametrize("n,visible", [(1, 1), (3, 3), (500, 1), (500, 3)])
def test_one_to_three_visible_gaussians_match_restatement(tmp_path, n, visible):
    """The row classes GSX_FLAG_ONE_VISIBLE / SMALL_BATCH: launch_project_raw projects in another float order there than
    the chain recomputes (rows class kRowsMany).  The scenes of tests/golden/geomgrad_rows*."""
    from intro_to_gaussian_splatting_amd.synthetic import make_few_visible_scene, make_scene

    seed = {(1, 1): 40, (3, 3): 40, (500, 1): 41, (500, 3): 43}[n, visible]     # every visible one on a rendered tile
    if n == visible:
        sc = make_scene(n, 48, 48, seed=seed)
    else:
        sc = make_few_visible_scene(n, 48, 48, seed=seed, visible=visible)
    scene = _scene(tmp_path, sc)
    W = _W((48, 48, 3), n + visible)
    st = {}
    frame, grads = _all_grads(scene, W, stats=st)
    assert st["n_visible"] == visible
    out = _check(scene, sc, frame, W, 16, grads, "n=%d visible=%d" % (n, visible))
    for k, key in enumerate(GEOMETRY):
        assert (np.abs(out[k]).sum(1) > 0).sum() == visible, key
        assert int((grads[key].abs().sum(1) > 0).sum()) == visible, key
    with torch.no_grad():
        again = scene.render_image_hip(1, tile_size=16)
    assert torch.equal(again, frame)


def _check_above_the_moment_floor(scene, sc, frame, W, tile, grads, tag, tiles=None):
    """_check on every row whose non-zero absolute moments (Sabs of gbr.moments) are all at or above MOMENT_FLOOR; a row
    below it is held to finiteness only (it takes the restatement's own value into _check).  A condition on the inputs,
    computed from the float64 restatement alone.  Returns (the restatement's result, the rows left out, the lit rows)."""
    as_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)  # noqa: E731
    pre = _oracle_pre(scene, sc)
    order = np.asarray(pre.order)
    n, w, h = sc["points"].shape[0], int(sc["width"]), int(sc["height"])
    _, Sabs = gbr.moments(pre, as_np(frame), as_np(W), w, h, tile, tiles=tiles)
    lit, below = np.zeros(n, bool), np.zeros(n, bool)
    lit[order[Sabs.sum(1) > 0]] = True
    below[order[((Sabs > 0) & (Sabs < MOMENT_FLOOR)).any(1)]] = True
    print("%s: %d lit rows, %d with a non-zero absolute moment below %g" % (tag, lit.sum(), below.sum(), MOMENT_FLOOR))
    ref = gbr.geometry_backward(pre, sc["points"], sc["scales"], sc["quaternions"], _camera(scene), as_np(frame), as_np(W),
                                w, h, tile, tiles=tiles)
    held = {}
    for k, key in enumerate(GEOMETRY):
        got = as_np(grads[key]).astype(np.float64)
        assert np.isfinite(got).all(), (tag, key)
        held[key] = np.where(below[:, None], ref[k], got)
    return _check(scene, sc, frame, W, tile, held, tag + " (rows above the moment floor)", tiles=tiles), below, lit


def test_faint_gaussians_keep_their_geometry_gradient(tmp_path):
    """Footprints of ~0.1 px (sigma_scale 0.07): many Gaussians have alpha < 2^-26 at every pixel centre of their tiles.
    The forward skips such records, the reference does not, and the geometry instance of the tile kernel must not either.
    Every row is held to the restatement, except that a row with a non-zero absolute moment below MOMENT_FLOOR is held
    to finiteness only (a condition on the inputs: 5 of 355 lit rows on the CPU; at most 3 % may be left out)."""
    from intro_to_gaussian_splatting_amd.synthetic import make_scene
    from oracle import cpu_ref

    sc = make_scene(600, 64, 48, seed=23, sigma_scale=0.07)
    scene = _scene(tmp_path, sc)
    W = _W((64, 48, 3), 23)
    frame, grads = _all_grads(scene, W)
    out, below, lit = _check_above_the_moment_floor(scene, sc, frame, W, 16, grads, "faint")
    assert lit.sum() >= 300 and below.sum() <= 0.03 * lit.sum()
    got = _np(grads)
    pre = _oracle_pre(scene, sc)
    order = np.asarray(pre.order)
    # the Gaussians that are faint on every pixel centre of every tile they are binned into
    amax = np.zeros(order.shape[0])
    op32 = (1.0 / (1.0 + np.exp(-np.asarray(pre.sigmoid_opacity, np.float64).reshape(-1)))).astype(np.float32)
    for x0 in cpu_ref.tile_origins(64, 16):
        for y0 in cpu_ref.tile_origins(48, 16):
            xs, ys = np.meshgrid(np.arange(x0, x0 + 16), np.arange(y0, y0 + 16), indexing="ij")
            px, py = xs.reshape(-1).astype(np.float32), ys.reshape(-1).astype(np.float32)
            for k in cpu_ref.tile_list(pre, x0, y0, 16):
                a = backward_restatement._alpha32(pre.points_xy[k, 0], pre.points_xy[k, 1], pre.inverse_covariance_2d[k],
                                                  op32[k], px, py)
                amax[k] = max(amax[k], float(a.max()))
    faint = order[(amax > 0) & (amax < 2.0 ** -26)]
    kept = faint[~below[faint]]
    print("faint: %d Gaussians below 2^-26 everywhere, %d of them above the moment floor" % (faint.size, kept.size))
    assert kept.size >= 10
    for k, key in enumerate(GEOMETRY):
        assert (np.abs(out[k][kept]).sum(1) > 0).all(), key
        assert (np.abs(got[key][kept]).sum(1) > 0).all(), key


def test_depth_ties_one_workgroup_sort(tmp_path):
    """Runs of four equal depths (the same point, scale and rotation; other colours and opacities per copy): the moments
    of each copy must land in that copy's slots."""
    sc = _duplicated_scene(1500, 128, 128, seed=61)       # 6000 Gaussians <= 16 384: the one-workgroup depth sort
    scene = _scene(tmp_path, sc)
    W = _W((128, 128, 3), 61)
    frame, grads = _all_grads(scene, W)
    _check(scene, sc, frame, W, 16, grads, "ties n=6000")
    d = np.ascontiguousarray(_oracle_pre(scene, sc).depths, np.float32).view(np.uint32)
    assert (d[1:] == d[:-1]).sum() >= 1000
    gp = grads["points"].cpu().numpy().reshape(1500, 4, 3)
    differ = (gp != gp[:, :1]).any((1, 2))
    print("ties n=6000: %d base Gaussians whose copies do not share one row of dL/dpoints" % differ.sum())
    assert differ.sum() >= 100


def test_depth_ties_sampled_sort(tmp_path):
    """200 000 Gaussians (16 384 < n <= 1.5M: the sampled depth sort), runs of four equal depths; eight graded tiles
    (52 of the 5728 lit rows reach them with the far tail of their footprint only: alpha_ref_tail's rows)."""
    sc = _duplicated_scene(50_000, 640, 480, seed=67)
    scene = _scene(tmp_path, sc)
    rng = np.random.default_rng(68)
    tiles = [(int(x) * 16, int(y) * 16) for x, y in zip(rng.integers(0, 39, 8), rng.integers(0, 29, 8))]
    Wn = np.zeros((640, 480, 3), np.float32)
    for x0, y0 in tiles:
        Wn[x0:x0 + 16, y0:y0 + 16] = rng.standard_normal((16, 16, 3))
    frame, grads = _all_grads(scene, torch.from_numpy(Wn).to(DEV))
    out = _check(scene, sc, frame, Wn, 16, grads, "ties n=200000, eight tiles", tiles=tiles)
    gp = grads["points"].cpu().numpy().reshape(50_000, 4, 3)
    assert (np.abs(out[0]).sum(1) > 0).sum() >= 1000 and (gp != gp[:, :1]).any((1, 2)).sum() >= 100


def test_grad_frame_arrives_in_any_layout(tmp_path):
    """dL/dframe as autograd hands it over -- expanded (stride 0), through a select, through a permute -- gives the
    gradients of the same W passed explicitly, bit for bit in all five outputs; backward twice gives exactly twice them."""
    gg = load_golden("grad_small_64x48_n300")
    scene = _golden_scene(tmp_path, gg)
    g = scene.gaussians
    W = torch.from_numpy(gg["W"]).to(DEV)

    def run(loss_of, times=1):
        for name in ALL:
            getattr(g, name).requires_grad_(True)
            getattr(g, name).grad = None
        frame = scene.render_image_hip(1, tile_size=16, geometry_gradients=True)
        loss = loss_of(frame)
        for k in range(times):
            loss.backward(retain_graph=k + 1 < times)
        out = {name: getattr(g, name).grad.detach().clone() for name in ALL}
        for name in ALL:
            getattr(g, name).requires_grad_(False)
            getattr(g, name).grad = None
        return out

    ones = torch.ones((64, 48, 3), device=DEV)
    chan1 = torch.zeros((64, 48, 3), device=DEV)
    chan1[..., 1] = 1.0
    for tag, loss_of, Wx in (("expanded", lambda f: f.sum(), ones),
                             ("select", lambda f: f[..., 1].sum(), chan1),
                             ("permute", lambda f: (f.permute(1, 0, 2) * W.permute(1, 0, 2)).sum(), W)):
        want = run(lambda f: (f * Wx).sum())
        got = run(loss_of)
        for name in ALL:
            assert want[name].abs().max() > 0 and torch.equal(got[name], want[name]), (tag, name)
    want = run(lambda f: (f * W).sum())
    twice = run(lambda f: (f * W).sum(), times=2)
    for name in ALL:
        assert torch.equal(twice[name], 2 * want[name]), name


def test_quaternions_far_from_unit_length_and_of_either_sign(tmp_path):
    """Every quaternion row times a factor log-uniform in [1e-3, 1e3], every second row negated: both normalisations and
    the 1 / n1 factor.  The gradient stays orthogonal to q, and dL/dpoints and dL/dscales stay what they were."""
    gg = load_golden("grad_small_64x48_n300")
    keys = ("points", "colors_0_255", "scales", "quaternions", "opacity", "qvec", "tvec", "fx", "fy", "cx", "cy",
            "width", "height", "colors")
    sc = {k: gg[k] for k in keys}
    factor = np.exp(np.random.default_rng(5).uniform(np.log(1e-3), np.log(1e3), 300)).astype(np.float32)
    factor[1::2] *= -1
    sc2 = dict(sc, quaternions=(sc["quaternions"] * factor[:, None]).astype(np.float32))
    norms = np.sqrt((sc2["quaternions"].astype(np.float64) ** 2).sum(1))
    assert norms.min() < 1e-2 and norms.max() > 1e2
    W = torch.from_numpy(gg["W"]).to(DEV)
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    scene = _golden_scene(tmp_path / "a", sc)
    frame, grads = _all_grads(scene, W)
    out = _check(scene, sc, frame, W, 16, grads, "(the same scene, unscaled)")
    scene2 = _golden_scene(tmp_path / "b", sc2)
    frame2, grads2 = _all_grads(scene2, W)
    out2 = _check(scene2, sc2, frame2, W, 16, grads2, "quaternions rescaled")
    # the restatement's gradient is orthogonal to q to 1e-12: only the kernel's bounded error remains
    q = sc2["quaternions"].astype(np.float64)
    gq = grads2["quaternions"].cpu().numpy().astype(np.float64)
    assert np.abs(gq).max() > 0
    dot = np.abs((q * gq).sum(1))
    allowed = np.abs(q).sum(1) * (BOUND_RESTATEMENT["quaternions"] * out2[5] + backward_restatement.SUBNORMAL)
    assert (dot <= allowed).all(), float((dot - allowed).max())
    # both runs are within the bound of their restatements, and those agree (on the same stage 1 to 1e-11; here each has
    # the float32 stage 1 of its own quaternions, and they differ by 3.6e-9 of the scale at most: measured on the CPU)
    for k, key in ((0, "points"), (1, "scales")):
        er = gbr.per_gaussian_error(out2[k], out[k], out[3 + k])
        e = gbr.per_gaussian_error(grads2[key].cpu().numpy(), grads[key].cpu().numpy(), out[3 + k])
        print("rescaled vs unscaled: %s: max difference / scale %.4g (bound %.3g); the two restatements %.3g" % (
            key, e, 2 * BOUND_RESTATEMENT[key], er))
        assert er <= 1e-8, (key, er)
        assert e <= 2 * BOUND_RESTATEMENT[key], (key, e)


def test_workspace_another_scene_used_gives_the_same_bits(tmp_path):
    """A, then the larger B, then A again: the slot arrays, the pair lists and the geometry outputs' zeroing leave
    nothing of B behind."""
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    gg = load_golden("grad_small_64x48_n300")
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    scene_a = _golden_scene(tmp_path / "a", gg)
    scene_b = _scene(tmp_path / "b", make_scene(3000, 128, 128, seed=12))
    Wa, Wb = torch.from_numpy(gg["W"]).to(DEV), _W((128, 128, 3), 12)
    f0, first = _all_grads(scene_a, Wa)
    _, other = _all_grads(scene_b, Wb)
    f1, third = _all_grads(scene_a, Wa)
    assert torch.equal(f0, f1)
    for name in ALL:
        assert other[name].abs().max() > 0 and first[name].abs().max() > 0, name
        assert torch.equal(third[name], first[name]), name


# ---- the training step
TRAINED = ("points", "scales", "quaternions", "opacity", "sh")
# Adam step sizes of the 30 steps: the coefficients and logits as the merged 30-step tests take them; the geometry in its
# own units (the scene's depths are 2 .. 10 and its scales of the order of 1e-2, quaternions of order 1)
LR = {"sh": 0.02, "opacity": 0.02, "quaternions": 1e-3, "points": 1e-4, "scales": 1e-4}


def _perturbed_target(scene, seed):
    """test_hip_photometric_loss's _perturbed_target with the geometry perturbed too: the frame of the scene with noise
    on the coefficients (0.2), the quaternions (0.1), the points (0.01) and, by a factor exp(N(0, 0.1)), the scales."""
    g = scene.gaussians
    rs = np.random.RandomState(seed)
    noise = lambda t, sigma: torch.from_numpy(rs.normal(0, sigma, size=tuple(t.shape)).astype(np.float32)).to(DEV)  # noqa: E731
    with torch.no_grad():
        keep = {k: getattr(g, k).clone() for k in ("sh", "quaternions", "points", "scales")}
        g.sh.add_(noise(g.sh, 0.2))
        g.quaternions.add_(noise(g.quaternions, 0.1))
        g.points.add_(noise(g.points, 0.01))
        g.scales.mul_(torch.exp(noise(g.scales, 0.1)))
        target = scene.render_image_hip(1).clone()
        for k, v in keep.items():
            getattr(g, k).copy_(v)
    return target


def test_training_step_through_the_photometric_loss(tmp_path):
    """scene.photometric_loss on a frame rendered with geometry_gradients=True: the five gradients are those of
    frame.backward(gradient = the library's dL/dframe), bit for bit; thirty Adam steps on all five groups lower the loss."""
    from intro_to_gaussian_splatting_amd.loss import _call as loss_call

    scene, _ = _sh_scene(tmp_path, 2)
    g = scene.gaussians
    target = _perturbed_target(scene, 5)
    a, b = scene.rendered_region(1)

    def run(make_loss):
        for k in TRAINED:
            getattr(g, k).requires_grad_(True)
            getattr(g, k).grad = None
        frame = scene.render_image_hip(1, geometry_gradients=True)
        make_loss(frame)
        grads = {k: getattr(g, k).grad.detach().clone() for k in TRAINED}
        for k in TRAINED:
            getattr(g, k).requires_grad_(False)
            getattr(g, k).grad = None
        return frame.detach(), grads

    frame, got = run(lambda f: scene.photometric_loss(1, f, target).backward())
    G = loss_call(frame, target, 0.2, (a, b), True)[1]
    assert G[:a, :b].abs().max() > 0
    _, want = run(lambda f: f.backward(gradient=G))
    for k in TRAINED:
        assert got[k].shape == getattr(g, k).shape and torch.isfinite(got[k]).all(), k
        assert got[k].abs().max() > 0 and torch.equal(got[k], want[k]), k

    for k in TRAINED:
        getattr(g, k).requires_grad_(True)
    opt = torch.optim.Adam([dict(params=[getattr(g, k)], lr=LR[k]) for k in TRAINED])
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = scene.photometric_loss(1, scene.render_image_hip(1, geometry_gradients=True), target)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in losses]
    print("photometric loss, all five groups: first %.6g, last %.6g" % (losses[0], losses[-1]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    for k in TRAINED:
        getattr(g, k).requires_grad_(False)
