"""Backward pass on the GPU at the edges backward_tile_kernel and gsx_render_backward branch on: tile sizes of more than
256 pixels or not a multiple of 64, the hw3 layout, Gaussians that must get exactly zero, the row classes of one to
three visible Gaussians, runs of equal depths through every depth-sort route, the ways autograd hands over dL/dframe,
and the opacity gradient against a finite difference of the frame itself.

Every gradient is held against the float64 restatement (tests/backward_restatement.py) Gaussian by Gaussian: the
error of each one is at most TOL times its own error scale (test_backward_host.py), however small it is next to the
largest gradient -- besides the max-normalised REL check."""
import numpy as np
import pytest
import torch

from conftest import load_golden

import backward_restatement
from test_backward_host import GRAD_SCENES, REL, TOL
from test_hip_backward import DEV, _golden_scene, _grads, _oracle_pre, _scene

pytestmark = pytest.mark.gpu

KEPT_MAX_256 = 1536 * 1024      # gsx_sort.hip kKeptMax256: above it (without a kept hint) the depth sort takes LSD


def _check(scene, sc, frame, W, tile, gc, go, tag, tiles=None, idx=1):
    """gc, go against the restatement: per Gaussian (TOL) and max-normalised (REL).  frame, W: (width, height, 3)."""
    pre = _oracle_pre(scene, sc, idx)
    n = sc["points"].shape[0]
    w, h = int(sc["width"]), int(sc["height"])
    as_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)  # noqa: E731
    rc, ro, sc_, so_ = backward_restatement.backward(pre, as_np(frame), as_np(W), w, h, tile, n, tiles=tiles,
                                                     with_scale=True)
    gc, go = as_np(gc).astype(np.float64), as_np(go).astype(np.float64)
    ec, eo = backward_restatement.per_gaussian_error(gc, go, rc, ro, sc_, so_)
    print("%s: max error / scale: colours %.3g, opacity logits %.3g" % (tag, ec, eo))
    assert ec <= TOL and eo <= TOL, (tag, ec, eo)
    for a, r in ((gc, rc), (go, ro)):
        if np.abs(r).max() > 0:
            assert np.abs(a - r).max() <= REL * np.abs(r).max(), tag
        else:
            assert not a.any(), tag
    return pre, rc, ro, sc_, so_


def _W(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).to(DEV)


@pytest.mark.parametrize("name", GRAD_SCENES)
def test_hip_gradients_meet_the_per_gaussian_bound_on_fixtures(tmp_path, name):
    gg = load_golden("grad_" + name)
    scene = _golden_scene(tmp_path, gg)
    W = torch.from_numpy(gg["W"]).to(DEV)
    frame, gc, go = _grads(scene, W, tile=int(gg["tile"]))
    sc = {k: gg[k] for k in ("points", "scales", "quaternions", "opacity", "width", "height")}
    _check(scene, sc, frame, W, int(gg["tile"]), gc, go, name)


# tile -> (width, height, n): at least two rendered tiles per axis (REF_CPU renders range(0, extent - tile, tile))
TILE_SCENES = {1: (24, 20, 120), 3: (40, 32, 200), 12: (64, 52, 900), 20: (84, 64, 400), 24: (80, 80, 400),
               32: (112, 100, 500), 64: (160, 140, 600)}


@pytest.mark.parametrize("tile", sorted(TILE_SCENES))
def test_tile_sizes_match_restatement(tmp_path, tile):
    """1 and 3 (a wave of 64 lanes, 1 and 9 live pixels), 12 (144 px), 20 (400 = 256 + 144: the second chunk partial),
    24 (576), 32 (1024: four chunks, each after the first adding to the slot) and 64 (4096: sixteen chunks)."""
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    w, h, n = TILE_SCENES[tile]
    sc = make_scene(n, w, h, seed=100 + tile)
    scene = _scene(tmp_path, sc)
    W = _W((w, h, 3), tile)
    frame, gc, go = _grads(scene, W, tile=tile)
    _, rc, _, _, _ = _check(scene, sc, frame, W, tile, gc, go, "tile %d" % tile)
    assert (np.abs(rc).sum(1) > 0).sum() >= n // 4


def test_faint_gaussians_keep_their_gradient(tmp_path):
    """Footprints of ~0.1 px (sigma_scale 0.07): many Gaussians have alpha < 2^-26 at every pixel centre of their
    tiles.  The forward skips such records (gsx_blend.hip), the reference does not; the backward must not skip them:
    their gradients are tiny next to the largest, so only the per-Gaussian bound sees them."""
    from intro_to_gaussian_splatting_amd.synthetic import make_scene
    from oracle import cpu_ref

    sc = make_scene(600, 64, 48, seed=23, sigma_scale=0.07)
    scene = _scene(tmp_path, sc)
    W = _W((64, 48, 3), 23)
    frame, gc, go = _grads(scene, W)
    pre, rc, ro, sc_, so_ = _check(scene, sc, frame, W, 16, gc, go, "faint")
    # how many Gaussians are faint on every pixel of every tile they are binned into, yet get a gradient
    amax = np.zeros(pre.order.shape[0])
    for x0 in cpu_ref.tile_origins(64, 16):
        for y0 in cpu_ref.tile_origins(48, 16):
            xs, ys = np.meshgrid(np.arange(x0, x0 + 16), np.arange(y0, y0 + 16), indexing="ij")
            px, py = xs.reshape(-1).astype(np.float32), ys.reshape(-1).astype(np.float32)
            op32 = (1.0 / (1.0 + np.exp(-np.asarray(pre.sigmoid_opacity, np.float64).reshape(-1)))).astype(np.float32)
            for k in cpu_ref.tile_list(pre, x0, y0, 16):
                a = backward_restatement._alpha32(pre.points_xy[k, 0], pre.points_xy[k, 1], pre.inverse_covariance_2d[k],
                                                  op32[k], px, py)
                amax[k] = max(amax[k], float(a.max()))
    faint = np.asarray(pre.order)[(amax > 0) & (amax < 2.0 ** -26)]
    print("faint: %d Gaussians below 2^-26 everywhere" % faint.size)
    assert faint.size >= 5
    # those whose gradient is a normal float32 number get one (below it: per_gaussian_error's SUBNORMAL floor)
    normal = faint[np.abs(rc[faint]).max(1) >= backward_restatement.SUBNORMAL]
    assert normal.size >= 5 and (np.abs(gc.cpu().numpy()[normal]).sum(1) > 0).all()


@pytest.mark.parametrize("tile,w,h", [(16, 96, 80), (32, 96, 96)])
def test_hw3_layout_gradients_equal_wh3(tmp_path, tile, w, h):
    """layout="hw3" (a (height, width, 3) frame: the other OutDesc stride pair) gives the gradients of wh3 with W
    transposed, bit for bit."""
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    sc = make_scene(500, w, h, seed=7)
    scene = _scene(tmp_path, sc)
    W = _W((w, h, 3), 9)
    f1, c1, o1 = _grads(scene, W, tile=tile)
    f2, c2, o2 = _grads(scene, W.permute(1, 0, 2).contiguous(), tile=tile, layout="hw3")
    assert f2.shape == (h, w, 3)
    assert torch.equal(f2.permute(1, 0, 2), f1)
    assert torch.equal(c1, c2) and torch.equal(o1, o2)
    _check(scene, sc, f1, W, tile, c1, o1, "hw3 tile %d" % tile)


def test_gaussians_off_the_graded_tiles_get_exact_zeros(tmp_path):
    """W non-zero on three tiles: every Gaussian on none of their lists gets exactly 0.0 (a slot that went to the
    wrong Gaussian would not be hidden by a tolerance); the others match the restatement."""
    from intro_to_gaussian_splatting_amd.synthetic import make_scene
    from oracle import cpu_ref

    sc = make_scene(3000, 128, 128, seed=12)
    scene = _scene(tmp_path, sc)
    rng = np.random.default_rng(12)
    tiles = [(16, 32), (64, 0), (96, 96)]
    Wn = np.zeros((128, 128, 3), np.float32)
    for x0, y0 in tiles:
        Wn[x0:x0 + 16, y0:y0 + 16] = rng.standard_normal((16, 16, 3))
    W = torch.from_numpy(Wn).to(DEV)
    frame, gc, go = _grads(scene, W)
    pre, rc, ro, _, _ = _check(scene, sc, frame, Wn, 16, gc, go, "three tiles", tiles=tiles)
    on = np.zeros(3000, bool)
    for x0, y0 in tiles:
        on[np.asarray(pre.order)[cpu_ref.tile_list(pre, x0, y0, 16)]] = True
    gc, go = gc.cpu().numpy(), go.cpu().numpy()
    assert on.sum() > 50 and (~on).sum() > 1000
    assert not gc[~on].any() and not go[~on].any()
    assert (np.abs(gc[on]).sum(1) > 0).sum() > 50


def test_gaussians_only_on_the_unrendered_last_tiles_get_exact_zeros(tmp_path):
    """REF_CPU never renders the last tile row and column (range(0, extent - tile, tile)): a Gaussian whose rectangle
    reaches only those gets exactly 0.0, with W non-zero there too."""
    from intro_to_gaussian_splatting_amd.synthetic import make_scene
    from oracle import cpu_ref

    sc = make_scene(2000, 96, 80, seed=21)
    scene = _scene(tmp_path, sc)
    W = _W((96, 80, 3), 21)
    frame, gc, go = _grads(scene, W)
    pre, rc, ro, _, _ = _check(scene, sc, frame, W, 16, gc, go, "last row / column")
    on = np.zeros(2000, bool)
    for x0 in cpu_ref.tile_origins(96, 16):
        for y0 in cpu_ref.tile_origins(80, 16):
            on[np.asarray(pre.order)[cpu_ref.tile_list(pre, x0, y0, 16)]] = True
    visible = np.zeros(2000, bool)
    visible[np.asarray(pre.order)] = True
    edge_only = visible & ~on
    print("last row / column: %d visible Gaussians on no rendered tile" % edge_only.sum())
    assert edge_only.sum() >= 10
    gc, go = gc.cpu().numpy(), go.cpu().numpy()
    assert not gc[~on].any() and not go[~on].any()
    assert not frame[80:].any() and not frame[:, 64:].any()


def test_no_visible_gaussian_gives_all_zero_gradients(tmp_path):
    from intro_to_gaussian_splatting_amd.synthetic import make_few_visible_scene

    sc = make_few_visible_scene(64, 48, 48, seed=5, visible=0)
    scene = _scene(tmp_path, sc)
    g = scene.gaussians
    g.colors.requires_grad_(True)
    g.opacity.requires_grad_(True)
    # poison whatever the caching allocator hands out next: the zeros must be written, not inherited
    torch.full((1 << 20,), float("nan"), device=DEV).sum()
    frame = scene.render_image_hip(1, tile_size=16)
    (frame * _W((48, 48, 3), 5)).sum().backward()
    assert not frame.any()
    assert g.colors.grad.shape == (64, 3) and g.opacity.grad.shape == (64, 1)
    assert not g.colors.grad.any() and not g.opacity.grad.any()
    assert torch.isfinite(g.colors.grad).all() and torch.isfinite(g.opacity.grad).all()


@pytest.mark.parametrize("n,visible", [(1, 1), (3, 3), (500, 1), (500, 3)])
def test_one_to_three_visible_gaussians_match_restatement(tmp_path, n, visible):
    """The row classes GSX_FLAG_ONE_VISIBLE / SMALL_BATCH (_ffi.visible_rows_flag): the backward re-derives the flag
    from the forward's visible count and must project the footprints like the forward did."""
    from intro_to_gaussian_splatting_amd.synthetic import make_few_visible_scene, make_scene

    seed = {(1, 1): 40, (3, 3): 40, (500, 1): 41, (500, 3): 43}[n, visible]     # every visible one on a rendered tile
    if n == visible:
        sc = make_scene(n, 48, 48, seed=seed)
    else:
        sc = make_few_visible_scene(n, 48, 48, seed=seed, visible=visible)
    scene = _scene(tmp_path, sc)
    W = _W((48, 48, 3), n + visible)
    st = {}
    g = scene.gaussians
    g.colors.requires_grad_(True)
    g.opacity.requires_grad_(True)
    frame = scene.render_image_hip(1, tile_size=16, stats=st)
    (frame * W).sum().backward()
    assert st["n_visible"] == visible
    gc, go = g.colors.grad, g.opacity.grad
    _, rc, ro, _, _ = _check(scene, sc, frame.detach(), W, 16, gc, go, "n=%d visible=%d" % (n, visible))
    assert (np.abs(rc).sum(1) > 0).sum() == visible
    with torch.no_grad():
        again = scene.render_image_hip(1, tile_size=16)
    assert torch.equal(again, frame.detach())


def _duplicated_scene(n_base, width, height, seed, copies=4, **kw):
    """make_scene with every Gaussian repeated `copies` times: the same point, scale and rotation (runs of equal
    depth, bit for bit), other colours and opacities per copy, so that the order inside a run shows in the frame."""
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    sc = make_scene(n_base, width, height, seed=seed, **kw)
    rs = np.random.RandomState(seed + 1)
    n = n_base * copies
    for k in ("points", "scales", "quaternions"):
        sc[k] = np.ascontiguousarray(np.repeat(sc[k], copies, axis=0))
    sc["colors_0_255"] = rs.uniform(0.0, 255.0, (n, 3)).astype(np.float32)
    sc["opacity"] = rs.normal(0.0, 2.0, (n, 1)).astype(np.float32)
    return sc


def _homogeneity(frame, W, colors, gc):
    """(sum_k <dL/dc_k, c_k>, <W, F>) in float64: equal up to rounding when the backward walks the forward's lists."""
    lhs = float((gc.double() * colors.detach().double()).sum())
    rhs = float((W.double() * frame.double()).sum())
    return lhs, rhs


def test_depth_ties_one_workgroup_sort(tmp_path):
    sc = _duplicated_scene(1500, 128, 128, seed=61)       # 6000 Gaussians <= 16 384: the one-workgroup depth sort
    scene = _scene(tmp_path, sc)
    W = _W((128, 128, 3), 61)
    frame, gc, go = _grads(scene, W)
    pre, _, _, _, _ = _check(scene, sc, frame, W, 16, gc, go, "ties n=6000")
    d = np.ascontiguousarray(pre.depths, np.float32).view(np.uint32)
    assert (d[1:] == d[:-1]).sum() >= 1000
    lhs, rhs = _homogeneity(frame, W, scene.gaussians.colors, gc)
    assert abs(lhs - rhs) <= 1e-5 * abs(rhs), (lhs, rhs)


def test_depth_ties_sampled_sort(tmp_path):
    """200 000 Gaussians (16 384 < n <= 1.5M: the sampled depth sort), runs of four equal depths; the restatement on
    eight tiles and the exact homogeneity of the frame in the colours over the whole frame."""
    sc = _duplicated_scene(50_000, 640, 480, seed=67)
    scene = _scene(tmp_path, sc)
    W = torch.from_numpy(np.random.default_rng(67).uniform(0.5, 1.5, (640, 480, 3)).astype(np.float32)).to(DEV)
    frame, gc, go = _grads(scene, W)
    lhs, rhs = _homogeneity(frame, W, scene.gaussians.colors, gc)
    print("ties n=200000: sum <grad c, c> = %.10g, <W, F> = %.10g" % (lhs, rhs))
    assert abs(lhs - rhs) <= 1e-5 * abs(rhs), (lhs, rhs)
    rng = np.random.default_rng(68)
    tiles = [(int(x) * 16, int(y) * 16) for x, y in zip(rng.integers(0, 39, 8), rng.integers(0, 29, 8))]
    Wn = np.zeros((640, 480, 3), np.float32)
    for x0, y0 in tiles:
        Wn[x0:x0 + 16, y0:y0 + 16] = rng.standard_normal((16, 16, 3))
    frame, gc, go = _grads(scene, torch.from_numpy(Wn).to(DEV))
    _check(scene, sc, frame, Wn, 16, gc, go, "ties n=200000, eight tiles", tiles=tiles)


def test_depth_ties_warm_forward_on_another_route(tmp_path):
    """More than 1.5M Gaussians, most of them culled: the first frame has no kept hint, so its depth sort takes LSD;
    the second (hints on) takes the 256-bucket route from its kept hint.  The backward passes no hint and always takes
    LSD.  Both routes must order equal depths by original index: the backward after the warm frame equals the one after
    the cold frame bit for bit, and the frame is homogeneous in the colours over the backward's lists."""
    n_base = 450_000
    sc = _duplicated_scene(n_base, 1920, 1080, seed=71, behind_fraction=0.6, sigma_scale=0.45)
    n = 4 * n_base
    assert n > KEPT_MAX_256
    scene = _scene(tmp_path, sc)
    g = scene.gaussians
    W = torch.from_numpy(np.random.default_rng(71).uniform(0.5, 1.5, (1920, 1080, 3)).astype(np.float32)).to(DEV)
    g.colors.requires_grad_(True)
    g.opacity.requires_grad_(True)
    out = []
    for frame_no in range(2):
        st = {}
        g.colors.grad = g.opacity.grad = None
        frame = scene.render_image_hip(1, tile_size=16, stats=st)
        (frame * W).sum().backward()
        out.append((frame.detach().clone(), g.colors.grad.clone(), g.opacity.grad.clone()))
        print("frame %d: visible %d kept %d pairs %d" % (frame_no, st["n_visible"], st["n_kept"], st["n_instances"]))
        assert 0 < st["n_kept"] <= KEPT_MAX_256
    assert scene._kept_hints, "the second frame had no kept hint"
    (f0, c0, o0), (f1, c1, o1) = out
    assert torch.equal(f0, f1)
    assert torch.equal(c0, c1) and torch.equal(o0, o1)
    lhs, rhs = _homogeneity(f1, W, g.colors, c1)
    print("ties n=%d: sum <grad c, c> = %.10g, <W, F> = %.10g" % (n, lhs, rhs))
    assert abs(lhs - rhs) <= 1e-5 * abs(rhs), (lhs, rhs)


def _fresh(tmp_path):
    gg = load_golden("grad_small_64x48_n300")
    return gg, _golden_scene(tmp_path, gg)


def test_grad_frame_arrives_in_any_layout(tmp_path):
    """dL/dframe as autograd hands it over -- expanded (stride 0), through a select, through a permute -- gives the
    gradients of the same W passed explicitly, bit for bit."""
    gg, scene = _fresh(tmp_path)
    g = scene.gaussians
    W = torch.from_numpy(gg["W"]).to(DEV)

    def run(loss_of, colors=True, opacity=True, times=1):
        g.colors.requires_grad_(colors)
        g.opacity.requires_grad_(opacity)
        g.colors.grad = g.opacity.grad = None
        frame = scene.render_image_hip(1, tile_size=16)
        loss = loss_of(frame)
        for k in range(times):
            loss.backward(retain_graph=k + 1 < times)
        return (g.colors.grad.clone() if colors else None), (g.opacity.grad.clone() if opacity else None)

    ones = torch.ones((64, 48, 3), device=DEV)
    chan1 = torch.zeros((64, 48, 3), device=DEV)
    chan1[..., 1] = 1.0
    for tag, loss_of, Wx in (("expanded", lambda f: f.sum(), ones),
                             ("select", lambda f: f[..., 1].sum(), chan1),
                             ("permute", lambda f: (f.permute(1, 0, 2) * W.permute(1, 0, 2)).sum(), W)):
        ref_c, ref_o = run(lambda f: (f * Wx).sum())
        c, o = run(loss_of)
        assert torch.equal(c, ref_c) and torch.equal(o, ref_o), tag
        assert ref_c.abs().max() > 0 and ref_o.abs().max() > 0, tag
    ref_c, ref_o = run(lambda f: (f * W).sum())
    c2, o2 = run(lambda f: (f * W).sum(), times=2)
    assert torch.equal(c2, 2 * ref_c) and torch.equal(o2, 2 * ref_o)
    _, o = run(lambda f: (f * W).sum(), colors=False)
    assert g.colors.grad is None and torch.equal(o, ref_o)
    c, _ = run(lambda f: (f * W).sum(), opacity=False)
    assert g.opacity.grad is None and torch.equal(c, ref_c)


# Central difference of L(l) = <W, frame(l)> along a random direction V of all opacity logits.  Calibrated on the CPU
# with c_oracle.render at C1 (2000 Gaussians, 256x256, W seed 3, V seeds 1..3) against the restatement's gradient:
# relative error 3.6e-3 .. 5.2e-3 at h = 0.1 (curvature), 1.9e-4 .. 5.1e-4 at h = 0.03 and 0.01, up to 2.3e-2 at
# h = 1e-3 (float32 frames and pixels that stop on the other side of the 1e-6 rule).  h = 0.01, tolerance 3e-3.
# Measured on an MI355X: 3.1e-4 at C1, 7.5e-4 at C3.
FD_H, FD_TOL = 0.01, 3e-3


@pytest.mark.parametrize("config", ["c1", "c3"])
def test_opacity_gradient_matches_central_difference(tmp_path, config):
    """(L(l + hV) - L(l - hV)) / 2h == <dL/dl, V> end to end on the GPU, without the restatement.  V ~ N(0, 1) over
    every logit; the perturbation actually applied (float32 logits) is used for the inner product."""
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    n, w, h = {"c1": (2000, 256, 256), "c3": (1_000_000, 1920, 1080)}[config]
    sc = make_scene(n, w, h, seed=0)
    scene = _scene(tmp_path, sc)
    W = _W((w, h, 3), 3)
    _, _, go = _grads(scene, W)
    g = scene.gaussians
    V = torch.from_numpy(np.random.default_rng(1).standard_normal((n, 1)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        g.colors.requires_grad_(False)
        g.opacity.requires_grad_(False)
        l0 = g.opacity.clone()
        lp, lm = l0 + FD_H * V, l0 - FD_H * V
        g.opacity.copy_(lp)
        Lp = float((scene.render_image_hip(1).double() * W.double()).sum())
        g.opacity.copy_(lm)
        Lm = float((scene.render_image_hip(1).double() * W.double()).sum())
        g.opacity.copy_(l0)
    fd = (Lp - Lm) / (2 * FD_H)
    dot = float((go.double() * (lp.double() - lm.double())).sum()) / (2 * FD_H)
    print("%s: finite difference %.9g, <grad, V> %.9g, relative %.3g" % (config, fd, dot, abs(fd - dot) / abs(dot)))
    assert abs(fd - dot) <= FD_TOL * abs(dot), (fd, dot)
