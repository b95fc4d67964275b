"""The screen-space densification statistic on the GPU: gsx_render_backward_screen through ``screen_statistics=True``,
gsx_density_accumulate_screen, gsx_density_plan_screen and ``DensityControl(statistic="screen")`` on top.

dL/d(NDC mean) is held Gaussian by Gaussian against the float64 restatement (tests/screen_gradient_restatement.py) and against
the reference's own autograd (tests/golden/screengrad_*.npz, tools/capture_screen_grad_golden.py).  Bounds
(test_screen_statistic_host.py): E_REF_SCREEN = 4.308e-08 is the worst per-Gaussian scaled error of the reference's own float32
gradient against the restatement over all fixtures; the kernel is held to 12 E_REF_SCREEN = 5.17e-07 against the restatement
and to 13 E_REF_SCREEN = 5.60e-07 against the fixtures.  Everything else is bits: the five older gradients are
gsx_render_backward_geometry's, the radius is stage 1's, the two density calls equal their float32 restatements.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

import density_restatement as dr
import geometry_backward_restatement as gbr
import screen_gradient_restatement as sgr
from test_density_host import RULES, case
from test_geometry_backward_host import fixture_inputs
from test_hip_backward import DEV, _golden_scene, _oracle_pre
from test_hip_density import (LR, TRAINED, Guarded, _apply, _dev, _lib, _perturbed_target, _plan, _quantile_knobs, _rules_struct,
                              _same, _stream)
from test_hip_density import _scene as _fit_scene
from test_hip_geometry_backward import GEOMETRY, _all_grads
from test_screen_statistic_host import BOUND_FIXTURE, BOUND_RESTATEMENT, edge_case, plan_case, restated

pytestmark = pytest.mark.gpu

# Worst error / scale of grad_means2d measured on an MI355X over SCENES:
#   against the restatement            1.613e-07  (wide_64x64_n400)      bound 12 E_REF_SCREEN = 5.17e-07
#   against the reference's autograd   1.882e-07  (tiny_48x48_n600)      bound 13 E_REF_SCREEN = 5.60e-07
# per scene, restatement | autograd: tile2 5.74e-09 | 9.52e-09, small 1.59e-08 | 2.66e-08, tiny 1.06e-07 | 1.88e-07, wide 1.61e-07 |
# 1.61e-07, cull 7.02e-08 | 6.65e-08, needle 6.39e-09 | 5.98e-09, rows1_n1 1.84e-09 | 2.16e-09, rows3_n500 1.74e-08 | 2.27e-08.
# Short fit (400 Gaussians, 64 x 64, 30 steps, one round after step 15): loss first 0.0669991, before the round 0.0110978, after it
# 0.0745072, last 0.0222149; rows 400 -> 406 (24 pruned, 15 cloned, 15 split); grad_threshold 0.00599 per NDC unit, prune_radius 26 px.
SCENES = ["tile2_40x32_n80", "small_64x48_n300", "tiny_48x48_n600", "wide_64x64_n400", "cull_96x80_n400", "needle_160x160_n110",
          "rows1_48x48_n1", "rows3_48x48_n500"]
FIVE = GEOMETRY + ("colors", "opacity")


def _screen_grads(scene, W, tile=16, only=None, **kw):
    """_all_grads through the screen entry: (frame, {name: gradient}, (image_idx, grad_means2d, screen_radius))."""
    scene.screen_statistics = None
    frame, grads = _all_grads(scene, W, tile=tile, only=only, screen_statistics=True, **kw)
    stat = scene.screen_statistics
    assert stat is not None and stat[0] == 1
    n = len(scene.gaussians)
    assert stat[1].shape == (n, 2) and stat[2].shape == (n,) and stat[1].dtype == stat[2].dtype == torch.float32
    return frame, grads, stat


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize("name", SCENES)
def test_screen_entry_keeps_the_five_gradients_and_matches_reference_and_restatement(tmp_path, name):
    gg, base = fixture_inputs(name)
    scene = _golden_scene(tmp_path, base)
    W = torch.from_numpy(base["W"]).to(DEV)
    tile = int(base["tile"])
    frame0, plain = _all_grads(scene, W, tile=tile)
    assert scene.screen_statistics is None              # the geometry entry leaves no statistic
    frame, grads, (_, g2d, radius) = _screen_grads(scene, W, tile=tile)
    assert torch.equal(_bits(frame0), _bits(frame))
    for k in FIVE:
        assert torch.equal(_bits(plain[k]), _bits(grads[k])), k
    # dL/d(NDC mean): the restatement on this frame, and the reference's own autograd
    pre_ref, n, w, h, _, _, _, _, ref = restated(name)
    sc = {k: base[k] for k in ("points", "scales", "quaternions", "opacity", "width", "height")}
    gn, scale = sgr.screen_gradient(_oracle_pre(scene, sc), n, frame.cpu().numpy(), base["W"], w, h, tile)
    got = g2d.cpu().numpy().astype(np.float64)
    e, ef = gbr.per_gaussian_error(got, gn, scale), gbr.per_gaussian_error(got, ref, scale)
    print("%s: grad_means2d: kernel vs restatement, max error / scale %.4g (bound %.3g); vs reference autograd %.4g (bound %.3g)"
          % (name, e, BOUND_RESTATEMENT, ef, BOUND_FIXTURE))
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    assert e <= BOUND_RESTATEMENT, (name, e)
    assert ef <= BOUND_FIXTURE, (name, ef)
    # the radius: stage 1's bits for every listed Gaussian, +0 for the rest, and the gradient is zero where the radius is
    want = sgr.screen_radius(pre_ref, n, sgr.listed(pre_ref, w, h, tile))
    assert np.array_equal(radius.cpu().numpy().view(np.uint32), want.view(np.uint32))
    dead = torch.from_numpy(want == 0).to(DEV)
    assert not _bits(g2d)[dead].any() and not _bits(radius)[dead].any()
    for k in GEOMETRY:
        assert not _bits(grads[k])[dead].any(), k


def test_radius_on_the_cull_scene_has_all_three_classes(tmp_path):
    name = "cull_96x80_n400"
    gg, base = fixture_inputs(name)
    fwd = load_golden(name)
    scene = _golden_scene(tmp_path, base)
    _, _, (_, g2d, radius) = _screen_grads(scene, torch.from_numpy(base["W"]).to(DEV), tile=int(base["tile"]))
    pre, n, w, h, tile = restated(name)[:5]
    on = sgr.listed(pre, w, h, tile)
    order = np.asarray(fwd["order"], np.int64)
    listed = np.zeros(n, bool)
    listed[order[on]] = True
    culled = ~fwd["in_view"]
    unlisted = ~culled & ~listed
    assert (int(culled.sum()), int(unlisted.sum()), int(listed.sum())) == (112, 44, 244)
    want = np.zeros(n, np.float32)
    want[order[on]] = fwd["pre_radius"].astype(np.float32)[on]
    got = radius.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and (got[listed] > 0).all()
    assert not got[culled | unlisted].view(np.uint32).any()
    assert not g2d.cpu().numpy()[culled | unlisted].view(np.uint32).any()


def test_a_visible_gaussian_on_no_list_gives_zeros_and_is_not_seen(tmp_path):
    fwd = load_golden("onevisible_48x48_n7")
    assert int(fwd["in_view"].sum()) == 1 and not fwd["image"].any()
    scene = _golden_scene(tmp_path, fwd)
    n = len(scene.gaussians)
    W = torch.ones((48, 48, 3), device=DEV)
    frame, grads, (_, g2d, radius) = _screen_grads(scene, W, tile=int(fwd["tile"]))
    assert not frame.any() and not _bits(g2d).any() and not _bits(radius).any()
    assert all(not _bits(grads[k]).any() for k in FIVE)
    _, lib = _lib()
    grad_sum, seen, radius_max = (torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, device=DEV))
    rc = lib.gsx_density_accumulate_screen(g2d.data_ptr(), radius.data_ptr(), n, grad_sum.data_ptr(), seen.data_ptr(),
                                           radius_max.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0 and not seen.any() and not grad_sum.any() and not radius_max.any()


def test_deterministic_follows_spatial_order_and_runs_whoever_requires_grad(tmp_path):
    from intro_to_gaussian_splatting_amd import GaussianScene

    gg = load_golden("grad_trainedlike_128x128_n3000")
    scene = _golden_scene(tmp_path, gg)
    W = torch.from_numpy(gg["W"]).to(DEV)
    _, a, sa = _screen_grads(scene, W)
    _, b, sb = _screen_grads(scene, W)
    _, c, sc = _screen_grads(scene, W, use_hints=False)
    assert sa[1] is not sb[1]                           # every such backward replaces the statistic
    for other in (sb, sc):
        assert torch.equal(_bits(sa[1]), _bits(other[1])) and torch.equal(_bits(sa[2]), _bits(other[2]))
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])) and torch.equal(_bits(a[k]), _bits(c[k])), k
    assert float(sa[1].abs().max()) > 0 and int((sa[2] > 0).sum()) > 1000 and int((sa[2] == 0).sum()) > 0
    # only the colours require grad: the screen entry still runs, the geometry gets no gradient
    _, d, sd = _screen_grads(scene, W, only=("colors",))
    assert all(d[k] is None for k in GEOMETRY + ("opacity",)) and torch.equal(_bits(d["colors"]), _bits(a["colors"]))
    assert torch.equal(_bits(sd[1]), _bits(sa[1])) and torch.equal(_bits(sd[2]), _bits(sa[2]))
    # no grad_fn, no statistic; geometry_gradients alone leaves none either
    scene.screen_statistics = None
    assert scene.render_image_hip(1, geometry_gradients=True, screen_statistics=True).grad_fn is None
    assert scene.screen_statistics is None
    with pytest.raises(ValueError, match="needs geometry_gradients=True"):
        scene.render_image_hip(1, screen_statistics=True)
    # a spatially ordered container: the permuted bits
    with torch.no_grad():
        ordered = scene.gaussians.spatially_ordered()
    _, e, se = _screen_grads(GaussianScene(str(tmp_path), ordered), W)
    oi = ordered.original_index.long()
    assert torch.equal(_bits(se[1]), _bits(sa[1][oi])) and torch.equal(_bits(se[2]), _bits(sa[2][oi]))
    for k in a:
        assert torch.equal(_bits(e[k]), _bits(a[k][oi])), k


def test_an_sh_scene_s_statistic_is_the_rgb_scene_s_of_the_evaluated_colours(tmp_path):
    from intro_to_gaussian_splatting_amd import GaussianScene
    from test_hip_sh_backward import _rgb_copy, _sh_scene

    scene, W = _sh_scene(tmp_path, 2)
    g = scene.gaussians
    with torch.no_grad():
        colors = scene._colors(1).clone()
    for name in GEOMETRY + ("opacity", "sh"):
        getattr(g, name).requires_grad_(True)
    (scene.render_image_hip(1, geometry_gradients=True, screen_statistics=True) * W).sum().backward()
    _, sh_g2d, sh_radius = scene.screen_statistics
    sh_points = g.points.grad.clone()
    rgb = GaussianScene(str(tmp_path), _rgb_copy(g, colors))
    _, rgb_grads, (_, g2d, radius) = _screen_grads(rgb, W)
    assert float(g2d.abs().max()) > 0
    assert torch.equal(_bits(sh_g2d), _bits(g2d)) and torch.equal(_bits(sh_radius), _bits(radius))
    assert not torch.equal(sh_points, rgb_grads["points"])          # the view direction's share reaches points.grad only


# ---- gsx_density_accumulate_screen
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_accumulate_screen_equals_the_restatement_bit_for_bit(n):
    _, lib = _lib()
    got = [Guarded(n), Guarded(n, 0, torch.int32), Guarded(n)]
    for t in got:
        t.view.zero_()
    want = (np.zeros(n, np.float32), np.zeros(n, np.uint32), np.zeros(n, np.float32))
    for call in range(3):
        g, r, s0, c0, m0 = edge_case(n, seed=call)
        if call == 0:           # the first call starts from a statistic that is not zero
            want = (s0, c0, m0)
            for t, a in zip(got, want):
                t.view.copy_(_dev(a.view(np.int32) if a.dtype == np.uint32 else a))
        grad, radius = Guarded(2 * n, call), Guarded(n, call)       # (later calls: bases off 16- and 8-byte alignment)
        grad.view.copy_(_dev(g).reshape(-1))
        radius.view.copy_(_dev(r))
        rc = lib.gsx_density_accumulate_screen(grad.view.data_ptr(), radius.view.data_ptr(), n, got[0].view.data_ptr(),
                                               got[1].view.data_ptr(), got[2].view.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.gsx_last_error()
        want = sgr.accumulate_screen(g, r, *want)
        for t, a in zip(got, want):
            assert np.array_equal(t.view.cpu().numpy().view(np.uint32), a.view(np.uint32)), (n, call)
            assert t.intact()
        assert grad.intact() and radius.intact()
    if n >= 4:                  # the edge rows were among them: a zero gradient counted, a NaN gradient added
        assert want[1][2] == edge_case(n, 0)[3][2] + 3 and np.isnan(want[0][3])


# ---- gsx_density_plan_screen
def _plan_screen(c, n, radius_max, prune_radius, r=RULES):
    """_plan of tests/test_hip_density.py through gsx_density_plan_screen (radius_max None: NULL)."""
    _, lib = _lib()
    need = lib.gsx_density_workspace_bytes(n)
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = ws[(-ws.data_ptr()) % 256:][:need]
    held = [_dev(c["grad_sum"]), _dev(c["seen"].view(np.int32)), _dev(c["scales"]), _dev(c["opacity"])]
    rm = None if radius_max is None else _dev(radius_max)
    counts = (ctypes.c_int64 * 4)(-1, -1, -1, -1)
    rules = _rules_struct(r)
    rc = lib.gsx_density_plan_screen(held[0].data_ptr(), held[1].data_ptr(), held[2].data_ptr(), held[3].data_ptr(),
                                     None if rm is None else rm.data_ptr(), prune_radius, n, ctypes.byref(rules), ws.data_ptr(), need,
                                     counts, _stream())
    assert rc == 0, lib.gsx_last_error()
    return ws, tuple(int(v) for v in counts)


@pytest.mark.parametrize("n", [1, 257, 1025, 5000])
def test_plan_screen_without_radii_is_the_plan_s_bytes_and_counts(n):
    c = case(n, "random", 2)
    ws0, counts0 = _plan(c, n)
    for prune_radius in (20.0, float("inf")):
        ws1, counts1 = _plan_screen(c, n, None, prune_radius)
        assert counts1 == counts0 and torch.equal(ws0, ws1)
    # and with radii that never exceed the threshold
    ws2, counts2 = _plan_screen(c, n, np.full(n, 20.0, np.float32), 20.0)
    assert counts2 == counts0 and torch.equal(ws0, ws2)


@pytest.mark.parametrize("n", [1, 257, 1025, 5000])
def test_plan_screen_gives_the_restatement_s_action_for_every_row(n):
    c, radius_max = plan_case(n, 4)
    action, prefix, want_counts = sgr.plan_screen(c["grad_sum"], c["seen"], c["scales"], c["opacity"], radius_max, 20.0, RULES)
    ws, counts = _plan_screen(c, n, radius_max, 20.0)
    assert counts == want_counts, (counts, want_counts)
    if n >= 257:
        base = dr.plan(c["grad_sum"], c["seen"], c["scales"], c["opacity"], RULES)[2]
        assert counts[1] > base[1] and (radius_max == 20.0).any() and np.isnan(radius_max).any()
    n_out = counts[0]
    if n_out == 0:
        return
    src = np.arange(3 * n, dtype=np.float32).reshape(n, 3)
    rc, dsts, rows = _apply(ws, n, n_out, [(3, dr.COPY)], [src], c["noise"], 0)       # the unchanged gsx_density_apply
    assert rc == 0, _lib()[1].gsx_last_error()
    row, _, _, want_rows = dr.source_rows(action, prefix, n_out)
    assert _same(rows.view.cpu().numpy(), want_rows) and rows.intact()
    assert _same(dsts[0].view.cpu().numpy().reshape(n_out, 3), src[row]) and dsts[0].intact()


# ---- DensityControl(statistic="screen")
def _fit_step(scene, opt, target):
    opt.zero_grad()
    loss = scene.photometric_loss(1, scene.render_image_hip(1, geometry_gradients=True, screen_statistics=True), target)
    loss.backward()
    return loss.detach()


def test_density_control_on_the_screen_statistic_end_to_end(tmp_path):
    from intro_to_gaussian_splatting_amd import DensityControl, GaussianAdam, GaussianScene, Gaussians

    scene = _fit_scene(tmp_path)
    g = scene.gaussians
    target = _perturbed_target(scene, 3)
    for k in TRAINED:
        getattr(g, k).requires_grad_(True)
    opt = GaussianAdam(g, lr=LR)
    dc = DensityControl(g, optimizer=opt, scene=scene, statistic="screen")
    n = len(g)
    cpu = lambda t: t.detach().cpu().numpy()  # noqa: E731
    with pytest.raises(ValueError, match="scene.screen_statistics is None"):
        dc.accumulate()
    want = (np.zeros(n, np.float32), np.zeros(n, np.uint32), np.zeros(n, np.float32))
    for _ in range(3):
        _fit_step(scene, opt, target)
        idx, g2d, radius = scene.screen_statistics
        assert idx == 1 and g2d.shape == (n, 2) and radius.shape == (n,)
        want = sgr.accumulate_screen(cpu(g2d), cpu(radius), *want)
        dc.accumulate()
        assert scene.screen_statistics is None              # consumed
        with pytest.raises(ValueError, match="scene.screen_statistics is None"):
            dc.accumulate()
        for got, w in zip((dc.grad_sum, dc.seen, dc.radius_max), want):
            assert np.array_equal(cpu(got).view(np.uint32), w.view(np.uint32))
        opt.step()
    assert 0 < int((dc.seen == 3).sum()) and float(dc.radius_max.max()) > 0
    # a row-count mismatch is refused
    scene.screen_statistics = (1, torch.zeros((n + 1, 2), device=DEV), torch.zeros(n + 1, device=DEV))
    with pytest.raises(ValueError, match="rows changed"):
        dc.accumulate()
    # knobs from the scene itself; the radius threshold is a value some Gaussians hold exactly (radii are whole pixels)
    _quantile_knobs(dc, g)
    dc.prune_radius = float(torch.quantile(dc.radius_max[dc.seen > 0], 0.9, interpolation="lower"))
    r = dr.rules(dc.grad_threshold, dc.dense_scale, dc.prune_logit, dc.prune_scale, dc.split_shrink)
    stat = (cpu(dc.grad_sum), cpu(dc.seen).view(np.uint32), cpu(g.scales), cpu(g.opacity))
    action, prefix, want_counts = sgr.plan_screen(*stat, cpu(dc.radius_max), dc.prune_radius, r)
    base_action = dr.plan(*stat, r)[0]
    by_radius = (action == dr.PRUNE) & (base_action != dr.PRUNE)
    assert by_radius.sum() > 0 and (cpu(dc.radius_max) == np.float32(dc.prune_radius)).any() and min(want_counts) > 0, want_counts
    seed = 5
    noise = cpu(torch.randn((n, 2, 3), generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV))
    roles = {"points": dr.POINTS, "scales": dr.SCALES, "quaternions": dr.QUATS}
    moments = [(key, k) for k in opt.names for key in ("exp_avg", "exp_avg_sq")]
    groups = [(cpu(getattr(g, k)), roles.get(k, dr.COPY)) for k in TRAINED] + [(cpu(getattr(opt, key)[k]), dr.ZERO_NEW) for key, k in moments]
    outs, source_row = dr.apply(groups, action, prefix, want_counts[0], noise, r["split_shrink"])
    before = {k: getattr(g, k).detach().clone() for k in TRAINED}
    before_m = {(key, k): getattr(opt, key)[k].clone() for key, k in moments}
    _fit_step(scene, opt, target)                           # a statistic nobody consumed: the round drops it
    opt.zero_grad()
    assert scene.screen_statistics is not None
    counts = dc.densify_and_prune(generator=torch.Generator(device=DEV).manual_seed(seed))
    assert tuple(counts[k] for k in ("n_out", "n_pruned", "n_cloned", "n_split")) == want_counts
    n_out = counts["n_out"]
    assert scene.screen_statistics is None and len(g) == n_out != n
    for t in (dc.grad_sum, dc.seen, dc.radius_max):
        assert t.shape == (n_out,) and not t.any()
    kept = torch.from_numpy(source_row >= 0).to(DEV)
    src = torch.from_numpy(np.where(source_row >= 0, source_row, 0)).to(DEV).long()
    assert not np.isin(np.flatnonzero(by_radius), source_row[source_row >= 0]).any()      # the rows the radius pruned are gone
    for k, w in zip(TRAINED, outs[:len(TRAINED)]):
        t = getattr(g, k)
        assert t.is_leaf and t.requires_grad and t.grad is None
        assert _same(cpu(t).reshape(n_out, -1), w), k
        assert torch.equal(_bits(t)[kept], _bits(before[k])[src[kept]]), k
    for (key, k), w in zip(moments, outs[len(TRAINED):]):
        m = getattr(opt, key)[k]
        assert _same(cpu(m).reshape(n_out, -1), w), (key, k)
        assert torch.equal(_bits(m)[kept], _bits(before_m[(key, k)])[src[kept]]) and not _bits(m)[~kept].any(), (key, k)
    # the frames after it are those of a fresh scene, and the next step runs on the new rows
    _fit_step(scene, opt, target)
    frame = scene.render_image_hip(1, geometry_gradients=True, screen_statistics=True).detach()
    dc.accumulate()
    opt.step()
    assert int(dc.seen.sum()) == int((dc.radius_max > 0).sum()) > 0
    fresh_g = Gaussians.from_arrays(g.points.detach().cpu(), g.colors.detach().cpu() * 256, g.scales.detach().cpu(),
                                    g.quaternions.detach().cpu(), g.opacity.detach().cpu(), device=DEV)
    assert torch.equal(fresh_g.colors, g.colors.detach())
    with torch.no_grad():
        fresh = GaussianScene(str(tmp_path), fresh_g).render_image_hip(1)
        assert torch.equal(_bits(fresh), _bits(scene.render_image_hip(1)))
    assert frame.shape == fresh.shape


def test_the_default_statistic_is_untouched_by_a_screen_backward(tmp_path):
    """statistic="points" (the default) reads points.grad as it always has, whether or not the frame left a screen statistic."""
    from intro_to_gaussian_splatting_amd import DensityControl, GaussianAdam

    sums = []
    for screen in (False, True):
        scene = _fit_scene(tmp_path)
        g = scene.gaussians
        target = _perturbed_target(scene, 3)
        for k in TRAINED:
            getattr(g, k).requires_grad_(True)
        opt = GaussianAdam(g, lr=LR)
        dc = DensityControl(g, optimizer=opt, scene=scene)
        assert dc.statistic == "points" and dc.radius_max is None
        opt.zero_grad()
        scene.photometric_loss(1, scene.render_image_hip(1, geometry_gradients=True, screen_statistics=screen), target).backward()
        dc.accumulate()
        assert (scene.screen_statistics is not None) == screen
        sums.append((dc.grad_sum.clone(), dc.seen.clone()))
    assert torch.equal(_bits(sums[0][0]), _bits(sums[1][0])) and torch.equal(sums[0][1], sums[1][1])


def test_a_short_fit_on_the_screen_statistic_with_one_round_in_the_middle(tmp_path):
    from intro_to_gaussian_splatting_amd import DensityControl, GaussianAdam

    scene = _fit_scene(tmp_path)
    g = scene.gaussians
    target = _perturbed_target(scene, 4)
    for k in TRAINED:
        getattr(g, k).requires_grad_(True)
    opt = GaussianAdam(g, lr=LR, skip_zero_rows=True)
    dc = DensityControl(g, optimizer=opt, scene=scene, statistic="screen")
    losses, rows = [], [len(g)]
    for step in range(30):
        losses.append(_fit_step(scene, opt, target))
        dc.accumulate()
        opt.step()
        if step == 14:
            _quantile_knobs(dc, g)
            dc.prune_radius = float(torch.quantile(dc.radius_max[dc.seen > 0], 0.97, interpolation="lower"))
            counts = dc.densify_and_prune(generator=torch.Generator(device=DEV).manual_seed(2))
            rows.append(len(g))
    losses = [float(v) for v in losses]
    print("short fit, screen statistic: loss first %.6g, before the round %.6g, after it %.6g, last %.6g; rows %d -> %d %s; "
          "grad_threshold %.3g per NDC unit, prune_radius %g px"
          % (losses[0], losses[14], losses[15], losses[-1], rows[0], rows[1], counts, dc.grad_threshold, dc.prune_radius))
    assert all(np.isfinite(losses)) and rows[1] != rows[0] and len(g) == rows[1] == counts["n_out"]
    assert losses[-1] < losses[0]
    assert opt.step_count == 30 and bool((g.scales > 0).all())
