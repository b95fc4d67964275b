"""The absolute screen statistic on the GPU: gsx_render_backward_screen_abs through ``screen_statistics="abs"``,
``DensityControl(statistic="screen_abs")`` and ``Trainer(statistic="screen_abs")`` on top.

grad_means2d_abs is held Gaussian by Gaussian against the float64 restatement (tests/abs_gradient_restatement.py) and, where a
fixture exists, against the reference's own per-pixel autograd (tests/golden/absgrad_*.npz, tools/capture_abs_grad_golden.py).
Bounds (test_abs_statistic_host.py): E_REF_ABS is the worst per-Gaussian scaled error of the reference's own float32 terms
against the restatement over all fixtures; the kernel is held to 12 E_REF_ABS against the restatement and to 13 E_REF_ABS
against the fixtures, the ratios the merged screen test grants.  Everything else is bits: the seven older outputs are
gsx_render_backward_screen's, and the density call on the absolute array equals its float32 restatement.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

import abs_gradient_restatement as agr
import geometry_backward_restatement as gbr
import screen_gradient_restatement as sgr
from test_abs_statistic_host import ABS_SCENES, BOUND_FIXTURE, BOUND_RESTATEMENT, reference_abs
from test_geometry_backward_host import GEOM_SCENES, fixture_inputs
from test_hip_backward import DEV, _golden_scene, _oracle_pre
from test_hip_density import LR, TRAINED, Guarded, _perturbed_target, _quantile_knobs
from test_hip_density import _scene as _fit_scene
from test_hip_geometry_backward import GEOMETRY, _all_grads
from test_hip_screen_statistic import FIVE, _bits, _screen_grads
from test_screen_statistic_host import restated

pytestmark = pytest.mark.gpu

# Worst error / scale of grad_means2d_abs measured on an MI355X over GEOM_SCENES:
#   against the restatement            1.683e-07  (wide_64x64_n400)      bound 12 E_REF_ABS = 3.53e-07
#   against the reference's autograd   5.003e-08  (cull_96x80_n400)      bound 13 E_REF_ABS = 3.82e-07
# per scene, restatement | autograd (- : no fixture): tile2 6.97e-09 | 7.31e-09, small_64x48 1.75e-08 | 1.71e-08, small_80x64_tile8
# 3.28e-08 | -, tile12_dense 1.49e-08 | -, tile20 5.98e-09 | 4.82e-08, tile32 2.51e-08 | -, needle 2.92e-09 | -, tiny 1.21e-07 | -,
# wide 1.68e-07 | -, cull 5.88e-08 | 5.00e-08, rows1_n1 2.70e-09 | 4.13e-09, rows3_n3 4.69e-09 | 5.10e-09, rows1_n500 3.49e-09 | -,
# rows3_n500 1.52e-08 | 1.26e-08.  Relative to the absolute value itself the worst Gaussian of a scene is off by 7e-08 .. 4e-06 on
# ten scenes; on tile12_dense (1.3e-03), wide (1.4e-02) and tiny (1.3e-01) it is a Gaussian whose own absolute value is a
# small fraction of its error scale -- faint behind opaque neighbours --, which is what the scale is for.
# Short fit (400 Gaussians, 64 x 64, 30 steps, one round after step 15): loss first 0.0669991, before the round 0.0110978, after it
# 0.0829488, last 0.0247494; rows 400 -> 406 (24 pruned, 15 cloned, 15 split); grad_threshold 0.0191 per NDC unit (the signed
# statistic's quantile on the same fit: 0.00599), prune_radius 26 px.


def _abs_grads(scene, W, tile=16, only=None, **kw):
    """_all_grads through the abs entry: (frame, {name: gradient}, (image_idx, grad_means2d, screen_radius, grad_means2d_abs))."""
    scene.screen_statistics = None
    frame, grads = _all_grads(scene, W, tile=tile, only=only, screen_statistics="abs", **kw)
    stat = scene.screen_statistics
    assert stat is not None and len(stat) == 4 and stat[0] == 1
    n = len(scene.gaussians)
    assert stat[1].shape == stat[3].shape == (n, 2) and stat[2].shape == (n,)
    assert stat[1].dtype == stat[2].dtype == stat[3].dtype == torch.float32 and stat[3].is_contiguous()
    return frame, grads, stat


@pytest.mark.parametrize("name", GEOM_SCENES)
def test_abs_entry_keeps_the_screen_entry_s_bits_and_matches_restatement_and_reference(tmp_path, name):
    gg, base = fixture_inputs(name)
    scene = _golden_scene(tmp_path, base)
    W = torch.from_numpy(base["W"]).to(DEV)
    tile = int(base["tile"])
    frame0, plain, (_, g2d0, radius0) = _screen_grads(scene, W, tile=tile)
    frame, grads, (_, g2d, radius, gabs) = _abs_grads(scene, W, tile=tile)
    assert torch.equal(_bits(frame0), _bits(frame))
    for k in FIVE:
        assert torch.equal(_bits(plain[k]), _bits(grads[k])), k
    assert torch.equal(_bits(g2d0), _bits(g2d)) and torch.equal(_bits(radius0), _bits(radius))
    # the absolute statistic: the restatement on this frame, and the reference's own per-pixel autograd
    n, w, h = restated(name)[1:4]
    sc = {k: base[k] for k in ("points", "scales", "quaternions", "opacity", "width", "height")}
    want, signed, scale = agr.abs_gradient(_oracle_pre(scene, sc), n, frame.cpu().numpy(), base["W"], w, h, tile, with_scale=True)
    got = gabs.cpu().numpy().astype(np.float64)
    e = gbr.per_gaussian_error(got, want, scale)
    ef = gbr.per_gaussian_error(got, reference_abs(name), scale) if name in ABS_SCENES else float("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(want > 0, np.abs(got - want) / want, 0.0).max()
    print("%s: grad_means2d_abs: kernel vs restatement, max error / scale %.4g (bound %.3g), relative to the value %.3g; "
          "vs reference autograd %.4g (bound %.3g)" % (name, e, BOUND_RESTATEMENT, rel, ef, BOUND_FIXTURE))
    assert np.isfinite(got).all() and got.max() > 0 and (got >= 0).all()
    assert e <= BOUND_RESTATEMENT, (name, e)
    if name in ABS_SCENES:
        assert ef <= BOUND_FIXTURE, (name, ef)
    # it bounds the signed statistic the same call wrote, up to the rounding the bound above grants
    slack = BOUND_RESTATEMENT * scale[:, None]
    assert (got + slack >= np.abs(g2d.cpu().numpy().astype(np.float64)) - slack).all()
    # exact +0 wherever the frame listed the Gaussian on no tile
    dead = radius == 0
    assert not _bits(gabs)[dead].any() and (name != "cull_96x80_n400" or int(dead.sum()) == 156)


def test_deterministic_with_and_without_hints_and_follows_spatial_order(tmp_path):
    from intro_to_gaussian_splatting_amd import GaussianScene

    gg = load_golden("grad_trainedlike_128x128_n3000")
    scene = _golden_scene(tmp_path, gg)
    W = torch.from_numpy(gg["W"]).to(DEV)
    _, a, sa = _abs_grads(scene, W)
    _, b, sb = _abs_grads(scene, W)
    _, c, sc = _abs_grads(scene, W, use_hints=False)
    assert sa[3] is not sb[3]
    for other in (sb, sc):
        assert all(torch.equal(_bits(sa[i]), _bits(other[i])) for i in (1, 2, 3))
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])) and torch.equal(_bits(a[k]), _bits(c[k])), k
    assert float(sa[3].max()) > 0 and int((sa[3].sum(1) > 0).sum()) > 1000 and int((sa[2] == 0).sum()) > 0
    # abs >= |signed| up to float32 summation: at most 128 x 128 terms, each sum within 16384 x 2^-24 of its absolute sum
    assert bool((sa[3] * (1 + 2e-3) >= sa[1].abs()).all())
    # only the colours require grad: the abs entry still runs
    _, d, sd = _abs_grads(scene, W, only=("colors",))
    assert all(d[k] is None for k in GEOMETRY + ("opacity",)) and torch.equal(_bits(sd[3]), _bits(sa[3]))
    # no grad_fn, no statistic
    scene.screen_statistics = None
    assert scene.render_image_hip(1, geometry_gradients=True, screen_statistics="abs").grad_fn is None
    assert scene.screen_statistics is None
    # a spatially ordered container: the permuted bits
    with torch.no_grad():
        ordered = scene.gaussians.spatially_ordered()
    _, e, se = _abs_grads(GaussianScene(str(tmp_path), ordered), W)
    oi = ordered.original_index.long()
    assert all(torch.equal(_bits(se[i]), _bits(sa[i][oi])) for i in (1, 2, 3))
    for k in a:
        assert torch.equal(_bits(e[k]), _bits(a[k][oi])), k


@pytest.mark.parametrize("n,w,h,tile", [(300, 64, 48, 16), (80, 40, 32, 2), (300, 64, 64, 20), (1, 48, 48, 16)])
def test_the_entry_stays_between_guarded_margins(tmp_path, n, w, h, tile):
    """A direct C call at exactly the workspace size, every array between two 64-element sentinel margins."""
    from intro_to_gaussian_splatting_amd import _ffi
    from intro_to_gaussian_splatting_amd.synthetic import make_scene
    from test_hip_depth import _W
    from test_hip_depth import _scene as _made_scene

    lib = _ffi.load()
    scene = _made_scene(tmp_path, make_scene(n, w, h, seed=40 if n == 1 else 3))
    st = {}
    with torch.no_grad():
        frame = scene.render_image_hip(1, tile_size=tile, stats=st)
    dev, nn, tensors = scene._inputs(1)
    cam = scene.images[1].gsx_camera()
    params, _ = scene._frame_params(dev, n, "wh3", "ref_cpu")
    params.flags |= _ffi.rows_flag(n, int(st["n_visible"]))
    cap = int(st["n_instances"]) + 1
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    need = int(lib.gsx_backward_geometry_workspace_bytes(n, w, h, tile, cap))
    assert need > 0 and need % 256 == 0
    results = []
    for entry, widths in ((lib.gsx_render_backward_screen_abs, (3, 1, 3, 3, 4, 2, 1, 2)), (lib.gsx_render_backward_screen, (3, 1, 3, 3, 4, 2, 1))):
        outs = [Guarded(n * k) for k in widths]
        gimg, ws = Guarded(w * h * 3), Guarded(need // 4)
        assert ws.view.data_ptr() % 256 == 0
        gimg.view.copy_(_W((w * h * 3,), 1))
        rc = entry(ctypes.byref(cam), *[t.data_ptr() for t in tensors], n, tile, frame.data_ptr(), gimg.view.data_ptr(),
                   *[o.view.data_ptr() for o in outs], ctypes.byref(params), ws.view.data_ptr(), need, stream)
        torch.cuda.synchronize()
        assert rc == 0, lib.gsx_last_error()
        assert ws.intact() and gimg.intact() and all(o.intact() for o in outs), "a write outside an array"
        assert all(torch.isfinite(o.view).all() for o in outs)
        results.append([o.view.clone() for o in outs])
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(results[0], results[1]))        # the seven older outputs
    assert float(results[0][7].max()) > 0 and float(results[0][7].min()) >= 0


def test_an_sh_scene_s_abs_statistic_is_the_rgb_scene_s_of_the_evaluated_colours(tmp_path):
    from intro_to_gaussian_splatting_amd import GaussianScene
    from test_hip_sh_backward import _rgb_copy, _sh_scene

    scene, W = _sh_scene(tmp_path, 2)
    g = scene.gaussians
    with torch.no_grad():
        colors = scene._colors(1).clone()
    for name in GEOMETRY + ("opacity", "sh"):
        getattr(g, name).requires_grad_(True)
    (scene.render_image_hip(1, geometry_gradients=True, screen_statistics="abs") * W).sum().backward()
    _, sh_g2d, sh_radius, sh_abs = scene.screen_statistics
    rgb = GaussianScene(str(tmp_path), _rgb_copy(g, colors))
    _, _, (_, g2d, radius, gabs) = _abs_grads(rgb, W)
    assert float(gabs.max()) > 0
    assert torch.equal(_bits(sh_abs), _bits(gabs)) and torch.equal(_bits(sh_g2d), _bits(g2d)) and torch.equal(_bits(sh_radius), _bits(radius))


# ---- DensityControl(statistic="screen_abs")
def _fit_step(scene, opt, target, mode="abs"):
    opt.zero_grad()
    loss = scene.photometric_loss(1, scene.render_image_hip(1, geometry_gradients=True, screen_statistics=mode), target)
    loss.backward()
    return loss.detach()


def _trained(tmp_path, seed):
    from intro_to_gaussian_splatting_amd import GaussianAdam

    tmp_path.mkdir(exist_ok=True)
    scene = _fit_scene(tmp_path)
    g = scene.gaussians
    target = _perturbed_target(scene, seed)
    for k in TRAINED:
        getattr(g, k).requires_grad_(True)
    return scene, g, target, GaussianAdam(g, lr=LR, skip_zero_rows=True)


def test_density_control_accumulates_the_abs_array_and_screen_is_unchanged(tmp_path):
    from intro_to_gaussian_splatting_amd import DensityControl

    cpu = lambda t: t.detach().cpu().numpy()  # noqa: E731
    scene, g, target, opt = _trained(tmp_path / "abs", 3)
    dc = DensityControl(g, optimizer=opt, scene=scene, statistic="screen_abs")
    n = len(g)
    assert dc.radius_max is not None
    with pytest.raises(ValueError, match="scene.screen_statistics is None: render with .*screen_statistics='abs'"):
        dc.accumulate()
    _fit_step(scene, opt, target, mode=True)            # a 3-tuple: refused, and says how to render
    with pytest.raises(ValueError, match="needs frames rendered with screen_statistics='abs'"):
        dc.accumulate()
    assert scene.screen_statistics is not None and not dc.seen.any()
    # "screen" on the same scene, fed 3-tuples in one run and 4-tuples in the other: the same statistic, bit for bit
    scene_s, g_s, target_s, opt_s = _trained(tmp_path / "screen", 3)
    dc_s = DensityControl(g_s, optimizer=opt_s, scene=scene_s, statistic="screen")
    want = (np.zeros(n, np.float32), np.zeros(n, np.uint32), np.zeros(n, np.float32))
    want_s = tuple(a.copy() for a in want)
    for step in range(3):
        _fit_step(scene, opt, target)
        idx, g2d, radius, gabs = scene.screen_statistics
        assert idx == 1 and gabs.shape == (n, 2) and radius.shape == (n,)
        want = sgr.accumulate_screen(cpu(gabs), cpu(radius), *want)
        want_s = sgr.accumulate_screen(cpu(g2d), cpu(radius), *want_s)
        dc.accumulate()
        assert scene.screen_statistics is None              # consumed
        _fit_step(scene_s, opt_s, target_s, mode="abs" if step % 2 else True)
        assert len(scene_s.screen_statistics) == (4 if step % 2 else 3)
        dc_s.accumulate()
        assert scene_s.screen_statistics is None
        for got, w in zip((dc.grad_sum, dc.seen, dc.radius_max), want):
            assert np.array_equal(cpu(got).view(np.uint32), w.view(np.uint32))
        for got, w in zip((dc_s.grad_sum, dc_s.seen, dc_s.radius_max), want_s):
            assert np.array_equal(cpu(got).view(np.uint32), w.view(np.uint32))
        opt.step()
        opt_s.step()
    assert 0 < int((dc.seen == 3).sum()) and float(dc.radius_max.max()) > 0
    assert torch.equal(dc.seen, dc_s.seen) and torch.equal(_bits(dc.radius_max), _bits(dc_s.radius_max))
    seen = dc.seen > 0
    # never below the signed statistic (up to float32 summation over at most 64 x 64 pixels), and above it on the whole
    assert bool((dc.grad_sum[seen] * (1 + 1e-3) >= dc_s.grad_sum[seen]).all())
    assert float(dc.grad_sum.sum()) > 1.01 * float(dc_s.grad_sum.sum())
    for k in TRAINED:                                       # and the parameters went the same way: the gradients are the same bits
        assert torch.equal(_bits(getattr(g, k)), _bits(getattr(g_s, k))), k


def test_a_short_fit_on_the_abs_statistic_with_one_round_in_the_middle(tmp_path):
    from intro_to_gaussian_splatting_amd import DensityControl

    scene, g, target, opt = _trained(tmp_path, 4)
    dc = DensityControl(g, optimizer=opt, scene=scene, statistic="screen_abs")
    losses, rows = [], [len(g)]
    for step in range(30):
        losses.append(_fit_step(scene, opt, target))
        dc.accumulate()
        opt.step()
        if step == 14:
            before = g.points.detach().clone()
            _quantile_knobs(dc, g)
            dc.prune_radius = float(torch.quantile(dc.radius_max[dc.seen > 0], 0.97, interpolation="lower"))
            counts = dc.densify_and_prune(generator=torch.Generator(device=DEV).manual_seed(2))
            rows.append(len(g))
    losses = [float(v) for v in losses]
    print("short fit, abs statistic: loss first %.6g, before the round %.6g, after it %.6g, last %.6g; rows %d -> %d %s; "
          "grad_threshold %.3g per NDC unit, prune_radius %g px"
          % (losses[0], losses[14], losses[15], losses[-1], rows[0], rows[1], counts, dc.grad_threshold, dc.prune_radius))
    assert all(np.isfinite(losses)) and rows[1] != rows[0] and len(g) == rows[1] == counts["n_out"]
    assert counts["n_cloned"] + counts["n_split"] > 0 and before.shape != g.points.shape
    assert losses[-1] < losses[0]
    assert opt.step_count == 30 and bool((g.scales > 0).all()) and all(bool(torch.isfinite(getattr(g, k)).all()) for k in TRAINED)


def test_trainer_on_the_abs_statistic_is_the_composition_written_out(tmp_path):
    from intro_to_gaussian_splatting_amd import DensityControl, GaussianAdam, Trainer
    from test_hip_depth import DENSITY, _state
    from test_hip_depth import LR as LR_FIT
    from test_hip_depth import _fit_scene as _depth_fit_scene

    steps, seed = 6, 5
    periods = dict(sh_degree_every=None, densify_every=4, opacity_reset_every=None, densify_from=0, densify_until=100)
    scene, targets, _ = _depth_fit_scene(tmp_path / "a", 1)
    trainer = Trainer(scene, targets, lr=LR_FIT, lambda_dssim=0.2, tile_size=16, statistic="screen_abs", density=DENSITY, seed=seed,
                      **periods)
    assert trainer.density.statistic == "screen_abs"
    seen = []
    trainer.fit(steps, callback=lambda t, losses, idx: seen.append((losses, idx, len(t.gaussians))))
    assert scene.screen_statistics is None

    scene2, targets2, _ = _depth_fit_scene(tmp_path / "b", 1)
    g = scene2.gaussians
    for name in LR_FIT:
        getattr(g, name).requires_grad_(True)
    opt = GaussianAdam(g, lr=LR_FIT)
    dc = DensityControl(g, optimizer=opt, scene=scene2, statistic="screen_abs", **DENSITY)
    split = torch.Generator(device=DEV).manual_seed(seed)
    by_hand = []
    for s in range(1, steps + 1):
        terms = {}
        frame = scene2.render_image_hip(1, tile_size=16, geometry_gradients=True, screen_statistics="abs")
        loss = scene2.photometric_loss(1, frame, targets2[1], tile_size=16, lambda_dssim=0.2, terms=terms)
        loss.backward()
        dc.accumulate()
        opt.step()
        opt.zero_grad()
        if s % 4 == 0:
            dc.densify_and_prune(generator=split)
        by_hand.append((torch.stack((loss.detach(), terms["l1"], terms["ssim"])), 1, len(g)))
    print("rows per step", [n for _, _, n in seen])
    assert [v[1:] for v in seen] == [v[1:] for v in by_hand]
    assert all(torch.equal(_bits(a[0]), _bits(b[0])) for a, b in zip(seen, by_hand))
    got, want = _state(trainer.gaussians, trainer.opt), _state(g, opt)
    for key in want:
        assert torch.equal(_bits(got[key]), _bits(want[key])), key
    assert trainer.opt.step_count == opt.step_count == steps

    # statistic="screen" on the same scene: the step it always was
    scene3, targets3, _ = _depth_fit_scene(tmp_path / "c", 1)
    first = Trainer(scene3, targets3, lr=LR_FIT, lambda_dssim=0.2, tile_size=16, statistic="screen", density=DENSITY, seed=seed,
                    **periods).step()[0]
    assert scene3.screen_statistics is None
    assert torch.equal(_bits(first), _bits(by_hand[0][0]))         # the first step's loss does not depend on the statistic
