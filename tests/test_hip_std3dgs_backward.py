"""Gradients of the std_3dgs frame on the GPU (gsx_render_backward_std through ``render_image_hip(semantics="std_3dgs")``),
held Gaussian by Gaussian to the float64 restatement (tests/std3dgs_backward_restatement.py) with dL/dframe = a fixed seeded
random image times the restatement's gradient mask (zero on the pixels whose decisions float32 could flip).

Bounds (tests/test_std3dgs_backward_host.py): BOUND = 12 E_REF per output array, E_REF the float32 mirror's own error against
float64 in the restatement's per-Gaussian norm.  The cases are the issue's seven of STD_CASES and that file's off-axis case.
All of them have fx = fy; unequal focal lengths and far poses are in tests/test_hip_camera_cases.py (STD_CAMERA_CASES).

Measured on an MI355X, kernel vs restatement, worst error / scale per case (tight rectangles; published_rects=True gives the
same figures to the last printed digit except scales: 2.57e-09 and 2.06e-09 in the two cases marked *):
  case                      colors     opacity    points     scales      quaternions  means2d
  stack_opaque_16x16        2.78e-08   0          1.28e-10   2.67e-10    0            4.01e-10
  stack_half_16x16          1.68e-08   2.68e-10   9.52e-11   9.07e-11    0            2.51e-10
  ring_40x24                1.64e-08   2.66e-09   5.78e-09   1.15e-09    0            6.74e-09
  random_130x70_n1500_t8    6.45e-08   1.75e-08   8.28e-09   2.86e-09 *  2.97e-10     1.78e-08
  random_64x64_n800_t2      8.50e-08   1.62e-08   3.92e-09   1.60e-09 *  1.31e-10     1.02e-08
  random_96x80_n1000_t32    1.62e-07   1.48e-08   4.50e-09   1.93e-09    1.08e-10     1.16e-08
  dense_96x96               6.70e-07   1.55e-08   1.73e-09   1.34e-09    1.47e-10     6.41e-09
  offaxis_48x32_n151        1.40e-07   7.93e-09   9.94e-10   1.04e-09    3.11e-11     4.07e-09
  BOUND = 12 E_REF          7.95e-06   1.91e-07   1.72e-07   7.37e-08    3.40e-09     3.12e-07
(the stacks and the ring hold identity quaternions and isotropic scales: their quaternion gradient is an exact zero.)

Deliberately wrong kernels, tried in scratch builds (not kept); per case, the arrays that leave the bound and by how much
(error / BOUND):
  a clamped pair given an opacity / geometry share (u = dL/dalpha alpha whatever the clamp):
      caught by stack_opaque_16x16 (points 26, scales 53, means2d 27), random_130x70_n1500_t8 (opacity 7100, points 225),
      dense_96x96 (opacity 2900, means2d 138), offaxis_48x32_n151 (opacity 12); the cases without clamped pairs pass.
  F taken without T_fin * bg (the backward handed the frame rendered over black):
      caught by every case with a coloured background under a gradient-carrying pair -- ring_40x24 (opacity 1.5e5), the
      random cases (opacity 1.9e5 .. 3.1e5), offaxis (3.3e4), dense_96x96 (351), stack_opaque_16x16 (means2d 78);
      stack_half_16x16, whose background is black, passes.
  the stopping record accumulated:
      caught by stack_opaque_16x16 (colors 315), stack_half_16x16 (colors 217), random_64x64_n800_t2 (colors 13),
      offaxis_48x32_n151 (opacity 12) and dense_96x96 (every array, by a factor beyond printing);
      ring_40x24 and the two other random cases, where no pixel stops, pass.
"""
import ctypes

import numpy as np
import pytest
import torch

import std3dgs_backward_restatement as sbr
from test_hip_backward import DEV, _scene
from test_std3dgs_backward_host import BOUND, backward_case

pytestmark = pytest.mark.gpu

GPU_CASES = ["stack_opaque_16x16", "stack_half_16x16", "ring_40x24", "random_130x70_n1500_t8", "random_64x64_n800_t2",
             "random_96x80_n1000_t32", "dense_96x96", "offaxis_48x32_n151"]
KEYS = ("colors", "opacity", "points", "scales", "quaternions", "means2d")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _std_scene(tmp_path, name):
    case = backward_case(name)
    return case, _scene(tmp_path, case["sc"], colors=case["colors"])


def _forward(scene, case, layout="hw3", **kw):
    st = {}
    with torch.no_grad():
        frame = scene.render_image_hip(1, tile_size=case["tile"], layout=layout, semantics="std_3dgs", background=case["bg"],
                                       stats=st, **kw)
    return frame, st


def _backward(scene, case, frame, st, gf, geometry=True, screen=True, layout="hw3", published=False):
    return scene._render_backward(1, case["tile"], layout, frame, gf, st["n_instances"], st["n_visible"], geometry=geometry,
                                  screen=screen, std=(case["bg"], published))


def _errors(case, outs):
    ref = case["ref"]
    got = dict(zip(("colors", "opacity", "points", "scales", "quaternions", "means2d"), (o.cpu().numpy() for o in outs[:6])))
    for k, v in got.items():
        assert np.isfinite(v).all(), k
    return {k: sbr.per_gaussian_error(got[k], ref.arrays[k], ref.scales[k]) for k in KEYS}


@pytest.mark.parametrize("name", GPU_CASES)
def test_case_matches_the_restatement(tmp_path, name):
    case, scene = _std_scene(tmp_path, name)
    gf = torch.from_numpy(case["g"]).to(DEV)
    frame, st = _forward(scene, case)
    outs = _backward(scene, case, frame, st, gf)
    assert len(outs) == 7
    err = _errors(case, outs)
    print("%s: kernel vs restatement, max error / scale: %s" % (name, ", ".join("%s %.3g (bound %.3g)" % (k, err[k], BOUND[k])
                                                                                 for k in KEYS)))
    # the radius is the stage-1 row's wherever the frame listed the Gaussian, 0 elsewhere; whoever has gradient is listed
    radius, rows = outs[6].cpu().numpy().reshape(-1), case["rows"]
    listed = radius > 0
    assert listed.any() and np.array_equal(radius[listed], rows[listed, 5])
    has_grad = case["ref"].scales["colors"] > 0
    assert listed[has_grad].all()
    for o in outs[:6]:
        assert not o.cpu().numpy()[~listed].any()
    # the colour-only call: the same colour and opacity bits; two calls: the same bits
    plain = _backward(scene, case, frame, st, gf, geometry=False, screen=False)
    assert len(plain) == 2 and torch.equal(_bits(plain[0]), _bits(outs[0])) and torch.equal(_bits(plain[1]), _bits(outs[1]))
    five = _backward(scene, case, frame, st, gf, screen=False)
    again = _backward(scene, case, frame, st, gf)
    assert len(five) == 5 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(five, outs))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, outs))
    # published rectangles: the same frame, other slots -- within the bound, not bit-equal
    frame_p, st_p = _forward(scene, case, published_rects=True)
    assert torch.equal(frame_p, frame) and st_p["n_instances"] >= st["n_instances"]
    outs_p = _backward(scene, case, frame_p, st_p, gf, published=True)
    err_p = _errors(case, outs_p)
    print("%s: published rectangles: %s" % (name, ", ".join("%s %.3g" % (k, err_p[k]) for k in KEYS)))
    radius_p = outs_p[6].cpu().numpy().reshape(-1)
    assert np.array_equal(radius_p[radius_p > 0], rows[radius_p > 0, 5]) and (radius_p > 0)[listed].all()
    for k in KEYS:
        assert err[k] <= BOUND[k], (name, k, err[k])
        assert err_p[k] <= BOUND[k], (name, "published", k, err_p[k])


@pytest.mark.parametrize("name", ["ring_40x24", "random_96x80_n1000_t32"])
def test_wh3_and_hw3_agree_bit_for_bit(tmp_path, name):
    case, scene = _std_scene(tmp_path, name)
    gf = torch.from_numpy(case["g"]).to(DEV)
    frame, st = _forward(scene, case)
    frame_w, st_w = _forward(scene, case, layout="wh3")
    assert torch.equal(frame_w.permute(1, 0, 2), frame)
    a = _backward(scene, case, frame, st, gf)
    b = _backward(scene, case, frame_w, st_w, gf.permute(1, 0, 2).contiguous(), layout="wh3")
    for k, (x, y) in enumerate(zip(a, b)):
        # (the ring's Gaussians are isotropic: their quaternion gradient, output 4, is an exact zero)
        assert (x.abs().max() > 0 or (k == 4 and name == "ring_40x24")) and torch.equal(_bits(x), _bits(y)), k


GUARD, SENTINEL = 64, 12345.0


def test_every_output_stays_inside_its_buffer(tmp_path):
    """The C ABI called directly with every output carved out of a guarded buffer: the margins keep the sentinel, every row
    inside is written, and the values are the ones the Python path gets."""
    from intro_to_gaussian_splatting_amd import _ffi
    from intro_to_gaussian_splatting_amd._device import _WORKSPACE, _ptr, _stream_handle

    case, scene = _std_scene(tmp_path, "random_130x70_n1500_t8")
    gf = torch.from_numpy(case["g"]).to(DEV)
    frame, st = _forward(scene, case)
    want = _backward(scene, case, frame, st, gf)
    lib = _ffi.load()
    dev, n, tensors = scene._inputs(1)
    cam = scene.images[1].gsx_camera()
    params, _ = scene._frame_params(dev, n, "hw3", "std_3dgs")
    params.background[0], params.background[1], params.background[2] = case["bg"]
    widths = (3, 1, 3, 3, 4, 2, 1)
    wholes = [torch.full((GUARD + n * k + GUARD,), SENTINEL, dtype=torch.float32, device=DEV) for k in widths]
    outs = [w[GUARD:GUARD + n * k] for w, k in zip(wholes, widths)]
    with torch.cuda.device(dev):
        nbytes = lib.gsx_backward_std_workspace_bytes(n, cam.width, cam.height, case["tile"], st["n_instances"] + 4096)
        ws = _WORKSPACE.get(dev, nbytes)
        rc = lib.gsx_render_backward_std(ctypes.byref(cam), *[_ptr(t.detach()) for t in tensors], n, case["tile"], _ptr(frame),
                                         _ptr(gf), *[_ptr(o) for o in outs], ctypes.byref(params), _ptr(ws), nbytes,
                                         _stream_handle(dev))
    _ffi.check(rc)
    for whole, out, k, ref in zip(wholes, outs, widths, want):
        w = whole.cpu().numpy()
        assert (w[:GUARD] == SENTINEL).all() and (w[GUARD + n * k:] == SENTINEL).all()
        assert not (out == SENTINEL).any()
        assert torch.equal(_bits(out), _bits(ref.reshape(-1)))


NAMES = ("points", "scales", "quaternions", "opacity", "colors")


def _autograd(scene, case, gf, names=NAMES, layout="hw3", **kw):
    g = scene.gaussians
    for name in NAMES + ("sh",):
        t = getattr(g, name, None)
        if t is not None:
            t.requires_grad_(name in names)
            t.grad = None
    frame = scene.render_image_hip(1, tile_size=case["tile"], layout=layout, semantics="std_3dgs", background=case["bg"], **kw)
    (frame * gf).sum().backward()
    out = {}
    for name in NAMES + ("sh",):
        t = getattr(g, name, None)
        if t is not None:
            out[name] = None if t.grad is None else t.grad.detach().clone()
            t.requires_grad_(False)
            t.grad = None
    return frame, out


def test_the_frame_with_grad_is_the_frame_without_and_backward_is_the_one_call(tmp_path):
    case, scene = _std_scene(tmp_path, "ring_40x24")
    gf = torch.from_numpy(case["g"]).to(DEV)
    plain, st = _forward(scene, case)
    want = _backward(scene, case, plain, st, gf)
    frame, grads = _autograd(scene, case, gf, geometry_gradients=True, screen_statistics=True)
    assert frame.grad_fn is not None and torch.equal(frame.detach(), plain)
    for name, ref in zip(("colors", "opacity", "points", "scales", "quaternions"), want):
        # (the ring's Gaussians are isotropic: their quaternion gradient is an exact zero)
        assert grads[name].abs().max() > 0 or name == "quaternions", name
        assert torch.equal(_bits(grads[name].reshape(-1)), _bits(ref.reshape(-1))), name
    idx, g2d, radius = scene.screen_statistics
    assert idx == 1 and torch.equal(_bits(g2d), _bits(want[5])) and torch.equal(_bits(radius), _bits(want[6].view(-1)))
    # without geometry_gradients: colours and opacity alone, the same bits
    frame2, grads2 = _autograd(scene, case, gf, names=("colors", "opacity"))
    assert torch.equal(frame2.detach(), plain) and grads2["points"] is None
    assert torch.equal(_bits(grads2["colors"]), _bits(grads["colors"])) and torch.equal(_bits(grads2["opacity"]), _bits(grads["opacity"]))
    # published_rects goes through to the backward
    frame3, grads3 = _autograd(scene, case, gf, geometry_gradients=True, published_rects=True)
    want3 = _backward(scene, case, plain, _forward(scene, case, published_rects=True)[1], gf, screen=False, published=True)
    assert torch.equal(_bits(grads3["points"].reshape(-1)), _bits(want3[2].reshape(-1)))


def test_the_refusals_under_std_3dgs_raise_by_name_and_run_without_grad(tmp_path):
    case, scene = _std_scene(tmp_path, "stack_half_16x16")
    g = scene.gaussians
    g.colors.requires_grad_(True)
    g.points.requires_grad_(True)
    kw = dict(tile_size=case["tile"], semantics="std_3dgs", background=case["bg"], geometry_gradients=True)
    bg_grad = torch.tensor([0.1, 0.2, 0.3], requires_grad=True)
    refused = [("camera_gradients", dict(kw, camera_gradients=True)),
               ("screen_statistics='abs'", dict(kw, screen_statistics="abs")),
               ("background", dict(kw, background=bg_grad)),
               ("semantics='ref_cuda'", dict(kw, semantics="ref_cuda", background=(0.0, 0.0, 0.0))),
               ("tile_window", dict(kw, tile_window=(0, 1, 0, 1)))]
    for word, call in refused:
        with pytest.raises(ValueError, match=word):
            scene.render_image_hip(1, **call)
    with torch.no_grad():
        for word, call in refused:
            if word == "background":
                call = dict(call, background=tuple(float(v) for v in bg_grad.detach()))
            assert scene.render_image_hip(1, **call).grad_fn is None
    assert scene.render_image_hip(1, **kw).grad_fn is not None
    g.colors.requires_grad_(False)
    g.points.requires_grad_(False)


def test_an_sh_scene_carries_the_kernel_s_colour_gradient_on_to_the_coefficients(tmp_path):
    from intro_to_gaussian_splatting_amd.synthetic import make_scene
    from test_hip_sh_backward import _sh_for

    sc = make_scene(200, 64, 48, seed=21, sigma_scale=2.0)
    scene = _scene(tmp_path, sc)
    g = scene.gaussians
    g.sh = torch.from_numpy(_sh_for(g.colors.cpu().numpy(), 2, 3)).to(DEV).contiguous()
    g.sh_degree = 2
    case = dict(tile=16, bg=(0.2, 0.4, 0.6))
    gf = torch.from_numpy(np.random.RandomState(3).uniform(-1, 1, (48, 64, 3)).astype(np.float32)).to(DEV)
    plain, st = _forward(scene, case)
    outs = _backward(scene, case, plain, st, gf, screen=False)
    gsh, gview = scene._sh_backward(1, outs[0], with_points=True)
    frame, grads = _autograd(scene, case, gf, names=("points", "opacity", "sh"), geometry_gradients=True)
    assert torch.equal(frame.detach(), plain) and grads["colors"] is None
    assert grads["sh"].abs().max() > 0 and torch.equal(_bits(grads["sh"].reshape(-1)), _bits(gsh.reshape(-1)))
    assert torch.equal(_bits(grads["opacity"].reshape(-1)), _bits(outs[1].reshape(-1)))
    assert torch.equal(_bits(grads["points"]), _bits(outs[2] + gview))


# ---------------------------------------------------------------------------------------------- Trainer
LR = {"points": 2e-4, "scales": 2e-3, "quaternions": 1e-3, "opacity": 2e-2, "colors": 5e-3}
DENSITY = dict(grad_threshold=2e-5, dense_scale=0.05, prune_logit=-4.5)
FIT_BG = (0.1, 0.2, 0.3)


def _fit_scene(path, seed):
    """64x48, 300 Gaussians, two views; the targets are the std_3dgs frames before a perturbation."""
    from intro_to_gaussian_splatting_amd import GaussianScene, Gaussians
    from intro_to_gaussian_splatting_amd.synthetic import make_scene, orbit_poses, write_colmap_text

    sc = make_scene(300, 64, 48, seed=31, sigma_scale=2.0)
    path.mkdir(exist_ok=True)
    write_colmap_text(str(path), sc, extra_poses=orbit_poses(2, step_deg=4.0, qvec=sc["qvec"], tvec=sc["tvec"])[1:])
    g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"], device=DEV)
    scene = GaussianScene(str(path), g)
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        targets = {i: scene.render_image_hip(i, semantics="std_3dgs", background=FIT_BG).clone() for i in sorted(scene.images)}
        g.points.add_(torch.from_numpy(rs.normal(0, 0.05, size=tuple(g.points.shape)).astype(np.float32)).to(DEV))
        g.opacity.add_(torch.from_numpy(rs.normal(0, 0.5, size=tuple(g.opacity.shape)).astype(np.float32)).to(DEV))
    assert len(targets) == 2
    return scene, targets


def _state(g, opt):
    out = {name: getattr(g, name).detach().clone() for name in LR}
    out.update({"m_" + name: opt.exp_avg[name].clone() for name in LR})
    out.update({"v_" + name: opt.exp_avg_sq[name].clone() for name in LR})
    return out


def test_trainer_under_std_3dgs_is_the_composition_written_out(tmp_path):
    from intro_to_gaussian_splatting_amd import DensityControl, GaussianAdam, Trainer

    steps, seed = 3, 5
    periods = dict(sh_degree_every=None, densify_every=2, opacity_reset_every=None, densify_from=0, densify_until=100)
    scene, targets = _fit_scene(tmp_path / "a", 1)
    trainer = Trainer(scene, targets, lr=LR, lambda_dssim=0.2, tile_size=16, statistic="screen", density=DENSITY, seed=seed,
                      semantics="std_3dgs", background=FIT_BG, **periods)
    seen = []
    trainer.fit(steps, callback=lambda t, losses, idx: seen.append((losses, idx, len(t.gaussians))))

    scene2, targets2 = _fit_scene(tmp_path / "b", 1)
    g = scene2.gaussians
    for name in LR:
        getattr(g, name).requires_grad_(True)
    opt = GaussianAdam(g, lr=LR)
    dc = DensityControl(g, optimizer=opt, scene=scene2, statistic="screen", **DENSITY)
    split = torch.Generator(device=DEV).manual_seed(seed)
    views = torch.Generator(device="cpu").manual_seed(seed)
    order, by_hand = [], []
    for s in range(1, steps + 1):
        if not order:
            order = [sorted(targets2)[i] for i in torch.randperm(2, generator=views).tolist()]
        idx = order.pop(0)
        terms = {}
        frame = scene2.render_image_hip(idx, tile_size=16, geometry_gradients=True, screen_statistics=True,
                                        semantics="std_3dgs", background=FIT_BG)
        assert tuple(scene2.rendered_region(idx, 16, semantics="std_3dgs")) == (64, 48)
        loss = scene2.photometric_loss(idx, frame, targets2[idx], tile_size=16, lambda_dssim=0.2, terms=terms,
                                       semantics="std_3dgs")
        loss.backward()
        dc.accumulate()
        opt.step()
        opt.zero_grad()
        if s % 2 == 0:
            dc.densify_and_prune(generator=split)
        by_hand.append((torch.stack((loss.detach(), terms["l1"], terms["ssim"])), idx, len(g)))
    print("views and rows per step", [v[1:] for v in seen])
    assert [v[1:] for v in seen] == [v[1:] for v in by_hand]
    assert all(torch.equal(_bits(a[0]), _bits(b[0])) for a, b in zip(seen, by_hand))
    got, want = _state(trainer.gaussians, trainer.opt), _state(g, opt)
    for key in want:
        assert torch.equal(_bits(got[key]), _bits(want[key])), key
    # evaluate() renders under the same rules: against the targets it was built from, a perfect score before the perturbation
    scene3, targets3 = _fit_scene(tmp_path / "c", 1)
    ev = Trainer(scene3, targets3, lr=LR, semantics="std_3dgs", background=FIT_BG, **periods).evaluate()
    with torch.no_grad():
        mse = ((scene3.render_image_hip(1, semantics="std_3dgs", background=FIT_BG) - targets3[1]) ** 2).mean()
    assert ev[1]["psnr"] == pytest.approx(-10.0 * np.log10(float(mse)), rel=1e-5)
    for bad in (dict(refine_poses=dict(lr_rotation=1e-3, lr_translation=1e-3)), dict(depth_targets={1: targets3[1][..., 0]}),
                dict(statistic="screen_abs")):
        with pytest.raises(ValueError, match="std_3dgs"):
            Trainer(scene3, targets3, lr=LR, semantics="std_3dgs", **bad)


def test_a_short_fit_under_std_3dgs_with_one_densify_event(tmp_path):
    from intro_to_gaussian_splatting_amd import Trainer
    from test_hip_density import _quantile_knobs

    scene, targets = _fit_scene(tmp_path / "a", 2)
    trainer = Trainer(scene, targets, lr=LR, lambda_dssim=0.2, tile_size=16, statistic="screen", density=DENSITY, seed=3,
                      semantics="std_3dgs", background=FIT_BG, sh_degree_every=None, densify_every=10, densify_from=0,
                      densify_until=10, opacity_reset_every=None)
    rows0 = len(scene.gaussians)
    losses = []

    def after_step(t, l, idx):
        losses.append(l[0])
        if len(losses) == 9:        # before the one event (step 10): thresholds from the scene itself, as the density tests
            _quantile_knobs(t.density, t.gaussians)         # set them -- here the hottest ~3 % densify and nothing is pruned:
            dc = t.density                                  # on 300 large Gaussians a round of 8 % costs more than 20 steps win back
            mean = dc.grad_sum / dc.seen.clamp(min=1).float()
            dc.grad_threshold = float(torch.quantile(mean[dc.seen > 0], 0.97))
            dc.prune_logit = -1e30

    trainer.fit(30, callback=after_step)
    losses = [float(v) for v in losses]
    print("short fit under std_3dgs: rows %d -> %d; losses %s" % (rows0, len(scene.gaussians), ["%.4g" % v for v in losses]))
    assert np.isfinite(losses).all()
    assert len(scene.gaussians) != rows0
    assert np.mean(losses[-4:]) < np.mean(losses[:4])           # both views are in either window
    # strategy="mcmc" takes the same frame
    scene2, targets2 = _fit_scene(tmp_path / "b", 2)
    mc = Trainer(scene2, targets2, lr=LR, semantics="std_3dgs", background=FIT_BG, strategy="mcmc", mcmc=dict(cap_max=400),
                 sh_degree_every=None, densify_every=None)
    first = float(mc.step()[0][0])
    assert np.isfinite(first)
