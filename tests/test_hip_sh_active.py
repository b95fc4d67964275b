"""The SH degree schedule on the GPU: gsx_sh_to_rgb_active / gsx_sh_backward_active against the existing kernels on the
packed array, ``Gaussians.active_sh_degree`` through ``GaussianScene``, ``GaussianAdam`` on the inactive bands, and
``Trainer`` against the same composition written out here.

Every comparison is of BITS (int32 views: -0 is not +0, NaN is not skipped); there is no tolerance in this file.  The contract
(include/gsx.h): with P = sh[:, :K_A] made contiguous the active entries give what gsx_sh_to_rgb(P, A) / gsx_sh_backward(P, A)
give, and the inactive tail of grad_sh is +0.
"""
import ctypes

import numpy as np
import pytest
import torch

import sh_backward_restatement as shr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAIRS = [(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3)]        # every (active, stored) with active < stored
SIZES = (1, 255, 256, 257, 1000)                                # one row, a block less one, a block, a block and one, four blocks
GUARD, SENTINEL = 64, 12345.0


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _lib():
    from intro_to_gaussian_splatting_amd import _ffi

    return _ffi, _ffi.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _center(center=shr.CENTER):
    return (ctypes.c_float * 3)(*[float(v) for v in center])


def _based(src, lead):
    """A contiguous copy of ``src`` whose base is 16-byte aligned (``lead`` 0) or only 4-byte aligned (``lead`` 1 .. 3)."""
    whole = torch.empty(8 + src.numel(), dtype=torch.float32, device=DEV)
    off = (-(whole.data_ptr() // 4)) % 4 + lead
    view = whole[off:off + src.numel()].view(src.shape)
    view.copy_(src)
    assert (view.data_ptr() % 16 == 0) == (lead == 0) and view.data_ptr() % 4 == 0
    return whole, view


def _guarded(shape, lead):
    """(whole buffer, a view of ``shape`` behind a guard with its base aligned like ``_based``'s, its offset) filled with
    the sentinel."""
    numel = int(np.prod(shape))
    whole = torch.full((GUARD + 8 + numel + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    off = GUARD + (-(whole.data_ptr() // 4 + GUARD)) % 4 + lead
    view = whole[off:off + numel].view(shape)
    assert (view.data_ptr() % 16 == 0) == (lead == 0)
    return whole, view, off


def _old(pts, packed, degree, gc, with_points=True):
    """(colours, dL/dsh, dL/dmean) of the existing entries on a packed degree-``degree`` array."""
    _ffi, lib = _lib()
    n, k = int(pts.shape[0]), (degree + 1) ** 2
    colors = torch.empty((n, 3), device=DEV)
    gsh = torch.empty((n, k, 3), device=DEV)
    gmean = torch.empty((n, 3), device=DEV) if with_points else None
    _ffi.check(lib.gsx_sh_to_rgb(_p(pts), _p(packed), degree, n, _center(), _p(colors), _stream()))
    _ffi.check(lib.gsx_sh_backward(_p(pts), _p(packed), degree, n, _center(), _p(gc), _p(gsh), _p(gmean), _stream()))
    return colors, gsh, gmean


def _active(pts, sh, stored, active, gc, lead, with_points=True):
    """The same of the active entries on the degree-``stored`` array; grad_sh behind guards, checked to be left alone."""
    _ffi, lib = _lib()
    n, ks = int(pts.shape[0]), (stored + 1) ** 2
    colors = torch.empty((n, 3), device=DEV)
    whole, gsh, off = _guarded((n, ks, 3), lead)
    gmean = torch.empty((n, 3), device=DEV) if with_points else None
    _ffi.check(lib.gsx_sh_to_rgb_active(_p(pts), _p(sh), stored, active, n, _center(), _p(colors), _stream()))
    _ffi.check(lib.gsx_sh_backward_active(_p(pts), _p(sh), stored, active, n, _center(), _p(gc), _p(gsh), _p(gmean),
                                          _stream()))
    w = whole.cpu().numpy()
    assert (w[:off] == SENTINEL).all() and (w[off + n * ks * 3:] == SENTINEL).all()
    return colors, gsh, gmean


@pytest.mark.parametrize("active,stored", PAIRS)
def test_active_entries_give_the_packed_kernels_bits(active, stored):
    ka = (active + 1) ** 2
    for n in SIZES:
        pts, sh, gc = shr.case_inputs(n, stored, 0)
        d_pts, d_gc = torch.from_numpy(pts).to(DEV), torch.from_numpy(gc).to(DEV)
        packed = torch.from_numpy(np.ascontiguousarray(sh[:, :ka])).to(DEV)
        want_c, want_sh, want_mean = _old(d_pts, packed, active, d_gc)
        _, want_sh_alone, _ = _old(d_pts, packed, active, d_gc, with_points=False)
        assert _same_bits(want_sh_alone, want_sh)
        poisoned = sh.copy()
        poisoned[:, ka:] = np.nan
        for lead in (0, 1):             # a 16-byte aligned base, and one that is only 4-byte aligned
            for src in (sh, poisoned):  # whatever the inactive coefficients hold
                keep, d_sh = _based(torch.from_numpy(src).to(DEV), lead)
                for with_points in (True, False):
                    got_c, got_sh, got_mean = _active(d_pts, d_sh, stored, active, d_gc, lead, with_points)
                    what = (n, lead, src is poisoned, with_points)
                    assert _same_bits(got_c, want_c), what
                    assert _same_bits(got_sh[:, :ka], want_sh), what
                    assert not _bits(got_sh[:, ka:]).any(), what                       # exact +0, every entry written
                    assert torch.isfinite(got_c).all() and torch.isfinite(got_sh).all(), what
                    if with_points:
                        assert _same_bits(got_mean, want_mean) and torch.isfinite(got_mean).all(), what
                        assert bool(got_mean.any()) == (active > 0), what
        assert want_sh.abs().max() > 0 and want_c.abs().max() > 0


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_every_band_active_is_the_old_entries_bits(degree):
    for n in (257, 1000):
        pts, sh, gc = shr.case_inputs(n, degree, 0)
        d_pts, d_sh, d_gc = (torch.from_numpy(a).to(DEV) for a in (pts, sh, gc))
        want = _old(d_pts, d_sh, degree, d_gc)
        got = _active(d_pts, d_sh, degree, degree, d_gc, 0)
        for a, b in zip(got, want):
            assert _same_bits(a, b)


def test_abi_accepts_nothing_and_names_the_degree_it_refuses():
    _ffi, lib = _lib()
    null, c = ctypes.c_void_p(0), _center()
    assert lib.gsx_sh_to_rgb_active(null, null, 3, 1, 0, c, null, _stream()) == _ffi.GSX_OK
    assert lib.gsx_sh_backward_active(null, null, 3, 1, 0, c, null, null, null, _stream()) == _ffi.GSX_OK
    t = torch.zeros(64, device=DEV)
    p = _p(t)
    for stored, active, name in ((4, 0, "stored_degree"), (-1, 0, "stored_degree"), (3, -1, "active_degree"),
                                 (3, 4, "active_degree"), (1, 2, "active_degree")):
        assert lib.gsx_sh_to_rgb_active(p, p, stored, active, 1, c, p, _stream()) == _ffi.GSX_ERR_INVALID_ARGUMENT
        assert name in lib.gsx_last_error().decode()
        assert lib.gsx_sh_backward_active(p, p, stored, active, 1, c, p, p, null, _stream()) == _ffi.GSX_ERR_INVALID_ARGUMENT
        assert name in lib.gsx_last_error().decode()


# ---- through the scene
def _scene(path, n, degree, views=1, seed=3, sh=None, sh_degree=None, arrays=None):
    """An 80 x 64 trained-like SH scene of ``n`` Gaussians stored at ``degree``, images 1 .. ``views`` on a small orbit.
    ``sh`` / ``sh_degree`` replace the coefficients (a truncated copy); ``arrays``: receives the scene's numpy arrays."""
    from intro_to_gaussian_splatting_amd import GaussianScene, Gaussians
    from intro_to_gaussian_splatting_amd.synthetic import make_trained_like_scene, orbit_poses, write_colmap_text

    sc = make_trained_like_scene(n, 80, 64, seed=seed, sh_degree=degree)
    poses = orbit_poses(3, step_deg=4.0)        # the base pose is the middle one
    write_colmap_text(str(path), sc, extra_poses=[poses[0], poses[2]][:views - 1])
    g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"], device=DEV)
    g.sh = torch.from_numpy(sc["sh"] if sh is None else sh).to(DEV).contiguous()
    g.sh_degree = degree if sh_degree is None else sh_degree
    if arrays is not None:
        arrays.update(sc)
    return GaussianScene(str(path), g)


TRAINED = ("points", "scales", "quaternions", "opacity", "sh")


def _frame_and_grads(scene, W):
    g = scene.gaussians
    for name in TRAINED:
        getattr(g, name).requires_grad_(True)
        getattr(g, name).grad = None
    frame = scene.render_image_hip(1, geometry_gradients=True)
    (frame * W).sum().backward()
    grads = {name: getattr(g, name).grad.detach().clone() for name in TRAINED}
    for name in TRAINED:
        getattr(g, name).requires_grad_(False)
        getattr(g, name).grad = None
    return frame.detach().clone(), grads


@pytest.mark.parametrize("active", [0, 1, 2])
def test_scene_on_its_schedule_is_the_truncated_scene(tmp_path, active):
    arrays = {}
    full = _scene(tmp_path, 300, 3, arrays=arrays)
    ka = (active + 1) ** 2
    cut = _scene(tmp_path, 300, 3, sh=np.ascontiguousarray(arrays["sh"][:, :ka]), sh_degree=active)
    assert cut.gaussians.active_sh_degree == active == cut.gaussians.sh_degree
    full.gaussians.active_sh_degree = active
    W = torch.from_numpy(np.random.RandomState(7).normal(size=(80, 64, 3)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        plain_full, plain_cut = full.render_image_hip(1).clone(), cut.render_image_hip(1).clone()
        colors_full, colors_cut = full._colors(1).clone(), cut._colors(1).clone()
    assert _same_bits(colors_full, colors_cut)
    assert plain_cut.abs().max() > 0
    # the frame without gradients: evaluated colours (full) against the projection's inline evaluation (cut)
    assert _same_bits(plain_full, plain_cut)
    frame_full, grads_full = _frame_and_grads(full, W)
    frame_cut, grads_cut = _frame_and_grads(cut, W)
    assert _same_bits(frame_full, plain_cut) and _same_bits(frame_cut, plain_cut)
    assert grads_full["sh"].shape == (300, 16, 3) and grads_cut["sh"].abs().max() > 0
    assert _same_bits(grads_full["sh"][:, :ka], grads_cut["sh"])
    assert not _bits(grads_full["sh"][:, ka:]).any()
    for name in ("points", "opacity", "scales", "quaternions"):
        assert grads_cut[name].abs().max() > 0 and _same_bits(grads_full[name], grads_cut[name]), name
    # the other entries honour the active degree too: stage 1's colours, a tile window, a frame enqueued without waiting
    with torch.no_grad():
        assert _same_bits(full.preprocess(1).colors, cut.preprocess(1).colors)
        assert _same_bits(full.render_image_hip(1, tile_window=(1, 3, 0, 2)), cut.render_image_hip(1, tile_window=(1, 3, 0, 2)))
        speculative = full.render_image_hip(1, no_sync=True)
        full.confirm_frames()
        assert _same_bits(speculative, plain_cut)
    cam_buf = torch.frombuffer(bytearray(bytes(full.images[1].gsx_camera())), dtype=torch.uint8).to(DEV)
    with torch.no_grad(), pytest.raises(ValueError, match="active_sh_degree"):
        full.render_image_hip(1, camera_buffer=cam_buf)


def test_every_band_active_renders_what_it_rendered(tmp_path):
    """``active_sh_degree`` set to the stored degree, and raised to it step by step: the frame of a scene that never heard of it."""
    a, b = _scene(tmp_path, 300, 3), _scene(tmp_path, 300, 3)
    with torch.no_grad():
        want = a.render_image_hip(1).clone()
        b.gaussians.active_sh_degree = 0
        assert not _same_bits(b.render_image_hip(1), want)
        assert [b.gaussians.oneup_sh_degree() for _ in range(4)] == [1, 2, 3, 3]
        assert _same_bits(b.render_image_hip(1), want)


def test_adam_leaves_the_inactive_bands_alone(tmp_path):
    from intro_to_gaussian_splatting_amd import GaussianAdam

    scene = _scene(tmp_path, 300, 3)
    g = scene.gaussians
    g.active_sh_degree = 1
    with torch.no_grad():
        target = scene.render_image_hip(1).clone() * 0.5
    start = g.sh.detach().clone()
    g.sh.requires_grad_(True)
    opt = GaussianAdam(g, lr={"sh": 0.01})
    for _ in range(10):
        scene.photometric_loss(1, scene.render_image_hip(1), target).backward()
        opt.step()
        opt.zero_grad()
    assert _same_bits(g.sh[:, 4:], start[:, 4:])
    assert not _same_bits(g.sh[:, :4], start[:, :4])
    for moments in (opt.exp_avg["sh"], opt.exp_avg_sq["sh"]):
        assert not _bits(moments[:, 4:]).any() and moments[:, :4].abs().max() > 0
    g.sh.requires_grad_(False)


def test_capture_frame_waits_for_the_last_band(tmp_path):
    scene = _scene(tmp_path, 300, 3)
    g = scene.gaussians
    g.active_sh_degree = 2
    with torch.no_grad():
        with pytest.raises(ValueError, match="active_sh_degree"):
            scene.capture_frame(1)
        assert g.oneup_sh_degree() == 3
        frame = scene.capture_frame(1)
        frame.replay()
        assert _same_bits(frame.confirm(), scene.render_image_hip(1))
        g.active_sh_degree = 1          # a frame captured with every band cannot follow the container back down
        with pytest.raises(ValueError, match="active_sh_degree"):
            frame.replay()


# ---- the fit loop
LR = {"points": 2e-4, "scales": 2e-3, "quaternions": 1e-3, "opacity": 2e-2, "sh": 5e-3}
PERIODS = dict(sh_degree_every=4, densify_every=5, opacity_reset_every=9, densify_from=0, densify_until=100)
DENSITY = dict(grad_threshold=2e-5, dense_scale=0.05, prune_logit=-4.5)
RESET_LOGIT = -2.0


def _fit_scene(path, seed):
    """(scene of 3 views stored at degree 2, on active degree 0, perturbed; targets rendered before the perturbation)."""
    scene = _scene(path, 300, 2, views=3)
    g = scene.gaussians
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        targets = {idx: scene.render_image_hip(idx).clone() for idx in (1, 2, 3)}
        g.sh.add_(torch.from_numpy(rs.normal(0, 0.3, size=tuple(g.sh.shape)).astype(np.float32)).to(DEV))
        g.opacity.add_(torch.from_numpy(rs.normal(0, 0.5, size=tuple(g.opacity.shape)).astype(np.float32)).to(DEV))
    g.active_sh_degree = 0
    return scene, targets


def _state(g, opt):
    out = {name: getattr(g, name).detach().clone() for name in TRAINED}
    out.update({"m_" + name: opt.exp_avg[name].clone() for name in TRAINED})
    out.update({"v_" + name: opt.exp_avg_sq[name].clone() for name in TRAINED})
    return out


def test_trainer_is_the_composition_written_out(tmp_path):
    from intro_to_gaussian_splatting_amd import DensityControl, GaussianAdam, Trainer

    steps, seed = 12, 5
    scene, targets = _fit_scene(tmp_path, 1)
    trainer = Trainer(scene, targets, lr=LR, lambda_dssim=0.2, tile_size=16, statistic="screen", density=DENSITY,
                      opacity_reset_logit=RESET_LOGIT, seed=seed, **PERIODS)
    seen = []
    trainer.fit(steps, callback=lambda t, losses, idx: seen.append((losses, idx, len(t.gaussians), t.gaussians.active_sh_degree)))
    assert trainer.step_count == steps and len(seen) == steps

    # the same by hand: the seven lines of fit.py's docstring
    scene2, targets2 = _fit_scene(tmp_path, 1)
    g = scene2.gaussians
    for name in TRAINED:
        getattr(g, name).requires_grad_(True)
    opt = GaussianAdam(g, lr=LR)
    dc = DensityControl(g, optimizer=opt, scene=scene2, statistic="screen", **DENSITY)
    views, split = torch.Generator(device="cpu").manual_seed(seed), torch.Generator(device=DEV).manual_seed(seed)
    order, by_hand = [], []
    for s in range(1, steps + 1):
        if not order:
            order = [(1, 2, 3)[i] for i in torch.randperm(3, generator=views).tolist()]
        idx = order.pop(0)
        terms = {}
        frame = scene2.render_image_hip(idx, tile_size=16, geometry_gradients=True, screen_statistics=True)
        loss = scene2.photometric_loss(idx, frame, targets2[idx], tile_size=16, lambda_dssim=0.2, terms=terms)
        loss.backward()
        dc.accumulate()
        opt.step()
        opt.zero_grad()
        if s % 5 == 0:
            dc.densify_and_prune(generator=split)
        if s % 9 == 0:
            dc.reset_opacity(RESET_LOGIT)
        if s % 4 == 0:
            g.oneup_sh_degree()
        by_hand.append((torch.stack((loss.detach(), terms["l1"], terms["ssim"])), idx, len(g), g.active_sh_degree))

    rows = [n for _, _, n, _ in seen]
    print("rows per step", rows, "active degree per step", [a for _, _, _, a in seen])
    assert [v[1:] for v in seen] == [v[1:] for v in by_hand]
    assert all(_same_bits(a[0], b[0]) for a, b in zip(seen, by_hand))
    assert sorted(v[1] for v in seen[:3]) == [1, 2, 3]                      # an epoch sees every view once
    assert [a for _, _, _, a in seen] == [0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 2]
    assert len(set(rows)) > 1                                               # the rounds did change the rows
    assert len(trainer.gaussians) == len(g) and trainer.gaussians.active_sh_degree == g.active_sh_degree == 2
    got, want = _state(trainer.gaussians, trainer.opt), _state(g, opt)
    for key in want:
        assert _same_bits(got[key], want[key]), key
    assert trainer.opt.step_count == opt.step_count == steps


def test_a_short_fit_recovers_the_scene(tmp_path):
    from intro_to_gaussian_splatting_amd import Trainer

    scene, targets = _fit_scene(tmp_path, 2)
    trainer = Trainer(scene, targets, lr={"sh": 0.02, "opacity": 0.05}, sh_degree_every=10, densify_every=None,
                      opacity_reset_every=None, seed=0)
    before = trainer.evaluate()
    losses = []
    trainer.fit(40, callback=lambda t, triple, idx: losses.append(triple))
    losses = [float(v[0]) for v in losses]
    after = trainer.evaluate([1, 2, 3])
    print("fit of 40 steps from active degree 0: loss first %.6g, last %.6g; PSNR %s -> %s" % (
        losses[0], losses[-1], ["%.2f" % before[i]["psnr"] for i in (1, 2, 3)], ["%.2f" % after[i]["psnr"] for i in (1, 2, 3)]))
    assert losses[-1] < losses[0]
    assert scene.gaussians.active_sh_degree == 2 and len(scene.gaussians) == 300
    assert set(after[1]) == {"l1", "ssim", "psnr"} and all(np.isfinite(list(v.values())).all() for v in after.values())
