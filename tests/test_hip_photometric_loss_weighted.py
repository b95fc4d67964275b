"""gsx_photometric_loss_weighted on the GPU: value, dL/dframe and dL/dexposure against the float64 restatement
(tests/photometric_loss_weighted_restatement.py) over its cases -- the shapes of the unweighted test at which the kernels
can go wrong (one pixel; a window larger than the image; T - 1 x T + 1; a halo across a whole neighbouring tile on the
scalar path; a cropped region whose weight stride differs from its columns and whose rows end inside a 16-byte access; an
unaligned base) x masks (none, ones, binary with edges on a tile seam and inside a halo, one pixel, random, all zero) x
exposures (none, identity, general, offset only) -- each at lambda in {0, 0.2, 1}, from raw ctypes calls between guarded
margins; bit-equality with gsx_photometric_loss when both options are NULL; repeatability; the Python surface; and the whole
chain: an exposure learned against a frame with another gain, and ``Trainer(masks=, exposure=)`` against its composition
written out by hand.

Bound: BOUND_W = 12 E_REF_W per output, E_REF_W the float32 reference's own error (tests/test_photometric_loss_weighted_host.py,
measured on the CPU: value 9.203e-07, grad 2.282e-06, grad_exposure 3.126e-06).  What the kernels measured on an MI355X over
the twelve cases with a non-zero mask x three lambdas, same units:
    value          1.181e-06  (halo_across_a_neighbour_single_none, lambda 1)
    grad           1.044e-06  (halo_across_a_neighbour_random_general, lambda 1)
    grad_exposure  6.674e-07  (one_pixel_ones_general, lambda 1)
and over the eleven LARGE_CASES with a non-zero mask (9, 16, 256 and 289 tiles: where the two one-workgroup reduces take
their loops' first and second step) x three lambdas, same bound:
    value          8.156e-08  (tiles_4x4_scalar_random_general, lambda 1)
    grad           9.153e-07  (tiles_289_scalar_binary_general, lambda 1)
    grad_exposure  1.472e-07  (tiles_289_scalar_binary_general, lambda 0)
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden

import photometric_loss_restatement as plr
import photometric_loss_weighted_restatement as wr
from test_hip_backward import DEV, _golden_scene
from test_photometric_loss_weighted_host import BOUND_W

pytestmark = pytest.mark.gpu

GUARD = 64              # floats on both sides of every buffer that the call must leave alone
WS_GUARD = 256          # bytes on both sides of the workspace
SENTINEL = 12345.0


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _guarded(values, skip):
    """`values` (numpy float32, any shape) on the device, `skip` floats behind a 64-float guard and in front of another;
    (whole buffer, view of the values' shape)."""
    n = values.size
    whole = torch.full((GUARD + skip + n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    view = whole[GUARD + skip:GUARD + skip + n].view(values.shape)
    view.copy_(torch.from_numpy(values))
    return whole, view


def _guards_intact(whole, skip, n):
    w = whole.cpu().numpy()
    return w.size == GUARD + skip + n + GUARD and (w[:GUARD + skip] == SENTINEL).all() and (w[GUARD + skip + n:] == SENTINEL).all()


def _p(t, off=0):
    return ctypes.c_void_p(0 if t is None else t.data_ptr() + off)


def _call(x_dev, y_dev, m_dev, e_dev, region, lam, grad_dev, want_grad_e):
    """One library call on device views; returns (loss_out (4 floats, numpy), dL/dE (3, 4) numpy or None).  loss_out,
    grad_exposure and the workspace are guarded."""
    from intro_to_gaussian_splatting_amd import _ffi

    lib = _ffi.load()
    a, b = region
    stride = int(x_dev.shape[1]) * 3
    nbytes = lib.gsx_photometric_loss_weighted_workspace_bytes(a, b, 0 if grad_dev is None else 1)
    assert nbytes > 0 and nbytes % 256 == 0
    ws = torch.full((WS_GUARD + nbytes + WS_GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    out_whole = torch.full((GUARD + 4 + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    ge_whole = torch.full((GUARD + 12 + GUARD,), SENTINEL, dtype=torch.float32, device=DEV) if want_grad_e else None
    _ffi.check(lib.gsx_photometric_loss_weighted(
        _p(x_dev), stride, _p(y_dev), stride, _p(m_dev), int(x_dev.shape[1]), _p(e_dev), a, b, lam, _p(out_whole, 4 * GUARD),
        _p(grad_dev), stride, _p(ge_whole, 4 * GUARD) if want_grad_e else None, _p(ws, WS_GUARD), nbytes, _stream()))
    torch.cuda.synchronize()
    w = ws.cpu().numpy()
    assert (w[:WS_GUARD] == 0xA5).all() and (w[WS_GUARD + nbytes:] == 0xA5).all(), "the workspace was overrun"
    assert _guards_intact(out_whole, 0, 4)
    grad_e = None
    if want_grad_e:
        assert _guards_intact(ge_whole, 0, 12)
        grad_e = ge_whole[GUARD:GUARD + 12].cpu().numpy().reshape(3, 4)
    return out_whole[GUARD:GUARD + 4].cpu().numpy(), grad_e


def _evaluate(x, y, m, E, region, skip, lam):
    """Value + gradients call, the same call again and the value-only call on fresh buffers: (loss_out, the full-tensor
    dL/dframe buffer as numpy -- sentinel where nothing was written --, dL/dE or None), with everything the contract
    promises about writes and repeatability asserted on the way."""
    a, b = region
    wx, dx = _guarded(x, skip)
    wy, dy = _guarded(y, skip)
    wm, dm = (None, None) if m is None else _guarded(m, skip)
    de = None if E is None else torch.from_numpy(E).to(DEV)
    wg, dg = _guarded(np.full(x.shape, SENTINEL, np.float32), skip)
    assert (dx.data_ptr() % 16 == 0) == (skip % 4 == 0) and dg.data_ptr() % 16 == dx.data_ptr() % 16
    out, grad_e = _call(dx, dy, dm, de, region, lam, dg, E is not None)
    grad = dg.cpu().numpy()
    # inputs untouched, nothing outside the region written (nothing behind a row's 3 cols floats, nothing below the region),
    # every region element written
    assert _guards_intact(wx, skip, x.size) and _guards_intact(wy, skip, x.size) and _guards_intact(wg, skip, x.size)
    assert np.array_equal(dx.cpu().numpy(), x) and np.array_equal(dy.cpu().numpy(), y)
    if m is not None:
        assert _guards_intact(wm, skip, m.size) and np.array_equal(dm.cpu().numpy(), m)
    if E is not None:
        assert np.array_equal(de.cpu().numpy(), E) and np.isfinite(grad_e).all()
    outside = np.ones(x.shape, bool)
    outside[:a, :b] = False
    assert (grad[outside] == SENTINEL).all(), "written outside the region"
    assert not (grad[:a, :b] == SENTINEL).any() and np.isfinite(grad[:a, :b]).all() and np.isfinite(out).all()
    # two calls: the same bits, dL/dE included; the value-only call, and the call without dL/dE: the same four loss_out bits
    wg2, dg2 = _guarded(np.full(x.shape, SENTINEL, np.float32), skip)
    out2, grad_e2 = _call(dx, dy, dm, de, region, lam, dg2, E is not None)
    assert np.array_equal(out2.view(np.uint32), out.view(np.uint32)) and torch.equal(_bits(dg2), _bits(dg))
    if E is not None:
        assert np.array_equal(grad_e2.view(np.uint32), grad_e.view(np.uint32))
        wg3, dg3 = _guarded(np.full(x.shape, SENTINEL, np.float32), skip)
        out4, _ = _call(dx, dy, dm, de, region, lam, dg3, False)
        assert np.array_equal(out4.view(np.uint32), out.view(np.uint32)) and torch.equal(_bits(dg3), _bits(dg))
    out3, _ = _call(dx, dy, dm, de, region, lam, None, False)
    assert np.array_equal(out3.view(np.uint32), out.view(np.uint32))
    return out, grad, grad_e


@functools.lru_cache(maxsize=None)          # one float64 reference per (case, lambda), shared
def _reference(name, lam):
    x, y, m, E = wr.cropped_inputs(name)
    return wr.forward(x, y, lam, m, E), wr.gradient(x, y, lam, m, E)


def _held_to_the_restatement(name):
    _, (a, b), skip = wr.case_geometry(name)
    x, y, m, E = wr.case_inputs(name)
    for lam in wr.LAMBDAS:
        out, grad, grad_e = _evaluate(x, y, m, E, (a, b), skip, lam)
        ref, (ref_grad, ref_grad_e) = _reference(name, lam)
        e = wr.errors(out[0], grad[:a, :b], grad_e, ref[0], ref_grad, ref_grad_e)
        print("%s lambda %.1f: kernel vs restatement: %s" % (name, lam, ", ".join(
            "%s %.4g (bound %.3g)" % (k, v, BOUND_W[k]) for k, v in sorted(e.items()))))
        for key, val in e.items():
            assert val <= BOUND_W[key], (name, lam, key, val)
        # l1 and ssim are weighted means of quantities of order one: the value's bound, absolute; W in its own units
        assert abs(float(out[1]) - ref[1]) <= BOUND_W["value"] and abs(float(out[2]) - ref[2]) <= BOUND_W["value"], (out, ref)
        assert abs(float(out[3]) - ref[3]) <= BOUND_W["value"] * ref[3], (out, ref)


@pytest.mark.parametrize("name", wr.NONZERO_CASE_IDS)
def test_value_and_gradients_match_the_restatement_at_every_edge(name):
    _held_to_the_restatement(name)


@pytest.mark.parametrize("name", wr.LARGE_NONZERO_CASE_IDS)
def test_value_and_gradients_match_the_restatement_where_the_reduce_loops_repeat(name):
    """wr.LARGE_CASES: loss, l1, ssim, W, dL/dimage and dL/dE within the same 12 E_REF_W at 9, 16, 256 and 289 tile
    partials -- at 289 threads 0..32 of wloss_reduce_kernel and of wloss_exposure_reduce_kernel (the only user of
    sum_records<12>) take a second record."""
    _, region, _ = wr.case_geometry(name)
    assert plr.tiles_of(region) in (9, 16, 256, 289) and (plr.tiles_of(region) == 289) == name.startswith("tiles_289")
    _held_to_the_restatement(name)


def _zero_weight_gives_exact_zeros(name):
    _, (a, b), skip = wr.case_geometry(name)
    x, y, m, E = wr.case_inputs(name)
    assert not m[:a, :b].any() and m[a:].all() and m[:, b:].all()
    for lam in wr.LAMBDAS:
        out, grad, grad_e = _evaluate(x, y, m, E, (a, b), skip, lam)
        assert not out.view(np.uint32).any()                                  # +0, bit for bit
        assert not np.ascontiguousarray(grad[:a, :b]).view(np.uint32).any()
        assert grad_e is None or not grad_e.view(np.uint32).any()


@pytest.mark.parametrize("name", wr.ZERO_CASE_IDS)
def test_an_all_zero_weight_gives_exact_zeros(name):
    _zero_weight_gives_exact_zeros(name)


@pytest.mark.parametrize("name", wr.LARGE_ZERO_CASE_IDS)
def test_an_all_zero_weight_gives_exact_zeros_over_289_tiles(name):
    x, y, m, E = wr.case_inputs(name)
    assert plr.tiles_of(wr.case_geometry(name)[1]) == 289 and E is not None
    _zero_weight_gives_exact_zeros(name)


@pytest.mark.parametrize("base", ["tile_minus_1_by_tile_plus_1", "cropped_45x50_of_48x64", "unaligned_base"])
def test_both_options_null_are_the_bits_of_the_plain_entry(base):
    from intro_to_gaussian_splatting_amd import _ffi

    lib = _ffi.load()
    _, shape, (a, b), skip = plr.CASES[plr.CASE_IDS.index(base)]
    x, y = plr.case_inputs(base)
    stride = 3 * shape[1]
    for lam in wr.LAMBDAS:
        wx, dx = _guarded(x, skip)
        wy, dy = _guarded(y, skip)
        out, grad, _ = _evaluate(x, y, None, None, (a, b), skip, lam)
        wg, dg = _guarded(np.full(x.shape, SENTINEL, np.float32), skip)
        plain = torch.full((3,), SENTINEL, dtype=torch.float32, device=DEV)
        nbytes = lib.gsx_photometric_loss_workspace_bytes(a, b, 1)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
        _ffi.check(lib.gsx_photometric_loss(_p(dx), stride, _p(dy), stride, a, b, lam, _p(plain), _p(dg), stride, _p(ws), nbytes,
                                            _stream()))
        torch.cuda.synchronize()
        assert np.array_equal(plain.cpu().numpy().view(np.uint32), out[:3].view(np.uint32))
        assert np.array_equal(dg.cpu().numpy().view(np.uint32), grad.view(np.uint32))       # the untouched sentinels included
        assert out[3] == np.float32(a * b)


# ---- the Python surface
def test_python_surface_autograd_is_the_raw_call_times_grad_output():
    from intro_to_gaussian_splatting_amd import photometric_loss
    from intro_to_gaussian_splatting_amd.loss import _call_weighted

    name = "cropped_45x50_of_48x64_random_offset"
    x, y, m, E = wr.case_inputs(name)
    _, (a, b), _ = wr.case_geometry(name)
    tx, ty, tm, tE = (torch.from_numpy(v).to(DEV) for v in (x, y, m, E))
    terms = {}
    value = photometric_loss(tx, ty, region=(a, b), terms=terms, weight=tm, exposure=tE)
    assert value.shape == () and value.dtype == torch.float32 and not value.requires_grad
    ref, (ref_grad, ref_grad_e) = _reference(name, 0.2)
    assert abs(float(value) - ref[0]) <= BOUND_W["value"] * ref[0]
    assert abs(float(terms["l1"]) - ref[1]) <= BOUND_W["value"] and abs(float(terms["ssim"]) - ref[2]) <= BOUND_W["value"]
    assert terms["weight_sum"].shape == () and abs(float(terms["weight_sum"]) - ref[3]) <= BOUND_W["value"] * ref[3]
    out, G, GE = _call_weighted(tx, ty, 0.2, (a, b), True, tm, tE, True)
    assert torch.equal(_bits(out[0]), _bits(value)) and not G[a:].any() and not G[:, b:].any()
    tx.requires_grad_(True)
    tE.requires_grad_(True)
    terms2 = {}
    loss = photometric_loss(tx, ty, region=(a, b), terms=terms2, weight=tm, exposure=tE)
    assert loss.requires_grad and torch.equal(_bits(loss), _bits(value)) and torch.equal(terms2["ssim"], terms["ssim"])
    with torch.no_grad():
        assert not photometric_loss(tx, ty, region=(a, b), weight=tm, exposure=tE).requires_grad
    (3.0 * loss).backward()
    assert torch.equal(_bits(tx.grad), _bits(3.0 * G)) and torch.equal(_bits(tE.grad), _bits(3.0 * GE))
    assert wr.rel_max(tx.grad.cpu().numpy()[:a, :b] / 3.0, ref_grad) <= BOUND_W["grad"]
    assert wr.rel_max(tE.grad.cpu().numpy() / 3.0, ref_grad_e) <= BOUND_W["grad_exposure"]
    # an exposure that requires grad under a frame that does not: dL/dexposure alone
    tE.grad = None
    photometric_loss(tx.detach(), ty, region=(a, b), weight=tm, exposure=tE).backward()
    assert torch.equal(_bits(tE.grad), _bits(GE))
    # without the two arguments the plain entry is the one called: its three terms, no weight_sum
    terms3 = {}
    photometric_loss(tx.detach(), ty, region=(a, b), terms=terms3)
    assert sorted(terms3) == ["l1", "ssim"]


def test_l1_alone_under_a_binary_mask_leaves_exact_zeros_on_masked_pixels():
    from intro_to_gaussian_splatting_amd import photometric_loss

    name = "halo_across_a_neighbour_binary_general"
    x, y, m, _ = wr.case_inputs(name)
    assert set(np.unique(m)) == {0.0, 1.0}
    tx, ty, tm = (torch.from_numpy(v).to(DEV) for v in (x, y, m))
    tx.requires_grad_(True)
    photometric_loss(tx, ty, lambda_dssim=0.0, weight=tm).backward()
    g = tx.grad.cpu().numpy()
    assert not g[m == 0].any() and (g[m == 1] != 0).any()
    want = np.float32(1.0 / (3.0 * float(m.sum()))) * np.sign(x.astype(np.float64) - y.astype(np.float64)).astype(np.float32)
    assert np.array_equal(g[m == 1], want[m == 1])        # exact: sign(x - y) / (3 W)


def test_python_surface_refusals_on_the_device():
    from intro_to_gaussian_splatting_amd import photometric_loss

    x, y = torch.zeros((8, 6, 3), device=DEV), torch.zeros((8, 6, 3), device=DEV)
    with pytest.raises(ValueError, match="weight is on cpu"):
        photometric_loss(x, y, weight=torch.ones((8, 6)))
    with pytest.raises(ValueError, match="exposure is on cpu"):
        photometric_loss(x, y, exposure=torch.eye(3, 4))
    with pytest.raises(ValueError, match="weight must have shape"):
        photometric_loss(x, y, region=(4, 4), weight=torch.ones((4, 4), device=DEV))     # the frame's axes, not the region's
    assert photometric_loss(x, y, weight=torch.ones((8, 6), device=DEV), exposure=torch.eye(3, 4, device=DEV)).shape == ()


# ---- end to end: synthetic, 64 x 48, n = 300
def _exposed_scene(path):
    """(scene; targets {1: gain * frame + offset with a rectangle of noise}; masks {1: 0 on the rectangle, 1 elsewhere})."""
    path.mkdir(exist_ok=True)
    scene = _golden_scene(path, load_golden("grad_small_64x48_n300"))
    assert scene.rendered_region(1) == (48, 32)
    rs = np.random.RandomState(11)
    with torch.no_grad():
        frame0 = scene.render_image_hip(1).clone()
        gain = torch.tensor([1.25, 0.8, 1.1], device=DEV)
        offset = torch.tensor([0.05, -0.03, 0.02], device=DEV)
        target = (frame0 * gain + offset).contiguous()
        target[10:22, 8:20] = torch.from_numpy(rs.uniform(size=(12, 12, 3)).astype(np.float32)).to(DEV)
        mask = torch.ones(frame0.shape[:2], device=DEV)
        mask[10:22, 8:20] = 0.0
    return scene, {1: target}, {1: mask}


def test_thirty_exposure_steps_with_the_gaussians_frozen_lower_the_loss(tmp_path):
    from intro_to_gaussian_splatting_amd import ExposureRefiner

    scene, targets, masks = _exposed_scene(tmp_path / "s")
    refiner = ExposureRefiner(scene, [1], lr=0.01)
    with torch.no_grad():
        frame = scene.render_image_hip(1).clone()
    losses = []
    for _ in range(30):
        loss = scene.photometric_loss(1, frame, targets[1], weight=masks[1], exposure=refiner.exposure(1))
        loss.backward()
        assert refiner.step() == 1
        losses.append(loss.detach())
    losses = [float(v) for v in losses]
    print("weighted loss under a learned exposure: first %.6g, last %.6g" % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]
    assert not torch.equal(refiner.exposure(1).detach(), torch.eye(3, 4, device=DEV)) and refiner.steps[1] == 30


LR = {"points": 2e-4, "scales": 2e-3, "quaternions": 1e-3, "opacity": 2e-2, "colors": 5e-3}
DENSITY = dict(grad_threshold=2e-5, dense_scale=0.05, prune_logit=-4.5)


def test_trainer_with_masks_and_exposure_is_the_composition_written_out(tmp_path):
    from intro_to_gaussian_splatting_amd import DensityControl, ExposureRefiner, GaussianAdam, Trainer

    steps, seed = 3, 5
    periods = dict(sh_degree_every=None, densify_every=None, opacity_reset_every=None)
    scene, targets, masks = _exposed_scene(tmp_path / "a")
    trainer = Trainer(scene, targets, lr=LR, lambda_dssim=0.2, tile_size=16, statistic="screen", density=DENSITY, seed=seed,
                      masks=masks, exposure=dict(lr=0.01), **periods)
    assert isinstance(trainer.exposure_refiner, ExposureRefiner) and trainer.exposure_refiner.indices == [1]
    seen = []
    trainer.fit(steps, callback=lambda t, losses, idx: seen.append((losses, idx)))

    scene2, targets2, masks2 = _exposed_scene(tmp_path / "b")
    g = scene2.gaussians
    for name in LR:
        getattr(g, name).requires_grad_(True)
    opt = GaussianAdam(g, lr=LR)
    dc = DensityControl(g, optimizer=opt, scene=scene2, statistic="screen", **DENSITY)
    refiner = ExposureRefiner(scene2, [1], lr=0.01)
    by_hand = []
    for _ in range(steps):
        terms = {}
        frame = scene2.render_image_hip(1, tile_size=16, geometry_gradients=True, screen_statistics=True)
        loss = scene2.photometric_loss(1, frame, targets2[1], tile_size=16, lambda_dssim=0.2, terms=terms, weight=masks2[1],
                                       exposure=refiner.exposure(1))
        loss.backward()
        dc.accumulate()
        opt.step()
        opt.zero_grad()
        refiner.step()
        by_hand.append((torch.stack((loss.detach(), terms["l1"], terms["ssim"])), 1))
    assert [v[1] for v in seen] == [v[1] for v in by_hand]
    assert all(torch.equal(_bits(a[0]), _bits(b[0])) for a, b in zip(seen, by_hand))
    for name in LR:
        assert torch.equal(_bits(getattr(trainer.gaussians, name)), _bits(getattr(g, name))), name
        assert torch.equal(_bits(trainer.opt.exp_avg[name]), _bits(opt.exp_avg[name])), name
    assert torch.equal(_bits(trainer.exposure_refiner.exposure(1)), _bits(refiner.exposure(1)))
    assert not torch.equal(refiner.exposure(1).detach(), torch.eye(3, 4, device=DEV))
    # evaluate(): the weighted terms, and the PSNR of the exposure-corrected frame under the mask
    report = trainer.evaluate()[1]
    with torch.no_grad():
        a, b = scene.rendered_region(1, 16)
        E = trainer.exposure_refiner.exposure(1).detach()
        shown = scene.render_image_hip(1, tile_size=16)[:a, :b] @ E[:, :3].t() + E[:, 3]
        m = masks[1][:a, :b]
        mse = float((m[..., None] * (shown - targets[1][:a, :b]) ** 2).sum() / (3 * m.sum()))
    assert abs(report["psnr"] - (-10.0 * np.log10(mse))) <= 1e-3 and 0 < report["ssim"] <= 1 and report["l1"] > 0
