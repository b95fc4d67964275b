"""Anti-aliased std_3dgs frames on the GPU (GSX_FLAG_ANTIALIASED through ``render_image_hip(semantics="std_3dgs",
antialiased=True)``, gsx_render_backward_std and gsx_render_contribution), held to tests/antialias_restatement.py.

Forward: every pixel decided within BOUND = 12 E_REF (tests/test_rule_sets_host.py) of the float64 walk on the float32
mirror's records, or an ambiguous pixel within BOUND of one of its alternatives, nothing left out -- and the count bar of
tests/test_hip_std3dgs.py against the walk's colour.  The opacity the kernel packs is the mirror's bit for bit: the library
exports no record, so it is read through one-Gaussian frames whose Gaussian sits on a pixel, with sigmoid(logit) = 1, unit
colour and a black background -- the pixel IS op_eff = rho.

Backward: colors, opacity, points, scales, quaternions, means2d per Gaussian within BOUND_AA = 12 E_REF_AA of the float64
restatement (tests/test_antialias_host.py measures E_REF_AA from the float32 mirror), dL/dframe the seeded random image times
the gradient mask.  Every case here has fx = fy and the Treehill or identity pose; unequal focal lengths and far poses are in
tests/test_hip_camera_cases.py (STD_CAMERA_CASES, the four that are not off axis).

Measured on an MI355X.  Frames: worst decided pixel 2.78e-07 (random_64x64_n800_t2; bound 5.39e-06), two ambiguous pixels in
all the cases together (random_130x70_n1500_t8, 9.8e-08 from an alternative), nothing left out, no pixel beyond 1e-4; every
probe's centre pixel equal to the mirror's rho bit for bit, the three on the floor 0.005f.  Gradients, kernel vs restatement,
worst error / scale per case:
  case                      colors     opacity    points     scales     quaternions  means2d
  stack_half_16x16          6.18e-09   9.82e-10   4.16e-11   3.12e-11   0            2.75e-10
  ring_40x24                1.54e-08   4.96e-09   3.14e-09   5.71e-10   0            4.37e-09
  random_64x64_n800_t2      7.36e-08   1.17e-08   4.55e-09   9.46e-10   5.29e-11     1.07e-08
  random_130x70_n1500_t8    5.35e-08   9.64e-09   3.43e-09   1.54e-09   1.24e-10     8.67e-09
  subpixel_32x32            3.90e-07   5.00e-08   3.41e-08   8.84e-09   2.40e-10     5.09e-08
  needle_48x48              1.30e-07   2.11e-08   1.05e-08   3.42e-07   6.95e-10     1.58e-08
  BOUND_AA = 12 E_REF_AA    4.68e-06   4.74e-07   2.96e-07   4.11e-06   8.23e-09     4.58e-07
(the needles' scales: 3.42e-07, the mirror's own figure -- kernel and mirror divide by the same float32 det0 -- against
1.5e-09 on the random scenes; the stack and the ring hold identity quaternions and isotropic scales.)
The coarser frame: mean over black at 64x64 / 16x16 0.04685 / 0.04081 with the flag, 0.11285 / 0.46222 without.
"""
import numpy as np
import pytest
import torch

import antialias_restatement as aar
import std3dgs_backward_restatement as sbr
from test_antialias_host import BACKWARD_CASES, BOUND_AA, IDENTITY, backward_case, build_case, forward_case
from test_hip_backward import DEV, _scene
from test_hip_parity import _oracle_cam
from test_hip_rule_sets import _judge, _same_camera
from test_rule_sets_host import BOUND

pytestmark = pytest.mark.gpu

KEYS = aar.KEYS
FORWARD_CASES = ["stack_half_16x16", "ring_40x24", "random_64x64_n800_t2", "random_130x70_n1500_t8", "subpixel_32x32",
                 "needle_48x48"]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _make(tmp_path, case):
    """The scene of a case; the case again on the scene object's own camera where that rounds differently."""
    scene = _scene(tmp_path, case["sc"], colors=case["colors"])
    gcam = _oracle_cam(scene)
    if not _same_camera(case["cam"], gcam):
        print("walking the scene object's own camera")
        case = build_case(case["sc"], case["tile"], case["bg"], cam=gcam, colors=case["colors"])
    return case, scene


def _frame(scene, case, layout="hw3", **kw):
    st = {}
    with torch.no_grad():
        img = scene.render_image_hip(1, tile_size=case["tile"], layout=layout, semantics="std_3dgs", background=case["bg"],
                                     stats=st, **kw)
    return img, st


def _count_bar(img, wk, what):
    """tests/test_hip_std3dgs.py's bar, against the walk's colour: pixels beyond 1e-4 are rare and bounded."""
    d = np.abs(img.astype(np.float64) - wk.colour).max(axis=-1)
    bad = int((d > 1e-4).sum())
    assert bad <= 2 + int(1e-5 * d.size), (what, bad, float(d.max()))
    assert d.max() < 0.006, (what, float(d.max()))


def _hold_frame(tag, case, img_t, st):
    img = img_t.cpu().numpy()
    assert np.isfinite(img).all(), tag
    assert st["n_visible"] == case["nvis"], tag
    _judge(tag, case["fwd"].wk, img, BOUND["std_3dgs"])
    _count_bar(img, case["fwd"].wk, tag)


# ---------------------------------------------------------------------------------------------- 1, 4: the frame

@pytest.mark.parametrize("name", FORWARD_CASES)
def test_the_frame_is_the_walk_on_the_mirrors_records(tmp_path, name):
    case, scene = _make(tmp_path, forward_case(name))
    img, st = _frame(scene, case, antialiased=True, published_rects=True)
    assert tuple(img.shape) == (case["H"], case["W"], 3) and st["n_instances"] == case["inst"]
    _hold_frame("antialiased " + name, case, img, st)
    # the rectangles are the flag-clear frame's (sized by sigmoid(logit)): the same pairs, tight or published
    plain, st0 = _frame(scene, case)
    tight, st1 = _frame(scene, case, antialiased=True)
    assert torch.equal(tight, img) and st1["n_instances"] == st0["n_instances"] <= case["inst"]
    assert not torch.equal(plain, img)
    # every other route: the same bits
    assert torch.equal(_frame(scene, case, antialiased=True, generic_kernels=True)[0], img)
    assert torch.equal(_frame(scene, case, layout="wh3", antialiased=True)[0].permute(1, 0, 2), img)


PROBES = [  # scales in pixels at z = 4 (sigma along x, y, z), rotation about the view axis
    ((2.0, 2.0, 2.0), 0.0), ((0.6, 0.6, 0.6), 0.0), ((0.25, 0.4, 0.3), 0.7), ((3.0, 0.03, 0.03), 0.5), ((1.2, 0.1, 5.0), 2.1),
    ((0.02, 0.02, 0.02), 0.0), ((0.5, 0.0001, 0.0001), 0.8), ((0.02, 0.03, 0.01), 1.3)]


@pytest.mark.parametrize("k", range(len(PROBES)))
def test_the_packed_opacity_is_the_mirrors_bit_for_bit(tmp_path, k):
    """One Gaussian on the centre pixel of a 33x33 frame, sigmoid(20) = 1 in float32, colour 1, black background: the centre
    pixel is op_eff = rho, the bits the record holds.  The last three probes sit on the floor: 0.005f exactly."""
    from oracle import std3dgs_ref

    (sx, sy, sz), angle = PROBES[k]
    w = h = 33
    fx = 24.0
    z = 4.0
    sc = dict(points=np.array([[0.0, 0.0, z]], np.float32), colors_0_255=np.array([[256.0, 256.0, 256.0]], np.float32),
              scales=(np.array([[sx, sy, sz]]) * z / fx).astype(np.float32),
              quaternions=np.array([[np.cos(angle / 2), 0.0, 0.0, np.sin(angle / 2)]], np.float32),
              opacity=np.array([[20.0]], np.float32), fx=np.float64(fx), fy=np.float64(fx), cx=np.float64(w / 2),
              cy=np.float64(h / 2), width=np.int64(w), height=np.int64(h), **IDENTITY)
    scene = _scene(tmp_path, sc, colors=np.ones((1, 3), np.float32))
    cam = _oracle_cam(scene)
    st1 = std3dgs_ref.stage1(sc["points"], sc["scales"], sc["quaternions"], sc["opacity"], cam, 16)
    assert tuple(st1.xy[0]) == (16.0, 16.0) and st1.opacity[0] == np.float32(1.0)
    fac = aar.factor(*aar.covariance32(sc["points"], sc["scales"], sc["quaternions"], cam))
    rho = fac.rho[0]
    assert np.float32(1.0 / 255.0) <= rho < np.float32(0.99)          # composited, and not the alpha clamp
    assert bool(fac.clamped[0]) == (k >= 5) and (not fac.clamped[0] or rho == np.float32(0.005))
    with torch.no_grad():
        img = scene.render_image_hip(1, layout="hw3", semantics="std_3dgs", antialiased=True)
        plain = scene.render_image_hip(1, layout="hw3", semantics="std_3dgs")
    got = img[16, 16].cpu().numpy()
    print("probe %d: rho mirror %.9g (det0 %.6g, ratio %.6g), kernel %.9g" % (k, rho, fac.det0[0], fac.ratio[0], got[0]))
    assert (got.view(np.int32) == np.float32(rho).view(np.int32)).all(), (k, got, rho)
    assert (plain[16, 16].cpu().numpy() == np.float32(0.99)).all()      # without the flag: sigmoid = 1, clamped at 0.99


# ---------------------------------------------------------------------------------------------- 2, 3, 4: the gradients

def _backward(scene, case, frame, st, gf, geometry=True, screen=True, antialiased=True, std=None):
    std = (case["bg"], False, antialiased) if std is None else std
    return scene._render_backward(1, case["tile"], "hw3", frame, gf, st["n_instances"], st["n_visible"], geometry=geometry,
                                  screen=screen, std=std)


def _errors(ref, outs):
    got = dict(zip(KEYS, (o.cpu().numpy() for o in outs[:6])))
    for k, v in got.items():
        assert np.isfinite(v).all(), k
    return got, {k: sbr.per_gaussian_error(got[k], ref.arrays[k], ref.scales[k]) for k in KEYS}


@pytest.mark.parametrize("name", BACKWARD_CASES)
def test_the_gradients_match_the_restatement(tmp_path, name):
    case = backward_case(name)
    scene = _scene(tmp_path, case["sc"], colors=case["colors"])
    assert _same_camera(case["cam"], _oracle_cam(scene))
    gf = torch.from_numpy(case["g"]).to(DEV)
    frame, st = _frame(scene, case, antialiased=True)
    outs = _backward(scene, case, frame, st, gf)
    assert len(outs) == 7
    got, err = _errors(case["ref"], outs)
    print("%s: kernel vs restatement, max error / scale: %s" % (name, ", ".join("%s %.3g (bound %.3g)" % (k, err[k], BOUND_AA[k])
                                                                                 for k in KEYS)))
    radius, rows = outs[6].cpu().numpy().reshape(-1), case["rows0"]
    listed = radius > 0
    assert listed.any() and np.array_equal(radius[listed], rows[listed, 5])
    assert listed[case["ref"].scales["colors"] > 0].all()
    for o in outs[:6]:
        assert not o.cpu().numpy()[~listed].any()
    # the colour-only and the five-output calls, and a second call: the same bits
    plain = _backward(scene, case, frame, st, gf, geometry=False, screen=False)
    assert len(plain) == 2 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(plain, outs))
    five = _backward(scene, case, frame, st, gf, screen=False)
    again = _backward(scene, case, frame, st, gf)
    assert len(five) == 5 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(five, outs))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, outs))
    # the rows on the floor: the chain without U's rho term (the restatement's clamp branch), dL/dlogit still U (1 - sigmoid)
    clamped = case["fwd"].fac32.clamped & listed
    if clamped.any():
        sc = case["sc"]
        bare = aar.backward(case["fwd"], case["dec"], sc["points"], sc["scales"], sc["quaternions"], case["cam"], case["g"],
                            case["bg"], with_rho=False)
        for k in ("points", "scales", "quaternions", "opacity"):
            assert np.array_equal(bare.arrays[k][clamped], case["ref"].arrays[k][clamped])
            e = sbr.per_gaussian_error(got[k][clamped], bare.arrays[k][clamped], case["ref"].scales[k][clamped])
            assert e <= BOUND_AA[k], (name, "clamped rows", k, e)
        assert np.abs(got["opacity"][clamped]).max() > 0 and np.abs(got["scales"][clamped]).max() > 0
    for k in KEYS:
        assert err[k] <= BOUND_AA[k], (name, k, err[k])


# ---------------------------------------------------------------------------------------------- 5: flag off is today

@pytest.mark.parametrize("name", ["ring_40x24", "needle_48x48"])
def test_the_flag_clear_calls_keep_their_bits(tmp_path, name):
    case = backward_case(name)
    scene = _scene(tmp_path, case["sc"], colors=case["colors"])
    gf = torch.from_numpy(case["g"]).to(DEV)
    frame, st = _frame(scene, case)
    off, st_off = _frame(scene, case, antialiased=False)
    on, _ = _frame(scene, case, antialiased=True)
    assert torch.equal(_bits(off), _bits(frame)) and st_off["n_instances"] == st["n_instances"]
    assert not torch.equal(on, frame)
    a = _backward(scene, case, frame, st, gf, std=(case["bg"], False))              # the argument not passed at all
    b = _backward(scene, case, frame, st, gf, antialiased=False)
    assert len(a) == len(b) == 7 and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    c = _backward(scene, case, on, st, gf)
    assert not torch.equal(c[1], a[1]) and not torch.equal(c[3], a[3])
    con = scene.render_contribution_hip(1, semantics="std_3dgs", tile_size=case["tile"])
    con_off = scene.render_contribution_hip(1, semantics="std_3dgs", tile_size=case["tile"], antialiased=False)
    con_on = scene.render_contribution_hip(1, semantics="std_3dgs", tile_size=case["tile"], antialiased=True)
    for x, y in zip(con, con_off):
        assert torch.equal(_bits(x), _bits(y))
    assert not torch.equal(con_on.weight_sum, con.weight_sum)


# ---------------------------------------------------------------------------------------------- 6: what it is for

def test_a_coarser_frame_keeps_its_brightness_with_the_flag(tmp_path):
    """Small Gaussians at 64x64 and, with the same field of view, at 16x16.  Dilation alone widens them and keeps their
    peak, so the coarse frame comes out brighter; with the compensation its mean stays closer to the fine frame's."""
    mean = {}
    for size in (64, 16):
        (tmp_path / str(size)).mkdir()
        case, scene = _make(tmp_path / str(size), forward_case("small_%dx%d" % (size, size)))
        on, st = _frame(scene, case, antialiased=True)
        _hold_frame("antialiased small %d" % size, case, on, st)
        off, _ = _frame(scene, case)
        black = dict(case, bg=(0.0, 0.0, 0.0))
        mean[size] = (float(_frame(scene, black, antialiased=True)[0].double().mean()), float(_frame(scene, black)[0].double().mean()))
        assert not torch.equal(on, off)
    print("mean of the frame over black, antialiased / not: 64x64 %.5f / %.5f, 16x16 %.5f / %.5f" % (mean[64] + mean[16]))
    assert abs(mean[16][0] - mean[64][0]) < abs(mean[16][1] - mean[64][1])


# ---------------------------------------------------------------------------------------------- 7: contribution

def test_weight_sum_is_the_colour_gradient_of_the_summed_frame(tmp_path):
    case = backward_case("random_130x70_n1500_t8")
    scene = _scene(tmp_path, case["sc"], colors=case["colors"])
    g = scene.gaussians
    g.colors.requires_grad_(True)
    frame = scene.render_image_hip(1, tile_size=case["tile"], semantics="std_3dgs", background=case["bg"], antialiased=True)
    assert frame.grad_fn is not None
    frame.sum().backward()
    want = g.colors.grad[:, 0].detach().clone()
    g.colors.requires_grad_(False)
    g.colors.grad = None
    con = scene.render_contribution_hip(1, semantics="std_3dgs", tile_size=case["tile"], antialiased=True)
    assert want.abs().max() > 0 and torch.equal(_bits(con.weight_sum), _bits(want))
    plain = scene.render_contribution_hip(1, semantics="std_3dgs", tile_size=case["tile"])
    assert not torch.equal(plain.weight_sum, con.weight_sum)
    swept = scene.contribution([1], semantics="std_3dgs", tile_size=case["tile"], antialiased=True)
    assert torch.equal(_bits(swept.weight_sum), _bits(con.weight_sum))


# ---------------------------------------------------------------------------------------------- 8: refusals

def test_the_refusals_raise_by_name_and_the_view_keys_tell_the_modes_apart(tmp_path):
    import ctypes

    from intro_to_gaussian_splatting_amd import _ffi
    from intro_to_gaussian_splatting_amd._device import _WORKSPACE, _ptr, _stream_handle

    case = forward_case("stack_half_16x16")
    scene = _scene(tmp_path, case["sc"], colors=case["colors"])
    g = scene.gaussians
    for sem in ("ref_cpu", "ref_cuda"):
        with pytest.raises(ValueError, match="antialiased=True needs semantics='std_3dgs'"):
            scene.render_image_hip(1, semantics=sem, antialiased=True)
    g.colors.requires_grad_(True)
    g.points.requires_grad_(True)
    kw = dict(tile_size=16, semantics="std_3dgs", background=case["bg"], geometry_gradients=True, antialiased=True)
    with pytest.raises(ValueError, match="antialiased=True.*camera_gradients"):
        scene.render_image_hip(1, camera_gradients=True, **kw)
    with pytest.raises(ValueError, match="antialiased=True.*screen_statistics='abs'"):
        scene.render_image_hip(1, screen_statistics="abs", **kw)
    assert scene.render_image_hip(1, **kw).grad_fn is not None
    g.colors.requires_grad_(False)
    g.points.requires_grad_(False)
    # the depth image: its Python call renders the ref_cpu frame and has no such argument; the entry refuses the flag by name
    lib = _ffi.load()
    dev, n, tensors = scene._inputs(1)
    cam = scene.images[1].gsx_camera()
    for sem in ("std_3dgs", "ref_cpu"):
        params, _ = scene._frame_params(dev, n, "wh3", sem)
        params.flags |= _ffi.GSX_FLAG_ANTIALIASED
        out = torch.zeros((16, 16, 2), dtype=torch.float32, device=DEV)
        with torch.cuda.device(dev):
            nbytes = lib.gsx_depth_workspace_bytes(n, cam.width, cam.height, 16, 8192)
            ws = _WORKSPACE.get(dev, nbytes)
            rc = lib.gsx_render_depth(ctypes.byref(cam), *[_ptr(t.detach()) for t in tensors], n, 16, _ptr(out),
                                      ctypes.byref(params), _ptr(ws), nbytes, _stream_handle(dev))
        assert rc == _ffi.GSX_ERR_INVALID_ARGUMENT and b"GSX_FLAG_ANTIALIASED" in lib.gsx_last_error()
        assert not out.any()
    # capacity hints and hint slots are kept per mode
    with torch.no_grad():
        scene.render_image_hip(1, semantics="std_3dgs")
        scene.render_image_hip(1, semantics="std_3dgs", antialiased=True)
    keys = [k[3] for k in scene._cap_hints]
    assert "std_3dgs" in keys and "std_3dgs/antialiased" in keys
    # a captured frame bakes the mode in
    with torch.no_grad():
        want = scene.render_image_hip(1, semantics="std_3dgs", antialiased=True).clone()
    cap = scene.capture_frame(1, semantics="std_3dgs", antialiased=True)
    cap.replay()
    assert torch.equal(cap.confirm(), want) and cap._call["antialiased"] is True


# ---------------------------------------------------------------------------------------------- 9: Trainer

def test_trainer_with_the_flag_is_the_composition_written_out(tmp_path):
    from intro_to_gaussian_splatting_amd import DensityControl, GaussianAdam, Trainer
    from test_hip_std3dgs_backward import DENSITY, FIT_BG, LR, _fit_scene, _state

    steps, seed = 4, 5
    periods = dict(sh_degree_every=None, densify_every=2, opacity_reset_every=None, densify_from=0, densify_until=100)
    scene, targets = _fit_scene(tmp_path / "a", 1)
    trainer = Trainer(scene, targets, lr=LR, lambda_dssim=0.2, tile_size=16, statistic="screen", density=DENSITY, seed=seed,
                      semantics="std_3dgs", background=FIT_BG, antialiased=True, prune_contribution_at=[3],
                      prune_contribution=dict(threshold=0.02), **periods)
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
                                        semantics="std_3dgs", background=FIT_BG, antialiased=True)
        loss = scene2.photometric_loss(idx, frame, targets2[idx], tile_size=16, lambda_dssim=0.2, terms=terms,
                                       semantics="std_3dgs")
        loss.backward()
        dc.accumulate()
        opt.step()
        opt.zero_grad()
        if s % 2 == 0:
            dc.densify_and_prune(generator=split)
        if s == 3:
            dc.prune_contribution(scene2.contribution(None, semantics="std_3dgs", tile_size=16, antialiased=True), threshold=0.02)
        by_hand.append((torch.stack((loss.detach(), terms["l1"], terms["ssim"])), idx, len(g)))
    print("views and rows per step", [v[1:] for v in seen])
    assert [v[1:] for v in seen] == [v[1:] for v in by_hand]
    assert all(torch.equal(_bits(a[0]), _bits(b[0])) for a, b in zip(seen, by_hand))
    got, want = _state(trainer.gaussians, trainer.opt), _state(g, opt)
    for key in want:
        assert torch.equal(_bits(got[key]), _bits(want[key])), key
    # and it is not the flag-clear fit
    scene3, targets3 = _fit_scene(tmp_path / "c", 1)
    other = Trainer(scene3, targets3, lr=LR, lambda_dssim=0.2, tile_size=16, statistic="screen", density=DENSITY, seed=seed,
                    semantics="std_3dgs", background=FIT_BG, **periods)
    first = other.step()[0]
    assert not torch.equal(first, seen[0][0])
    # evaluate() renders with the flag
    ev = trainer.evaluate()
    with torch.no_grad():
        frame = scene.render_image_hip(1, semantics="std_3dgs", background=FIT_BG, antialiased=True)
        mse = ((frame - targets[1]) ** 2).mean()
    assert ev[1]["psnr"] == pytest.approx(-10.0 * np.log10(float(mse)), rel=1e-5)
