"""The frame and its gradients on the GPU at the cameras of tests/camera_cases.py: unequal focal lengths (fx / fy = 0.65,
2.33, 0.69), a pose 140 degrees about an oblique axis, a pose with R00, R11 < 0.  Every other gradient test sees
fx = fy = 0.75 width and the Treehill pose, where an fx written for an fy in csrc/gsx_backward.hip's geometry_chain, or a
transposed contraction with world2view, changes nothing.

The checks are the sibling files' own (their _check functions, error units and bounds): the five gradients per Gaussian,
the camera entry's two matrices, the depth entry, the screen and abs statistics, each against its float64 restatement and,
where the reference was captured (tests/golden/*_cam_*.npz), against the reference's own autograd.  Bounds
(tests/test_camera_cases_host.py): E_REF_CAM, the reference's own error at these cameras, is below the sibling file's E_REF
for every output but two (the geometry's dL/dpoints and the depth entry's dL/dopacity), so 12 max(E_REF, E_REF_CAM) and
13 max(E_REF, E_REF_CAM) are the sibling files' 12 E_REF and 13 E_REF, which their checks apply here too: for those two
outputs that is tighter than this file would have to be.  Colours and opacity logits are held to test_backward_host.py's TOL
per Gaussian.

Worst error / scale measured on an MI355X over the tests of this file (24 tests, 4.4 s in all), and the scene that sets it:
                                against the restatement                    against the reference's autograd
    geometry     points         1.135e-07  (aniso fixture)                 1.167e-07  (aniso)        bounds 2.61e-07, 2.82e-07
                 scales         6.689e-08  (aniso fixture)                 5.989e-08  (aniso)               5.62e-06, 6.09e-06
                 quaternions    4.796e-09  (aniso fixture)                 5.690e-09  (aniso)               4.55e-08, 4.93e-08
                 colours        1.656e-06  (farpose, 350 Gaussians)        1.502e-06  (farpose)             8e-06
                 opacity        7.543e-07  (aniso fixture)                 7.630e-07  (aniso)               8e-06
    camera       world2view     7.815e-11  (roll fixture)                  1.097e-10  (aniso_tall)          3.49e-08, 3.79e-08
                 full_proj      3.729e-10  (aniso_tall fixture)            7.515e-10  (aniso_tall)          6.64e-08, 7.19e-08
    depth        points         4.833e-09  scales 1.157e-08  quaternions 3.210e-10  colors 3.944e-07  opacity 1.218e-07  (all roll;
                 against the autograd 5.914e-09, 1.177e-08, 3.722e-10, 4.056e-07, 1.171e-07; opacity bounds 5.83e-07, 6.32e-07)
                 maps           |dD| / z_listed 1.2e-07, |dA| 2.1e-07 (roll); against the composed frame 1.7e-07, 2.4e-07
    screen                      7.526e-08  (roll)                          8.700e-08  (roll)                5.17e-07, 5.60e-07
    abs                         7.745e-08  (roll)                          9.223e-08  (roll)                3.53e-07, 3.82e-07
    frames against the C oracle: at most 2.98e-07 (bound 1e-4)
The aniso fixture's footprints are a quarter of the usual size (it carries the floored determinant), which is why it leads,
as tiny_48x48_n600 leads the sibling files; at the usual footprints every figure is 20 to 1000 times inside its bound.  No
case exceeded its bound: no kernel defect was found at these cameras.

That the file could have seen one, once and not committed: with cam.fx written for cam.fy where geometry_chain forms g_cy,
13 of the 24 tests fail -- every geometry, camera-entry and depth case at aniso, aniso_tall and roll (dL/dpoints off by 1.5e-04
.. 1.2e-03 of its scale against a bound of 2.61e-07) -- the farpose cases (fx = fy) pass, and all 31 tests of
tests/test_hip_geometry_backward.py pass as if nothing had happened.

The std_3dgs rule set (second half of the file).  Its route shares no camera term with the one above: geo_camera_std and
project_std derive fx = width / (2 tan_fovx), fy = height / (2 tan_fovy) themselves, and the kStd / kAa instances of
geometry_chain add h3 + 1e-7, the c10 = c01 merge and the rho term.  The six cases of camera_cases.STD_CAMERA_CASES (3072
pixels, at most 612 instances; two with the EWA clamp's gradient branch at limx != limy), the four that are not off axis also
anti-aliased.  The checks and bounds are the sibling files' own and unchanged -- the frame by rule_set_restatement's classify
at BOUND = 12 E_REF (tests/test_rule_sets_host.py), the gradients at BOUND = 12 E_REF (tests/test_std3dgs_backward_host.py)
and BOUND_AA = 12 E_REF_AA (tests/test_antialias_host.py), the contribution at tests/test_hip_contribution.py's TOL, the SH
link at tests/test_sh_backward_host.py's BOUND -- and tests/test_std3dgs_camera_cases_host.py asserts on the CPU that the
float32 mirror's own error on these cases stays within the recorded E_REF / E_REF_AA.  The scene object rounds tan_fovx of
aniso and roll one bit away from cpu_ref.build_camera: those cases are walked on the scene object's own camera.

Measured on an MI355X (23 tests, 4.8 s in all), kernel vs restatement, worst error / scale per case; published rectangles
give the same figures to the last printed digit:
  std_3dgs                             frame      colors     opacity    points     scales     quaternions  means2d
  std_aniso_64x48_n120                 1.47e-07   3.02e-08   5.69e-09   1.69e-09   8.26e-10   9.41e-11     3.83e-09
  std_aniso_tall_48x64_n100            1.22e-07   2.73e-08   1.29e-08   3.35e-09   2.74e-09   1.24e-10     7.41e-09
  std_farpose_64x48_n120               1.29e-07   2.95e-08   6.03e-09   2.34e-09   8.80e-10   4.67e-11     4.62e-09
  std_roll_64x48_n100                  1.30e-07   2.47e-08   5.75e-09   2.91e-09   1.19e-09   5.92e-11     4.82e-09
  std_offaxis_aniso_tall_48x64_n100    1.15e-07   6.27e-08   1.18e-08   6.57e-10   6.62e-10   4.23e-11     1.27e-08
  std_offaxis_roll_64x48_n100          2.31e-07   6.34e-08   2.48e-09   9.72e-10   1.47e-09   4.84e-11     5.72e-09
  BOUND = 12 E_REF                     5.39e-06   7.95e-06   1.91e-07   1.72e-07   7.37e-08   3.40e-09     3.12e-07
  anti-aliased
  std_aniso_64x48_n120                 1.29e-07   4.87e-08   1.36e-08   1.01e-09   5.75e-10   2.94e-11     4.98e-09
  std_aniso_tall_48x64_n100            1.01e-07   3.05e-08   1.09e-08   3.90e-09   7.29e-10   6.25e-11     7.38e-09
  std_farpose_64x48_n120               1.30e-07   2.72e-08   5.81e-09   1.93e-09   4.80e-10   4.00e-11     4.31e-09
  std_roll_64x48_n100                  1.45e-07   3.30e-08   9.71e-09   4.49e-09   7.82e-10   2.22e-11     6.82e-09
  BOUND_AA = 12 E_REF_AA               5.39e-06   4.68e-06   4.74e-07   2.96e-07   4.11e-06   8.23e-09     4.58e-07
(frame: the worst decided pixel; no frame has an ambiguous pixel, nothing is left out.)  The twelve probes' pixels are the
mirror's rho bit for bit, the four on the floor 0.005f.  Contribution: |weight_max - restatement| 6.84e-08 (roll), 7.78e-08
(offaxis_aniso_tall), bound 1e-4; weight_sum the backward's bits.  SH link at the roll camera's centre: sh 3.86e-07 (bound
8.31e-06), points 1.16e-07 (bound 4.61e-06).  Every figure is at least 14 times inside its bound: no kernel defect was found
under this rule set at these cameras.  The deliberately wrong scratch builds these tests caught are in
docs/lab_notes/std_camera_cases.md.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden

import abs_gradient_restatement as agr
import antialias_restatement as aar
import backward_restatement
import camera_cases as cc
import contribution_restatement as cr
import geometry_backward_restatement as gbr
import screen_gradient_restatement as sgr
import sh_backward_restatement as shr
import std3dgs_backward_restatement as sbr
import test_abs_statistic_host as abs_host
import test_antialias_host as aa_host
import test_hip_antialias as hip_aa
import test_hip_contribution as hip_con
import test_hip_std3dgs_backward as hip_std
import test_screen_statistic_host as screen_host
import test_sh_backward_host as sh_host
import test_std3dgs_backward_host as std_host
import test_std3dgs_camera_cases_host as std_cam
from test_backward_host import REL, TOL
from test_depth_host import depth_fixture
from test_hip_abs_statistic import _abs_grads
from test_hip_backward import DEV, _golden_scene, _oracle_pre, _scene
from test_hip_camera_gradient import _bits, _entry, _restate, _same, camera_centre_share
from test_hip_camera_gradient import _check as _check_camera
from test_hip_depth import _check as _check_depth
from test_hip_depth import _check_maps, _depth_grads
from test_hip_geometry_backward import _W, _all_grads, _camera
from test_hip_geometry_backward import _check as _check_geometry
from test_hip_parity import _oracle_cam
from test_hip_rule_sets import _judge, _same_camera
from test_hip_screen_statistic import FIVE, _screen_grads
from test_hip_sh_backward import _sh_for, carried_one_link_further
from test_rule_sets_host import BOUND as FRAME_BOUND

pytestmark = pytest.mark.gpu

PIXEL_TOL = 1e-4            # test_hip_parity.py's
# camera -> the synthetic scene held against the restatement: 350 Gaussians in the camera's own frustum
SYNTHETIC = {
    "aniso": dict(seed=201),
    "aniso_tall": dict(seed=202, spread=2.0, sigma_scale=4.0),      # the clamp, with limx != limy
    "farpose": dict(seed=203, behind_fraction=0.25),                # culled rows
    "roll": dict(seed=204),
}
N_SYNTHETIC = 350


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _sc(base):
    return {k: base[k] for k in ("points", "scales", "quaternions", "opacity", "width", "height")}


def _synthetic(name, **more):
    return cc.scene(name, N_SYNTHETIC, **dict(SYNTHETIC[name], **more))


def _check_colours(scene, sc, frame, W, tile, grads, tag, fixture=None):
    """dL/dcolours and dL/dopacity per Gaussian against backward_restatement (TOL of the Gaussian's own scale) and, with
    `fixture`, against the reference's autograd (the same unit, and test_hip_backward.py's max-normalised REL)."""
    n = sc["points"].shape[0]
    w, h = int(sc["width"]), int(sc["height"])
    gc, go, scale_c, scale_o = backward_restatement.backward(_oracle_pre(scene, sc), _np(frame), _np(W), w, h, tile, n, with_scale=True)
    got_c, got_o = _np(grads["colors"]).astype(np.float64), _np(grads["opacity"]).astype(np.float64)
    ec, eo = backward_restatement.per_gaussian_error(got_c, got_o, gc, go, scale_c, scale_o)
    line = "%s: colours, opacity: kernel vs restatement, max error / scale %.4g, %.4g (bound %.3g)" % (tag, ec, eo, TOL)
    if fixture is not None:
        fc, fo = backward_restatement.per_gaussian_error(got_c, got_o, fixture["grad_colors"], fixture["grad_opacity"], scale_c, scale_o)
        line += "; vs reference autograd %.4g, %.4g" % (fc, fo)
    print(line)
    assert np.abs(gc).max() > 0 and np.abs(go).max() > 0
    assert ec <= TOL and eo <= TOL, (tag, ec, eo)
    if fixture is not None:
        assert fc <= TOL and fo <= TOL, (tag, fc, fo)
        for got, ref in ((got_c, fixture["grad_colors"]), (got_o, fixture["grad_opacity"])):
            assert np.abs(got - ref).max() <= REL * np.abs(ref).max(), tag


# ---- the frame
@pytest.mark.parametrize("name", cc.NAMES)
def test_frame_matches_the_c_oracle_and_ignores_the_principal_point(tmp_path, name):
    """test_hip_parity.py's criterion per camera; then the same scene with cx, cy off the frame centre: the same bits,
    frame and gradients."""
    from oracle import c_oracle

    sc = _synthetic(name, behind_fraction=0.2)
    w, h = int(sc["width"]), int(sc["height"])
    scene = _scene(tmp_path, sc)
    c = scene.images[1].gsx_camera()
    assert (c.fx, c.fy) == (np.float32(cc.CAMERAS[name]["fx"]), np.float32(cc.CAMERAS[name]["fy"]))
    pre = _oracle_pre(scene, sc)
    ref, _, inst = c_oracle.render(pre, w, h, cc.TILE)
    stats = {}
    with torch.no_grad():
        got = scene.render_image_hip(1, tile_size=cc.TILE, stats=stats).cpu().numpy()
    finite = np.isfinite(ref)
    assert finite.all() and np.array_equal(np.isfinite(got), finite) and ref.max() > 0.1
    err = np.max(np.abs(got - ref))
    print("%s: frame vs C oracle %.3g, %d of %d visible, %d instances" % (name, err, pre.points.shape[0], N_SYNTHETIC, inst))
    assert err <= PIXEL_TOL
    assert stats["n_visible"] == pre.points.shape[0] < N_SYNTHETIC and stats["n_instances"] == inst
    # a principal point off the centre
    (tmp_path / "off").mkdir()
    moved = _scene(tmp_path / "off", cc.off_centre(sc))
    assert float(moved.images[1].c_x) != float(scene.images[1].c_x)
    W = _W((w, h, 3), 7)
    f0, a = _all_grads(scene, W, tile=cc.TILE)
    f1, b = _all_grads(moved, W, tile=cc.TILE)
    assert torch.equal(_bits(f0), _bits(f1))
    for k in a:
        assert a[k].abs().max() > 0 and torch.equal(_bits(a[k]), _bits(b[k])), k


# ---- the five gradients per Gaussian
@pytest.mark.parametrize("name", cc.NAMES)
def test_fixture_scene_gradients_match_reference_and_restatement(tmp_path, name):
    gg = load_golden("geomgrad_" + cc.FIXTURES[name])
    scene = _golden_scene(tmp_path, gg)
    W = torch.from_numpy(gg["W"]).to(DEV)
    tile = int(gg["tile"])
    frame, grads = _all_grads(scene, W, tile=tile)
    assert np.abs(frame.cpu().numpy() - gg["image"]).max() <= PIXEL_TOL
    sc = _sc(gg)
    out = _check_geometry(scene, sc, frame, W, tile, grads, name, fixture=gg)
    _check_colours(scene, sc, frame, W, tile, grads, name, fixture=gg)
    dead = (np.abs(gg["grad_colors"]).sum(1) == 0) & (np.abs(out[0]).sum(1) == 0)      # culled, or on no composited pixel
    for key in FIVE:
        assert not _np(grads[key])[dead].any(), key
    assert dead.sum() >= int(gg["n_culled"]) and (~dead).sum() >= 40


@pytest.mark.parametrize("name", cc.NAMES)
def test_synthetic_scene_gradients_match_restatement(tmp_path, name):
    sc = _synthetic(name)
    w, h = int(sc["width"]), int(sc["height"])
    scene = _scene(tmp_path, sc)
    cam = _camera(scene)
    st = gbr.stage1(sc["points"], sc["scales"], sc["quaternions"], cam)
    front = st["t"][:, 2] >= 0.2
    if name == "aniso_tall":        # both clamps bite, at different limits
        assert cam.tan_fovx != cam.tan_fovy and (~st["inx"] & front).sum() >= 20 and (~st["iny"] & front).sum() >= 20
    if name == "farpose":
        assert 40 <= (~front).sum() <= 140
    W = _W((w, h, 3), 11)
    frame, grads = _all_grads(scene, W, tile=cc.TILE)
    out = _check_geometry(scene, sc, frame, W, cc.TILE, grads, name + " synthetic")
    _check_colours(scene, sc, frame, W, cc.TILE, grads, name + " synthetic")
    graded = np.abs(out[0]).sum(1) > 0
    assert graded.sum() >= N_SYNTHETIC // 4
    if name == "aniso_tall":
        assert (graded & ~st["inx"]).sum() >= 5 and (graded & ~st["iny"]).sum() >= 5       # clamped rows with a gradient
    if name == "farpose":
        for key in FIVE:
            assert not _np(grads[key])[~front].any(), key


@pytest.mark.parametrize("tile", [8, 20])
def test_roll_at_other_tile_sizes_matches_restatement(tmp_path, tile):
    """Tile 8 (a quarter-filled chunk) and tile 20 (400 pixels: two chunks; 64 x 48 is no multiple of it)."""
    sc = _synthetic("roll")
    w, h = int(sc["width"]), int(sc["height"])
    scene = _scene(tmp_path, sc)
    W = _W((w, h, 3), tile)
    frame, grads = _all_grads(scene, W, tile=tile)
    out = _check_geometry(scene, sc, frame, W, tile, grads, "roll tile %d" % tile)
    _check_colours(scene, sc, frame, W, tile, grads, "roll tile %d" % tile)
    assert (np.abs(out[0]).sum(1) > 0).sum() >= N_SYNTHETIC // 4
    gv, gf = _entry(scene, W, tile)[1][-2:]
    _check_camera("roll tile %d" % tile, gv, gf, _restate(scene, sc, frame, W, tile))


# ---- the camera entry
@pytest.mark.parametrize("name", cc.NAMES)
def test_camera_entry_matches_restatement_and_reference(tmp_path, name):
    sc = _synthetic(name)
    scene = _scene(tmp_path, sc)
    W = _W((int(sc["width"]), int(sc["height"]), 3), 13)
    frame, outs, _ = _entry(scene, W, cc.TILE)
    gv, gf = outs[-2], outs[-1]
    assert gv.shape == gf.shape == (4, 4)
    # no zero of R hides an entry at these cameras: all 12 + 12 free entries carry a gradient
    assert (gv[:, :3] != 0).all() and (gf[:, [0, 1, 3]] != 0).all()
    _check_camera(name + " synthetic", gv, gf, _restate(scene, sc, frame, W, cc.TILE))
    if name not in cc.ENTRY_CAMERAS:
        return
    gg = load_golden("geomgrad_" + cc.FIXTURES[name])
    (tmp_path / "fixture").mkdir()
    scene = _golden_scene(tmp_path / "fixture", gg)
    W = torch.from_numpy(gg["W"]).to(DEV)
    frame, outs, _ = _entry(scene, W, cc.TILE)
    assert np.abs(frame.cpu().numpy() - gg["image"]).max() <= PIXEL_TOL
    _check_camera(name, outs[-2], outs[-1], _restate(scene, _sc(gg), frame, W, cc.TILE), fixture=load_golden("camgrad_" + cc.FIXTURES[name]))
    # the older outputs are the screen entry's bits
    _, screen, _ = _entry(scene, W, cc.TILE, camera=False)
    assert len(screen) == 7 and len(outs) == 9 and all(_same(a, b) for a, b in zip(screen, outs))


# ---- the depth entry
@pytest.mark.parametrize("name", cc.ENTRY_CAMERAS)
def test_depth_entry_matches_reference_and_restatement(tmp_path, name):
    dg, base, fwd = depth_fixture(cc.FIXTURES[name])
    scene = _golden_scene(tmp_path, base)
    tile = int(base["tile"])
    W = torch.from_numpy(base["W"]).to(DEV)
    Wd = torch.from_numpy(np.stack([dg["W_D"], dg["W_A"]], -1)).to(DEV)
    frame, depth, grads = _depth_grads(scene, W, Wd, tile=tile)
    sc = _sc(base)
    _check_maps(scene, sc, depth, tile, name)
    zmax = float(dg["z_max"])
    assert np.abs(_np(depth)[..., 0] - dg["D"]).max() <= 1e-4 * zmax and np.abs(_np(depth)[..., 1] - dg["A"]).max() <= 1e-4
    _check_depth(scene, sc, frame, depth, W, Wd, tile, grads, name, fixture=dg)
    # dL/ddepth = 0: the screen entry's bits, all seven outputs
    st = {}
    with torch.no_grad():
        frame, depth = scene.render_image_depth_hip(1, tile_size=tile, stats=st)
    args = (1, tile, "wh3", frame, W, st["n_instances"], st["n_visible"])
    screen = scene._render_backward(*args, geometry=True, screen=True)
    fused = scene._render_backward(*args, geometry=True, screen=True, depth=depth, grad_depth=torch.zeros_like(depth))
    assert len(screen) == len(fused) == 7
    for k, (a, b) in enumerate(zip(screen, fused)):
        assert a.abs().max() > 0 and torch.equal(_bits(a), _bits(b)), k


# ---- the screen and abs statistics
@pytest.mark.parametrize("name", cc.ENTRY_CAMERAS)
def test_screen_and_abs_statistics_match_reference_and_restatement(tmp_path, name):
    fixture = cc.FIXTURES[name]
    gg = load_golden("geomgrad_" + fixture)
    scene = _golden_scene(tmp_path, gg)
    W = torch.from_numpy(gg["W"]).to(DEV)
    tile = int(gg["tile"])
    frame0, plain = _all_grads(scene, W, tile=tile)
    frame, grads, (_, g2d, radius) = _screen_grads(scene, W, tile=tile)
    frame1, grads1, (_, g2d1, radius1, gabs) = _abs_grads(scene, W, tile=tile)
    assert torch.equal(_bits(frame0), _bits(frame)) and torch.equal(_bits(frame0), _bits(frame1))
    for k in FIVE:      # the screen entry keeps the geometry entry's bits, the abs entry the screen entry's
        assert torch.equal(_bits(plain[k]), _bits(grads[k])) and torch.equal(_bits(plain[k]), _bits(grads1[k])), k
    assert torch.equal(_bits(g2d), _bits(g2d1)) and torch.equal(_bits(radius), _bits(radius1))
    pre_ref, n, w, h, _, _, _, _, ref = screen_host.restated(fixture)
    assert sgr.half_extents(w, h)[0] != sgr.half_extents(w, h)[1]
    pre = _oracle_pre(scene, _sc(gg))
    gn, scale = sgr.screen_gradient(pre, n, _np(frame), gg["W"], w, h, tile)
    got = _np(g2d).astype(np.float64)
    e, ef = gbr.per_gaussian_error(got, gn, scale), gbr.per_gaussian_error(got, ref, scale)
    print("%s: grad_means2d: kernel vs restatement, max error / scale %.4g (bound %.3g); vs reference autograd %.4g (bound %.3g)"
          % (name, e, screen_host.BOUND_RESTATEMENT, ef, screen_host.BOUND_FIXTURE))
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    assert e <= screen_host.BOUND_RESTATEMENT and ef <= screen_host.BOUND_FIXTURE, (name, e, ef)
    want_radius = sgr.screen_radius(pre_ref, n, sgr.listed(pre_ref, w, h, tile))
    assert np.array_equal(_np(radius).view(np.uint32), want_radius.view(np.uint32))
    want, signed, scale_a = agr.abs_gradient(pre, n, _np(frame), gg["W"], w, h, tile, with_scale=True)
    got_a = _np(gabs).astype(np.float64)
    ea, eaf = gbr.per_gaussian_error(got_a, want, scale_a), gbr.per_gaussian_error(got_a, abs_host.reference_abs(fixture), scale_a)
    print("%s: grad_means2d_abs: kernel vs restatement, max error / scale %.4g (bound %.3g); vs reference autograd %.4g (bound %.3g)"
          % (name, ea, abs_host.BOUND_RESTATEMENT, eaf, abs_host.BOUND_FIXTURE))
    assert np.isfinite(got_a).all() and got_a.max() > 0 and (got_a >= 0).all()
    assert ea <= abs_host.BOUND_RESTATEMENT and eaf <= abs_host.BOUND_FIXTURE, (name, ea, eaf)
    dead = radius == 0
    assert not _bits(gabs)[dead].any() and not _bits(g2d)[dead].any()


# ---- an SH scene at the far pose
def _sh_scene(path, seed=19):
    from intro_to_gaussian_splatting_amd import GaussianScene, Gaussians
    from intro_to_gaussian_splatting_amd.synthetic import make_trained_like_scene, write_colmap_text

    sc = cc.scene("farpose", 300, seed, make=make_trained_like_scene, sh_degree=3)
    write_colmap_text(str(path), sc)
    g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"], device=DEV)
    g.sh = torch.from_numpy(sc["sh"]).to(DEV).contiguous()
    g.sh_degree = 3
    return GaussianScene(str(path), g)


def test_sh_scene_at_the_far_pose_carries_the_rgb_scene_s_gradients_and_the_centre_s_share(tmp_path):
    """The view direction goes through camera_center = -R^T t: at 140 degrees about an oblique axis no entry of R is near
    0 or 1.  test_hip_sh_backward.py's and test_hip_camera_gradient.py's checks, on this scene."""
    scene = _sh_scene(tmp_path)
    centre = np.asarray(scene.images[1].camera_center_host, np.float64)
    c = cc.CAMERAS["farpose"]
    assert np.abs(centre + cc.rotation(c["qvec"]).T @ np.asarray(c["tvec"])).max() <= 1e-5
    carried_one_link_further(tmp_path, scene, _W((64, 48, 3), 19), 3)
    (tmp_path / "share").mkdir()
    camera_centre_share(_sh_scene(tmp_path / "share"))


# ---- determinism
def test_two_runs_at_roll_give_equal_bits_with_and_without_hints(tmp_path):
    sc = _synthetic("roll")
    scene = _scene(tmp_path, sc)
    W = _W((64, 48, 3), 23)
    _, a, sa = _abs_grads(scene, W)
    _, b, sb = _abs_grads(scene, W)
    _, c, sc_ = _abs_grads(scene, W, use_hints=False)
    for other in (sb, sc_):
        assert all(torch.equal(_bits(sa[i]), _bits(other[i])) for i in (1, 2, 3))
    for k in a:
        assert a[k].abs().max() > 0 and torch.equal(_bits(a[k]), _bits(b[k])) and torch.equal(_bits(a[k]), _bits(c[k])), k
    _, first, _ = _entry(scene, W)
    _, again, _ = _entry(scene, W)
    assert len(first) == 9 and all(_same(x, y) for x, y in zip(first, again)) and first[-2].abs().max() > 0


# ================================================================================================ the std_3dgs rule set
# The cases of camera_cases.STD_CAMERA_CASES, the sibling files' own checks and bounds (module doc).

STD_NAMES = list(std_cam.CAMERA_CASES)
AA_NAMES = list(std_cam.CAMERA_CASES_AA)
_OWN_CAMERA = {}         # (case, antialiased) -> the case again on the scene object's own camera, built once


def _std_case(tmp_path, name, antialiased=False):
    """(case dict, scene).  Where the scene object rounds its camera otherwise than cpu_ref.build_camera (tan_fovx of aniso
    and roll, in the last bit), the case is the one walked on the arrays the kernels get."""
    case = (std_cam.backward_case_aa if antialiased else std_cam.backward_case)(name)
    scene = _scene(tmp_path, case["sc"], colors=case["colors"])
    gcam = _oracle_cam(scene)
    if _same_camera(case["cam"], gcam):
        return case, scene
    if (name, antialiased) not in _OWN_CAMERA:
        print("%s: walking the scene object's own camera" % name)
        args = (case["sc"], case["tile"], case["bg"])
        if antialiased:
            own = aa_host.build_backward(aa_host.build_case(*args, cam=gcam, colors=case["colors"]))
            wk = own["fwd"].wk
        else:
            own = std_host.build_backward(std_host.build_tuple(*args, cam=gcam, colors=case["colors"]))
            wk = own["wk"]
        assert not wk.left_out and (~own["mask"]).sum() <= std_host.MAX_MASKED_SHARE * own["mask"].size
        _OWN_CAMERA[(name, antialiased)] = own
    return _OWN_CAMERA[(name, antialiased)], scene


def _line(err, keys):
    return "  ".join("%s %.3g" % (k, err[k]) for k in keys)


# ---- the frame
@pytest.mark.parametrize("name", STD_NAMES)
def test_std3dgs_frame_is_decided_or_explained_on_every_route_and_ignores_the_principal_point(tmp_path, name):
    case, scene = _std_case(tmp_path, name)
    sc, tile, bg, w, h = case["sc"], case["tile"], case["bg"], case["W"], case["H"]
    c = scene.images[1].gsx_camera()
    camera = cc.CAMERAS[cc.STD_CAMERA_CASES[name][0]]
    assert (c.fx, c.fy, c.width, c.height) == (np.float32(camera["fx"]), np.float32(camera["fy"]), w, h)
    kw = dict(tile_size=tile, semantics="std_3dgs", background=bg)
    st, tight = {}, {}
    with torch.no_grad():
        img = scene.render_image_hip(1, layout="hw3", published_rects=True, stats=st, **kw)
        assert tuple(img.shape) == (h, w, 3)
        assert st["n_visible"] == case["nvis"] and st["n_instances"] == case["inst"]
        _judge("std_3dgs " + name, case["wk"], img.cpu().numpy(), FRAME_BOUND["std_3dgs"])
        # every other route: the same frame, bit for bit
        assert torch.equal(scene.render_image_hip(1, layout="hw3", stats=tight, **kw), img), "tight rectangles"
        assert tight["n_visible"] == case["nvis"] and tight["n_instances"] <= case["inst"]
        assert torch.equal(scene.render_image_hip(1, layout="hw3", generic_kernels=True, published_rects=True, **kw), img)
        assert torch.equal(scene.render_image_hip(1, layout="hw3", generic_kernels=True, **kw), img)
        assert torch.equal(scene.render_image_hip(1, layout="wh3", **kw).permute(1, 0, 2), img)
        assert torch.equal(scene.render_image_hip(1, layout="wh3", generic_kernels=True, **kw).permute(1, 0, 2), img)
        ntx, nty = (w + tile - 1) // tile, (h + tile - 1) // tile
        acc = torch.zeros_like(img)
        for x0, x1 in ((0, ntx // 2), (ntx // 2, ntx)):
            for y0, y1 in ((0, nty // 2), (nty // 2, nty)):
                acc += scene.render_image_hip(1, layout="hw3", tile_window=(x0, x1, y0, y1), **kw)
        assert torch.equal(acc, img), "tile windows"
        # a principal point off the centre: the render path reads none
        (tmp_path / "off").mkdir()
        moved = _scene(tmp_path / "off", cc.off_centre(sc), colors=case["colors"])
        assert float(moved.images[1].c_x) != float(scene.images[1].c_x)
        assert torch.equal(_bits(moved.render_image_hip(1, layout="hw3", published_rects=True, **kw)), _bits(img))


# ---- the gradients
@pytest.mark.parametrize("name", STD_NAMES)
def test_std3dgs_gradients_match_the_restatement(tmp_path, name):
    case, scene = _std_case(tmp_path, name)
    gf = torch.from_numpy(case["g"]).to(DEV)
    frame, st = hip_std._forward(scene, case)
    outs = hip_std._backward(scene, case, frame, st, gf)
    assert len(outs) == 7
    err = hip_std._errors(case, outs)
    print("%s: kernel vs restatement, max error / scale: %s" % (name, _line(err, hip_std.KEYS)))
    # the radius is the stage-1 row's wherever the frame listed the Gaussian, 0 elsewhere; whoever has gradient is listed
    radius, rows = outs[6].cpu().numpy().reshape(-1), case["rows"]
    listed = radius > 0
    assert listed.any() and np.array_equal(radius[listed], rows[listed, 5])
    assert listed[case["ref"].scales["colors"] > 0].all() and not listed[np.isnan(rows[:, 0])].any()
    for o in outs[:6]:
        assert o.abs().max() > 0 and not o.cpu().numpy()[~listed].any()
    # two runs: the same bits
    again = hip_std._backward(scene, case, frame, st, gf)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, outs))
    # published rectangles: the same frame, other slots -- within the bound
    frame_p, st_p = hip_std._forward(scene, case, published_rects=True)
    assert torch.equal(frame_p, frame) and st_p["n_instances"] >= st["n_instances"]
    outs_p = hip_std._backward(scene, case, frame_p, st_p, gf, published=True)
    err_p = hip_std._errors(case, outs_p)
    print("%s: published rectangles: %s" % (name, _line(err_p, hip_std.KEYS)))
    radius_p = outs_p[6].cpu().numpy().reshape(-1)
    assert np.array_equal(radius_p[radius_p > 0], rows[radius_p > 0, 5]) and (radius_p > 0)[listed].all()
    for o in outs_p[:6]:
        assert not o.cpu().numpy()[radius_p == 0].any()
    for k in hip_std.KEYS:
        assert err[k] <= std_host.BOUND[k], (name, k, err[k], std_host.BOUND[k])
        assert err_p[k] <= std_host.BOUND[k], (name, "published", k, err_p[k], std_host.BOUND[k])
    if name in cc.STD_OFFAXIS:      # the clamp's branch carried gradient on the GPU too
        ewa = case["ref"].clamped_ewa & (case["ref"].scales["points"] > 0)
        assert ewa.sum() >= 10 and np.abs(outs[2].cpu().numpy()[ewa]).max() > 0


# ---- anti-aliased
@pytest.mark.parametrize("name", AA_NAMES)
def test_antialiased_frame_and_gradients_match_the_restatement_and_the_flag_clear_call_keeps_its_bits(tmp_path, name):
    case, scene = _std_case(tmp_path, name, antialiased=True)
    img, st_p = hip_aa._frame(scene, case, antialiased=True, published_rects=True)
    assert tuple(img.shape) == (case["H"], case["W"], 3) and st_p["n_instances"] == case["inst"]
    hip_aa._hold_frame("antialiased " + name, case, img, st_p)
    plain, st0 = hip_aa._frame(scene, case)
    frame, st = hip_aa._frame(scene, case, antialiased=True)
    assert torch.equal(frame, img) and st["n_instances"] == st0["n_instances"] <= case["inst"]
    assert not torch.equal(plain, img)
    assert torch.equal(hip_aa._frame(scene, case, antialiased=True, generic_kernels=True)[0], img)
    assert torch.equal(hip_aa._frame(scene, case, layout="wh3", antialiased=True)[0].permute(1, 0, 2), img)
    # the gradients
    gf = torch.from_numpy(case["g"]).to(DEV)
    outs = hip_aa._backward(scene, case, frame, st, gf)
    assert len(outs) == 7
    got, err = hip_aa._errors(case["ref"], outs)
    print("%s: antialiased: kernel vs restatement, max error / scale: %s" % (name, _line(err, aar.KEYS)))
    radius, rows = outs[6].cpu().numpy().reshape(-1), case["rows0"]
    listed = radius > 0
    assert listed.any() and np.array_equal(radius[listed], rows[listed, 5])
    assert listed[case["ref"].scales["colors"] > 0].all()
    for o in outs[:6]:
        assert o.abs().max() > 0 and not o.cpu().numpy()[~listed].any()
    again = hip_aa._backward(scene, case, frame, st, gf)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, outs))
    # flag clear: the argument not passed, and passed as False -- the same bits, and not the anti-aliased ones
    a = hip_aa._backward(scene, case, plain, st0, gf, std=(case["bg"], False))
    b = hip_aa._backward(scene, case, plain, st0, gf, antialiased=False)
    off, st_off = hip_aa._frame(scene, case, antialiased=False)
    assert torch.equal(_bits(off), _bits(plain)) and st_off["n_instances"] == st0["n_instances"]
    assert len(a) == len(b) == 7 and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    assert not torch.equal(outs[1], a[1]) and not torch.equal(outs[3], a[3])
    for k in aar.KEYS:
        assert err[k] <= aa_host.BOUND_AA[k], (name, k, err[k], aa_host.BOUND_AA[k])


# scales in pixels at z = 4 along the Gaussian's own axes: an ordinary one, a needle, one on the floor of rho
AA_PROBES = [(2.0, 0.7, 1.2), (3.0, 0.03, 0.03), (0.02, 0.03, 0.01)]
PROBE_OFFSET = (9, -7)          # pixels from the frame centre: J's third column is not zero


@pytest.mark.parametrize("camera", cc.NAMES)
def test_antialiased_packed_opacity_is_the_mirrors_bit_for_bit(tmp_path, camera):
    """tests/test_hip_antialias.py's probes at these cameras: one Gaussian, sigmoid(20) = 1 in float32, colour 1, black
    background, so the pixel under its centre is op_eff exp(power) = rho exp(power).  At a far pose no float32 point
    projects onto a pixel centre exactly; the point is placed there in float64 and rounded, which leaves |power| below
    2^-26 (asserted from the C port's float32 stage 1): exp is 1 to the last bit and the pixel is rho's bits."""
    from oracle import std3dgs_ref

    c = cc.CAMERAS[camera]
    w, h, z = c["width"], c["height"], 4.0
    px, py = w // 2 + PROBE_OFFSET[0], h // 2 + PROBE_OFFSET[1]
    R, t = cc.rotation(c["qvec"]), np.asarray(c["tvec"], np.float64)
    p_cam = np.array([(px + 0.5 - w / 2) * z / c["fx"], (py + 0.5 - h / 2) * z / c["fy"], z])
    point = (R.T @ (p_cam - t)).astype(np.float32)[None]
    quat = (np.array([[0.7, 0.3, -0.5, 0.4]]) / np.linalg.norm([0.7, 0.3, -0.5, 0.4])).astype(np.float32)
    for k, sigma in enumerate(AA_PROBES):
        sc = dict(points=point, colors_0_255=np.full((1, 3), 256.0, np.float32),
                  scales=(np.array([sigma]) * z / np.sqrt(c["fx"] * c["fy"])).astype(np.float32), quaternions=quat,
                  opacity=np.array([[20.0]], np.float32), fx=np.float64(c["fx"]), fy=np.float64(c["fy"]), cx=np.float64(w / 2),
                  cy=np.float64(h / 2), width=np.int64(w), height=np.int64(h), qvec=np.asarray(c["qvec"], np.float64),
                  tvec=np.asarray(c["tvec"], np.float64))
        (tmp_path / str(k)).mkdir()
        scene = _scene(tmp_path / str(k), sc, colors=np.ones((1, 3), np.float32))
        cam = _oracle_cam(scene)
        st1 = std3dgs_ref.stage1(sc["points"], sc["scales"], sc["quaternions"], sc["opacity"], cam, 16)
        assert st1.opacity[0] == np.float32(1.0)
        dx, dy = float(st1.xy[0][0]) - px, float(st1.xy[0][1]) - py
        A, B, C = (float(v) for v in st1.conic[0])
        power = 0.5 * (A * dx * dx + C * dy * dy) + B * dx * dy
        assert abs(dx) < 1e-3 and abs(dy) < 1e-3 and abs(power) < 2.0 ** -26, (camera, k, dx, dy, power)
        fac = aar.factor(*aar.covariance32(sc["points"], sc["scales"], sc["quaternions"], cam))
        rho = fac.rho[0]
        assert np.float32(1.0 / 255.0) <= rho < np.float32(0.99)          # composited, and not the alpha clamp
        assert bool(fac.clamped[0]) == (k == 2) and (not fac.clamped[0] or rho == np.float32(0.005))
        with torch.no_grad():
            img = scene.render_image_hip(1, layout="hw3", semantics="std_3dgs", antialiased=True)
            plain = scene.render_image_hip(1, layout="hw3", semantics="std_3dgs")
        got = img[py, px].cpu().numpy()
        print("%s probe %d: rho mirror %.9g (det0 %.6g, ratio %.6g), kernel %.9g; centre %.2e, %.2e px off the pixel's" % (
            camera, k, rho, fac.det0[0], fac.ratio[0], got[0], dx, dy))
        assert (got.view(np.int32) == np.float32(rho).view(np.int32)).all(), (camera, k, got, rho)
        assert (plain[py, px].cpu().numpy() == np.float32(0.99)).all()      # without the flag: sigmoid = 1, clamped at 0.99


# ---- the contribution
@pytest.mark.parametrize("name", ["std_roll_64x48_n100", "std_offaxis_aniso_tall_48x64_n100"])
def test_std3dgs_contribution_sum_is_the_backward_s_bits_and_max_and_pixels_match_the_restatement(tmp_path, name):
    case, scene = _std_case(tmp_path, name)
    assert hip_con.BG == case["bg"]
    n, tile = case["n"], case["tile"]
    frame, st = hip_con._forward(scene, "std_3dgs", tile)
    con = hip_con._contribution(scene, "std_3dgs", tile, st)
    gc0 = hip_con._colour_gradient(scene, "std_3dgs", tile, frame, st)
    assert gc0.abs().max() > 0 and torch.equal(_bits(con.weight_sum), _bits(gc0))
    other = scene.render_contribution_hip(1, semantics="std_3dgs", tile_size=tile)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(con, other))
    ref = cr.std_3dgs(case["R"], case["W"], case["H"], n)
    assert not ref.excluded.any()
    wmax, wsum, pixels, views = (_np(x) for x in con)
    err, bad = cr.compare(wmax, pixels, ref)
    err_sum = float(np.abs(wsum - ref.weight_sum).max() / max(1.0, ref.weight_sum.max()))
    print("%s: |weight_max - restatement| %.3g (bound %.3g), weight_sum vs restatement %.3g of its largest, %d rows composited"
          % (name, err, hip_con.TOL, err_sum, int((pixels > 0).sum())))
    assert (pixels > 0).sum() >= 50 and err <= hip_con.TOL and bad.size == 0 and err_sum <= hip_con.TOL, (name, err, bad[:10])
    assert (views[pixels > 0] == 1).all() and not wsum[views == 0].any() and not wmax[views == 0].any()
    # published rectangles: the same composited pairs
    frame_p, st_p = hip_con._forward(scene, "std_3dgs", tile, published=True)
    con_p = hip_con._contribution(scene, "std_3dgs", tile, st_p, published=True)
    assert torch.equal(_bits(con_p.weight_max), _bits(con.weight_max)) and torch.equal(con_p.pixels, con.pixels)
    assert torch.equal(_bits(con_p.weight_sum), _bits(hip_con._colour_gradient(scene, "std_3dgs", tile, frame_p, st_p, published=True)))


# ---- through the public surface
def test_std3dgs_autograd_gives_the_raw_call_s_bits_and_an_sh_copy_carries_them_on(tmp_path):
    name = "std_offaxis_roll_64x48_n100"
    case, scene = _std_case(tmp_path, name)
    gf = torch.from_numpy(case["g"]).to(DEV)
    plain, st = hip_std._forward(scene, case)
    want = hip_std._backward(scene, case, plain, st, gf)
    frame, grads = hip_std._autograd(scene, case, gf, geometry_gradients=True, screen_statistics=True)
    assert frame.grad_fn is not None and torch.equal(frame.detach(), plain)
    for key, ref in zip(("colors", "opacity", "points", "scales", "quaternions"), want):
        assert grads[key].abs().max() > 0 and torch.equal(_bits(grads[key].reshape(-1)), _bits(ref.reshape(-1))), key
    idx, g2d, radius = scene.screen_statistics
    assert idx == 1 and torch.equal(_bits(g2d), _bits(want[5])) and torch.equal(_bits(radius), _bits(want[6].view(-1)))
    # the SH copy: degree 2, the case's colours lifted to DC.  The view direction reads the camera centre -R^T t
    g = scene.gaussians
    g.sh = torch.from_numpy(_sh_for(case["colors"], 2, 3)).to(DEV).contiguous()
    g.sh_degree = 2
    centre = np.asarray(scene.images[1].camera_center_host, np.float64)
    c = cc.CAMERAS["roll"]
    assert np.abs(centre + cc.rotation(c["qvec"]).T @ np.asarray(c["tvec"])).max() <= 1e-5
    plain_sh, st = hip_std._forward(scene, case)
    assert not torch.equal(plain_sh, plain)
    outs = hip_std._backward(scene, case, plain_sh, st, gf, screen=False)
    gsh, gview = scene._sh_backward(1, outs[0], with_points=True)
    frame, grads = hip_std._autograd(scene, case, gf, names=("points", "opacity", "sh"), geometry_gradients=True)
    assert torch.equal(frame.detach(), plain_sh) and grads["colors"] is None
    assert grads["sh"].abs().max() > 0 and torch.equal(_bits(grads["sh"].reshape(-1)), _bits(gsh.reshape(-1)))
    assert torch.equal(_bits(grads["opacity"].reshape(-1)), _bits(outs[1].reshape(-1)))
    assert gview.abs().max() > 0 and torch.equal(_bits(grads["points"]), _bits(outs[2] + gview))
    # and the link itself against its float64 restatement at this camera centre (tests/test_hip_sh_backward.py's check)
    pts, sh, gc = case["sc"]["points"], _np(g.sh), _np(outs[0])
    pre, mask = shr.forward(pts, sh, 2, centre)[:2]
    sure = np.abs(pre) >= shr.NEAR_ZERO
    assert (~sure).mean() <= 0.01 and 0.01 <= (~mask).mean() <= 0.5
    ref_sh, ref_mean, scale_sh, scale_mean = shr.backward(pts, sh, 2, centre, gc)
    e_sh = shr.scaled_error(_np(gsh), ref_sh, scale_sh, keep=sure[:, None, :])
    e_mean = shr.scaled_error(_np(gview), ref_mean, scale_mean, keep=sure.all(1)[:, None])
    print("%s: SH link vs restatement, max error / scale: sh %.4g (bound %.3g), points %.4g (bound %.3g)" % (
        name, e_sh, sh_host.BOUND["sh"], e_mean, sh_host.BOUND["points"]))
    assert e_sh <= sh_host.BOUND["sh"] and e_mean <= sh_host.BOUND["points"], (e_sh, e_mean)
