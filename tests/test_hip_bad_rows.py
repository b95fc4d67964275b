"""Every gradient entry on scenes with non-finite and degenerate rows (tests/bad_row_cases.py), on the GPU.

A fit does not stay made of healthy rows; include/gsx.h promises "exact zeros for a Gaussian that is culled or on no tile list"
and "same inputs, same bits" for every entry.  Each case is a scene with bad rows written in place and its clean twin (the
UNLISTED rows replaced by culled finite ones, the DEGENERATE rows kept).  Per case and entry:
  forward    the frame is finite, the twin's bits in both layouts, within PIXEL_TOL of the C oracle, with the oracle's pair count
  inert      every UNLISTED row holds +-0 in every per-Gaussian output; no output holds a non-finite value
  float64    every other row within BOUND_BAD = 12 E_REF_BAD of the restatement (tests/test_bad_rows_host.py), in the
             restatement's own norm; colours and opacity logits at test_backward_host.py's TOL; D and A at the depth maps' tolerance
  twin       every output is the twin's, bit for bit, in all rows but the replaced ones
  a fit      three Trainer steps on the scene and on its twin: the same losses, parameters, moments, poses; the UNLISTED
             rows keep their own bits and are never counted by the screen statistic
The entries: ref_cpu colour-only, geometry, screen, abs, camera, depth (with gsx_render_depth), contribution; std_3dgs
gsx_render_backward_std plain, with published rectangles and anti-aliased, and its contribution; the SH link
(gsx_sh_backward_active) behind the geometry, camera and depth entries, at the stored degree and at active degree 1.

Found: the SH link gave an UNLISTED row whose mean is NaN, infinite or the camera centre, or which holds a NaN coefficient,
a NaN dL/dpoints (0 * NaN), which ``camera_gradients=True`` sums into dL/dworld2view.  gsx_sh_backward / _active now apply
the zero-row rule (include/gsx.h).  Every other entry already skips a rank on no tile list.  And, on a healthy row of case
`base` whose centre lies outside the rendered region: the depth entry's dL/dopacity was 7.25e-07 of its scale from float64
(bound 5.83e-07), the rounding of power * log2(e) in alpha_ref; the list-walking kernels now evaluate alpha_ref_walk
(csrc/gsx_internal.h, docs/lab_notes/bad_rows.md).

Measured on an MI355X (35 tests, 6 s in all), kernel vs restatement, worst error / scale (base, roll) and the bound:
  geometry     points 3.20e-09, 4.76e-09 (2.61e-07)   scales 6.81e-08, 6.05e-09 (5.62e-06)   quaternions 3.89e-09, 2.92e-10 (4.55e-08)
               colours 8.69e-08, 1.73e-07   opacity 2.13e-08, 2.83e-08 (TOL 8e-06)
  screen, abs  grad_means2d 2.80e-07, 1.55e-08 (5.17e-07)   grad_means2d_abs 2.82e-07, 1.52e-08 (3.53e-07); the radius: bits
  camera       world2view 2.23e-11, 7.21e-11 (3.49e-08)   full_proj 3.66e-10, 2.53e-10 (6.64e-08)
  depth        points 5.93e-09, 1.42e-08 (6.05e-07)   scales 1.15e-07, 6.63e-09 (4.33e-07)   quaternions 6.66e-09, 2.51e-10 (5.07e-08)
               colors 8.69e-08, 1.73e-07 (2.33e-06)   opacity 3.31e-08, 1.62e-08 (5.83e-07)
               maps |dD| / z_listed 1.91e-07, 2.47e-07   |dA| 3.17e-07, 3.84e-07 (1e-4)
  contribution |weight_max - restatement| 1.19e-07, 1.09e-07; std_3dgs 9.57e-08, 8.79e-08 (1e-4)
  std_3dgs (std_base, std_roll; published rectangles give the same digits)
               colors 3.61e-08, 6.48e-08 (7.95e-06)   opacity 7.70e-09, 5.99e-09 (1.91e-07)   points 4.25e-09, 1.66e-09 (1.72e-07)
               scales 1.46e-09, 8.64e-10 (7.37e-08)   quaternions 6.75e-11, 2.20e-10 (3.47e-09)   means2d 8.17e-09, 3.36e-09 (3.12e-07)
  anti-aliased colors 4.52e-08, 4.77e-08   opacity 7.67e-09, 5.02e-09   points 3.01e-09, 1.23e-09   scales 8.34e-10, 5.86e-10
               quaternions 3.58e-11, 5.62e-11   means2d 8.84e-09, 4.56e-09 (BOUND_AA of tests/test_antialias_host.py)
  SH link      (sh3, sh3_active1) sh 5.13e-07, 2.14e-07 (8.31e-06)   points 2.25e-07, 2.06e-07 (4.61e-06)
  frames vs the C oracle at most 4.17e-07 (1e-4).  Everything else the tests assert is bits.
With the library of the parent commit (no zero-row rule) 12 of the 15 SH and fit tests fail on a NaN where a zero belongs.
"""
import numpy as np
import pytest
import torch

import abs_gradient_restatement as agr
import antialias_restatement as aar
import bad_row_cases as brc
import camera_cases as cc
import contribution_restatement as cr
import depth_restatement as dr
import geometry_backward_restatement as gbr
import screen_gradient_restatement as sgr
import sh_backward_restatement as shr
import test_abs_statistic_host as abs_host
import test_bad_rows_host as host
import test_hip_antialias as hip_aa
import test_hip_contribution as hip_con
import test_hip_std3dgs_backward as hip_std
import test_screen_statistic_host as screen_host
import test_sh_backward_host as sh_host
from test_hip_abs_statistic import _abs_grads
from test_hip_backward import DEV, _grads, _oracle_pre, _scene
from test_hip_camera_cases import _check_colours
from test_hip_camera_gradient import _bits, _entry, _restate
from test_hip_camera_gradient import _check as _check_camera
from test_hip_depth import _check_maps, _depth_grads
from test_hip_geometry_backward import _W, _all_grads, _camera
from test_hip_geometry_backward import _check as _check_geometry
from test_hip_parity import _oracle_cam
from test_hip_rule_sets import _same_camera
from test_hip_screen_statistic import FIVE, _screen_grads

pytestmark = pytest.mark.gpu

PIXEL_TOL = 1e-4            # test_hip_parity.py's
W_, H_, TILE, N = brc.WIDTH, brc.HEIGHT, brc.TILE, brc.N
RGB, SH, STD = list(brc.RGB_CASES), list(brc.SH_REF_CPU), list(brc.STD_CASES)
SH_TRAINED = ("points", "scales", "quaternions", "opacity", "sh")


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _build(path, sc, active=None):
    path.mkdir(exist_ok=True)
    scene = _scene(path, sc, colors=sc["colors"])
    if "sh" in sc:
        g = scene.gaussians
        g.sh = torch.from_numpy(sc["sh"]).to(DEV).contiguous()
        g.sh_degree = 3
        if active is not None and active < 3:
            g.active_sh_degree = active
    return scene


def _pair(tmp_path, kind, name):
    """(bad scene dict, twin scene dict, replaced rows' mask on the device and on the host, bad scene, twin scene)."""
    if kind == "rgb":
        bad, twin, rows = brc.rgb_case(name)
        active = None
    else:
        bad, twin, rows, _, active = brc.sh_case(name)
    a, b = _build(tmp_path / "bad", bad, active), _build(tmp_path / "twin", twin, active)
    if kind == "sh":        # the row on the camera centre is on THIS scene object's centre, to the bit
        centre = np.asarray(a.images[1].camera_center_host, np.float32)
        assert np.array_equal(bad["points"][rows["at_centre"]], centre)
        assert np.array_equal(_np(a.gaussians.points)[rows["at_centre"]], centre)
    rep = brc.replaced(rows)
    return bad, twin, torch.from_numpy(rep).to(DEV), rep, a, b


def _hold_pair(tag, got, want, rep_dev):
    """name -> tensor of the bad scene and of its twin: finite; +-0 in the replaced rows of every per-Gaussian output of the
    bad scene; the twin's bits everywhere else."""
    assert set(got) == set(want), tag
    for key, a in got.items():
        b = want[key]
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, key)
        if a.dtype.is_floating_point:
            assert torch.isfinite(a).all(), (tag, key, "non-finite")
        if a.dim() and a.shape[0] == N and key not in ("frame", "depth"):
            bits_a, bits_b = (_bits(a), _bits(b)) if a.dtype == torch.float32 else (a, b)
            inert = bits_a[rep_dev]
            if a.dtype == torch.float32:
                inert = inert & 0x7FFFFFFF      # +0 or -0
            assert not inert.any(), (tag, key, "an UNLISTED row is not exact zeros")
            assert torch.equal(bits_a[~rep_dev], bits_b[~rep_dev]), (tag, key, "differs from the clean twin")
            assert a[~rep_dev].abs().max() > 0 or key in ("views",), (tag, key, "all zero")
        else:
            assert torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b), (tag, key)


# ================================================================================================ the frame
@pytest.mark.parametrize("kind,name", [("rgb", k) for k in RGB] + [("sh", k) for k in SH])
def test_frame_is_finite_the_twin_s_bits_and_the_oracle_s(tmp_path, kind, name):
    """Keeps what test_huge_and_offscreen_splats' docstring promises of NaN inputs."""
    from oracle import c_oracle

    bad, twin, rep_dev, rep, a, b = _pair(tmp_path, kind, name)
    fwd, _ = host.forward_of(kind, name)
    frames = {}
    for layout in ("wh3", "hw3"):
        sa, sb = {}, {}
        with torch.no_grad():
            fa = a.render_image_hip(1, tile_size=TILE, layout=layout, stats=sa)
            fb = b.render_image_hip(1, tile_size=TILE, layout=layout, stats=sb)
        assert torch.isfinite(fa).all() and torch.equal(_bits(fa), _bits(fb)), layout
        assert sa["n_instances"] == sb["n_instances"] == fwd["bad"]["inst"], layout
        assert sa["n_visible"] == np.asarray(fwd["bad"]["pre"].order).size and sb["n_visible"] == np.asarray(fwd["twin"]["pre"].order).size
        assert sb["n_visible"] >= 4
        frames[layout] = fa
    assert torch.equal(frames["hw3"].permute(1, 0, 2), frames["wh3"])
    if kind == "rgb":
        pre = _oracle_pre(a, bad)
        ref, _, inst = c_oracle.render(pre, W_, H_, TILE)
        assert inst == fwd["bad"]["inst"]
    else:       # the oracle's frame over the float32 port's SH colours
        ref = fwd["bad"]["frame"]
    err = float(np.abs(_np(frames["wh3"]) - ref).max())
    print("%s %s: frame vs C oracle %.3g, %d instances" % (kind, name, err, fwd["bad"]["inst"]))
    assert ref.max() > 0.1 and err <= PIXEL_TOL


# ================================================================================================ ref_cpu, RGB scenes
@pytest.mark.parametrize("name", RGB)
def test_colour_only_and_geometry_entries(tmp_path, name):
    bad, twin, rep_dev, rep, a, b = _pair(tmp_path, "rgb", name)
    W = _W((W_, H_, 3), 5)
    out = {}
    for tag, scene in (("bad", a), ("twin", b)):
        frame0, gc, go = _grads(scene, W, tile=TILE)
        scene.gaussians.colors.requires_grad_(False)
        scene.gaussians.opacity.requires_grad_(False)
        frame, grads = _all_grads(scene, W, tile=TILE)
        assert torch.equal(_bits(frame0), _bits(frame))
        assert torch.equal(_bits(gc), _bits(grads["colors"])) and torch.equal(_bits(go), _bits(grads["opacity"]))
        out[tag] = dict(grads, frame=frame, colour_only_colors=gc, colour_only_opacity=go)
    _hold_pair(name, out["bad"], out["twin"], rep_dev)
    grads, frame = {k: out["bad"][k] for k in FIVE}, out["bad"]["frame"]
    restated = _check_geometry(a, bad, frame, W, TILE, grads, name)         # 12 E_REF = 12 E_REF_BAD for these three
    _check_colours(a, bad, frame, W, TILE, grads, name)
    assert (np.abs(restated[0]).sum(1) > 0).sum() >= N // 2
    for key in ("geometry",):
        for k in ("points", "scales", "quaternions"):
            assert host.BOUND_BAD[key][k] == 12 * host.geometry_host.E_REF[k]


@pytest.mark.parametrize("name", RGB)
def test_screen_and_abs_entries(tmp_path, name):
    bad, twin, rep_dev, rep, a, b = _pair(tmp_path, "rgb", name)
    W = _W((W_, H_, 3), 5)
    out = {}
    for tag, scene in (("bad", a), ("twin", b)):
        frame, grads, (_, g2d, radius) = _screen_grads(scene, W, tile=TILE)
        frame1, grads1, (_, g2d1, radius1, gabs) = _abs_grads(scene, W, tile=TILE)
        assert torch.equal(_bits(frame), _bits(frame1)) and torch.equal(_bits(g2d), _bits(g2d1)) and torch.equal(_bits(radius), _bits(radius1))
        for k in FIVE:
            assert torch.equal(_bits(grads[k]), _bits(grads1[k])), k
        out[tag] = dict(grads, frame=frame, grad_means2d=g2d, screen_radius=radius, grad_means2d_abs=gabs)
    _hold_pair(name, out["bad"], out["twin"], rep_dev)
    o = out["bad"]
    pre = _oracle_pre(a, bad)
    frame = _np(o["frame"])
    gn, scale = sgr.screen_gradient(pre, N, frame, _np(W), W_, H_, TILE)
    e = gbr.per_gaussian_error(_np(o["grad_means2d"]).astype(np.float64), gn, scale)
    want, signed, scale_a = agr.abs_gradient(pre, N, frame, _np(W), W_, H_, TILE, with_scale=True)
    ea = gbr.per_gaussian_error(_np(o["grad_means2d_abs"]).astype(np.float64), want, scale_a)
    print("%s: grad_means2d %.4g (bound %.3g), grad_means2d_abs %.4g (bound %.3g)" % (
        name, e, host.BOUND_BAD["screen"], ea, host.BOUND_BAD["abs"]))
    assert host.BOUND_BAD["screen"] == screen_host.BOUND_RESTATEMENT and host.BOUND_BAD["abs"] == abs_host.BOUND_RESTATEMENT
    assert e <= host.BOUND_BAD["screen"] and ea <= host.BOUND_BAD["abs"], (name, e, ea)
    # the radius: the stage-1 row's of every listed Gaussian, +0 elsewhere -- an UNLISTED row's radius is NaN in stage 1
    want_radius = sgr.screen_radius(pre, N, sgr.listed(pre, W_, H_, TILE))
    assert np.array_equal(_np(o["screen_radius"]).view(np.uint32), want_radius.view(np.uint32))
    assert (want_radius[list(brc.DEGENERATE.values())] > 0).all() and not want_radius[rep].any()


@pytest.mark.parametrize("name", RGB)
def test_camera_entry(tmp_path, name):
    bad, twin, rep_dev, rep, a, b = _pair(tmp_path, "rgb", name)
    W = _W((W_, H_, 3), 5)
    keys = FIVE_RAW + ("grad_means2d", "screen_radius", "grad_world2view", "grad_full_proj")
    out = {}
    for tag, scene in (("bad", a), ("twin", b)):
        frame, outs, _ = _entry(scene, W, TILE)
        assert len(outs) == 9
        out[tag] = dict(zip(keys, outs), frame=frame)
        for key in ("grad_world2view", "grad_full_proj"):
            assert out[tag][key].shape == (4, 4)
    _hold_pair(name, out["bad"], out["twin"], rep_dev)
    o = out["bad"]
    _check_camera(name, o["grad_world2view"], o["grad_full_proj"], _restate(a, bad, o["frame"], W, TILE))    # 12 E_REF = 12 E_REF_BAD


FIVE_RAW = ("colors", "opacity", "points", "scales", "quaternions")        # the order of the raw entries' outputs


@pytest.mark.parametrize("name", RGB)
def test_depth_entry_and_maps(tmp_path, name):
    bad, twin, rep_dev, rep, a, b = _pair(tmp_path, "rgb", name)
    W, Wd = _W((W_, H_, 3), 5), _W((W_, H_, 2), 6)
    out = {}
    for tag, scene in (("bad", a), ("twin", b)):
        frame, depth, grads = _depth_grads(scene, W, Wd, tile=TILE)
        with torch.no_grad():
            f0, d0 = scene.render_image_depth_hip(1, tile_size=TILE)
        assert torch.equal(_bits(f0), _bits(frame)) and torch.equal(_bits(d0), _bits(depth))
        out[tag] = dict(grads, frame=frame, depth=depth)
    _hold_pair(name, out["bad"], out["twin"], rep_dev)
    o = out["bad"]
    _check_maps(a, bad, o["depth"], TILE, name)
    pre = _oracle_pre(a, bad)
    ref = dr.depth_backward(pre, bad["points"], bad["scales"], bad["quaternions"], _camera(a), _np(o["frame"]), _np(W), _np(o["depth"]),
                            _np(Wd), W_, H_, TILE, with_scale=True)
    got = [_np(o[k]).astype(np.float64).reshape(N, -1) for k in dr.OUTPUTS]
    errs = dr.per_output_errors(got, ref[:5], ref[5:])
    print("%s: depth entry, max error / scale: %s" % (name, "  ".join("%s %.4g (bound %.3g)" % (k, errs[k], host.BOUND_BAD["depth"][k])
                                                                      for k in dr.OUTPUTS)))
    for k in dr.OUTPUTS:
        assert errs[k] <= host.BOUND_BAD["depth"][k], (name, k, errs[k])


@pytest.mark.parametrize("name", RGB)
def test_contribution(tmp_path, name):
    bad, twin, rep_dev, rep, a, b = _pair(tmp_path, "rgb", name)
    out = {}
    for tag, scene in (("bad", a), ("twin", b)):
        frame, st = hip_con._forward(scene, "ref_cpu", TILE)
        con = hip_con._contribution(scene, "ref_cpu", TILE, st)
        other = scene.render_contribution_hip(1, tile_size=TILE)
        assert all(torch.equal(x, y) for x, y in zip(con, other))
        out[tag] = dict(weight_max=con.weight_max, weight_sum=con.weight_sum, pixels=con.pixels, views=con.views)
    _hold_pair(name, out["bad"], out["twin"], rep_dev)
    ref = cr.ref_cpu(_oracle_pre(a, bad), W_, H_, TILE, N)
    wmax, wsum, pixels, views = (_np(out["bad"][k]) for k in ("weight_max", "weight_sum", "pixels", "views"))
    err, off = cr.compare(wmax, pixels, ref)
    err_sum = float(np.abs(wsum - ref.weight_sum).max() / max(1.0, ref.weight_sum.max()))
    print("%s: |weight_max - restatement| %.3g, weight_sum %.3g of its largest (bound %.3g), %d rows composited" % (
        name, err, err_sum, hip_con.TOL, int((pixels > 0).sum())))
    assert err <= hip_con.TOL and err_sum <= hip_con.TOL and off.size == 0 and (pixels > 0).sum() >= N // 2
    assert not views[rep].any() and (views[list(brc.DEGENERATE.values())] == 1).all()


# ================================================================================================ std_3dgs
def _std_pair(tmp_path, name, antialiased):
    built, rows = host.std_built(name, antialiased)
    rep = brc.replaced(rows)
    scenes = {}
    for tag in ("bad", "twin"):
        case = built[tag]
        scenes[tag] = _build(tmp_path / tag, case["sc"])
        assert _same_camera(case["cam"], _oracle_cam(scenes[tag])), "the host walked another camera"
    return built, torch.from_numpy(rep).to(DEV), rep, scenes


STD_KEYS = ("colors", "opacity", "points", "scales", "quaternions", "grad_means2d", "screen_radius")


@pytest.mark.parametrize("name", STD)
def test_std3dgs_entry_plain_and_with_published_rectangles(tmp_path, name):
    built, rep_dev, rep, scenes = _std_pair(tmp_path, name, False)
    for published in (False, True):
        out = {}
        for tag in ("bad", "twin"):
            case, scene = built[tag], scenes[tag]
            gf = torch.from_numpy(case["g"]).to(DEV)
            frame, st = hip_std._forward(scene, case, published_rects=published)
            outs = hip_std._backward(scene, case, frame, st, gf, published=published)
            assert len(outs) == 7
            out[tag] = dict(zip(STD_KEYS, (o.reshape(N, -1) for o in outs)), frame=frame)
            out[tag + " instances"], out[tag + " raw"] = st["n_instances"], outs
        assert out["bad instances"] == out["twin instances"] and (published or out["bad instances"] <= built["bad"]["inst"])
        tag = name + (" published" if published else "")
        _hold_pair(tag, out["bad"], out["twin"], rep_dev)
        err = hip_std._errors(built["bad"], out["bad raw"])
        print("%s: kernel vs restatement, max error / scale: %s" % (tag, "  ".join("%s %.3g" % (k, err[k]) for k in hip_std.KEYS)))
        for k in hip_std.KEYS:
            assert err[k] <= host.BOUND_BAD["std"][k], (tag, k, err[k], host.BOUND_BAD["std"][k])
        radius = _np(out["bad"]["screen_radius"]).reshape(-1)
        assert (radius[list(brc.DEGENERATE.values())] > 0).sum() >= len(brc.DEGENERATE) - 1       # logit -80 composites nowhere


@pytest.mark.parametrize("name", STD)
def test_std3dgs_antialiased_entry(tmp_path, name):
    built, rep_dev, rep, scenes = _std_pair(tmp_path, name, True)
    out = {}
    for tag in ("bad", "twin"):
        case, scene = built[tag], scenes[tag]
        gf = torch.from_numpy(case["g"]).to(DEV)
        frame, st = hip_aa._frame(scene, case, antialiased=True)
        outs = hip_aa._backward(scene, case, frame, st, gf)
        assert len(outs) == 7
        out[tag] = dict(zip(STD_KEYS, (o.reshape(N, -1) for o in outs)), frame=frame)
        out[tag + " raw"] = outs
    _hold_pair(name + " antialiased", out["bad"], out["twin"], rep_dev)
    got, err = hip_aa._errors(built["bad"]["ref"], out["bad raw"])
    print("%s antialiased: kernel vs restatement, max error / scale: %s" % (name, "  ".join("%s %.3g" % (k, err[k]) for k in aar.KEYS)))
    for k in aar.KEYS:
        assert err[k] <= host.BOUND_BAD["aa"][k], (name, k, err[k], host.BOUND_BAD["aa"][k])


@pytest.mark.parametrize("name", STD)
def test_std3dgs_contribution(tmp_path, name):
    built, rep_dev, rep, scenes = _std_pair(tmp_path, name, False)
    assert hip_con.BG == built["bad"]["bg"]
    out = {}
    for tag in ("bad", "twin"):
        frame, st = hip_con._forward(scenes[tag], "std_3dgs", TILE)
        con = hip_con._contribution(scenes[tag], "std_3dgs", TILE, st)
        gc0 = hip_con._colour_gradient(scenes[tag], "std_3dgs", TILE, frame, st)
        assert torch.equal(_bits(con.weight_sum), _bits(gc0))
        out[tag] = dict(weight_max=con.weight_max, weight_sum=con.weight_sum, pixels=con.pixels, views=con.views)
    _hold_pair(name, out["bad"], out["twin"], rep_dev)
    case = built["bad"]
    ref = cr.std_3dgs(case["R"], case["W"], case["H"], N)
    wmax, wsum, pixels, views = (_np(out["bad"][k]) for k in ("weight_max", "weight_sum", "pixels", "views"))
    err, off = cr.compare(wmax, pixels, ref)
    print("%s: |weight_max - restatement| %.3g (bound %.3g), %d rows composited" % (name, err, hip_con.TOL, int((pixels > 0).sum())))
    assert not ref.excluded.any() and err <= hip_con.TOL and off.size == 0 and not views[rep].any()


# ================================================================================================ the SH link
def _sh_grads(scene, W, Wd=None):
    """(frame, {name: gradient}) of an SH scene through the geometry entry, or with `Wd` through the depth entry."""
    g = scene.gaussians
    for name in SH_TRAINED:
        getattr(g, name).requires_grad_(True)
        getattr(g, name).grad = None
    if Wd is None:
        frame = scene.render_image_hip(1, tile_size=TILE, geometry_gradients=True)
        (frame * W).sum().backward()
    else:
        frame, depth = scene.render_image_depth_hip(1, tile_size=TILE)
        ((frame * W).sum() + (depth * Wd).sum()).backward()
    out = {name: getattr(g, name).grad.detach().clone() for name in SH_TRAINED}
    for name in SH_TRAINED:
        getattr(g, name).requires_grad_(False)
        getattr(g, name).grad = None
    return frame.detach(), out


@pytest.mark.parametrize("name", SH)
def test_sh_link_behind_the_geometry_and_depth_entries(tmp_path, name):
    bad, twin, rep_dev, rep, a, b = _pair(tmp_path, "sh", name)
    active = brc.sh_case(name)[4]
    W, Wd = _W((W_, H_, 3), 5), _W((W_, H_, 2), 6)
    out = {}
    for tag, scene in (("bad", a), ("twin", b)):
        frame, grads = _sh_grads(scene, W)
        _, dgrads = _sh_grads(scene, W, Wd)
        _, outs, _ = _entry(scene, W, TILE, screen=False, camera=False)
        gsh, gview = scene._sh_backward(1, outs[0], with_points=True)
        assert torch.equal(_bits(grads["sh"]), _bits(gsh)) and torch.equal(_bits(grads["points"]), _bits(outs[2] + gview))
        out[tag] = dict(grads, frame=frame, view_share=gview, dL_dcolour=outs[0], **{"depth_" + k: v for k, v in dgrads.items()})
    out["bad"]["sh"], out["twin"]["sh"] = out["bad"]["sh"].reshape(N, -1), out["twin"]["sh"].reshape(N, -1)
    out["bad"]["depth_sh"], out["twin"]["depth_sh"] = out["bad"]["depth_sh"].reshape(N, -1), out["twin"]["depth_sh"].reshape(N, -1)
    _hold_pair(name, out["bad"], out["twin"], rep_dev)
    # the inactive bands of dL/dsh are exact +0 in every row
    k_active = (active + 1) ** 2
    assert not _bits(out["bad"]["sh"].reshape(N, 16, 3)[:, k_active:]).any()
    # the link against float64 on the rows that have a view direction (tests/test_hip_sh_backward.py's check and bound)
    keep = ~rep
    pts, sh = bad["points"][keep], np.ascontiguousarray(bad["sh"][keep][:, :k_active])
    centre = np.asarray(a.images[1].camera_center_host, np.float64)
    gc = _np(out["bad"]["dL_dcolour"])[keep]
    pre = shr.forward(pts, sh, active, centre)[0]
    sure = np.abs(pre) >= shr.NEAR_ZERO
    ref_sh, ref_mean, scale_sh, scale_mean = shr.backward(pts, sh, active, centre, gc)
    got_sh = _np(out["bad"]["sh"]).reshape(N, 16, 3)[keep][:, :k_active]
    e_sh = shr.scaled_error(got_sh, ref_sh, scale_sh, keep=sure[:, None, :])
    e_mean = shr.scaled_error(_np(out["bad"]["view_share"])[keep], ref_mean, scale_mean, keep=sure.all(1)[:, None])
    print("%s: SH link vs restatement, max error / scale: sh %.4g (bound %.3g), points %.4g (bound %.3g)" % (
        name, e_sh, sh_host.BOUND["sh"], e_mean, sh_host.BOUND["points"]))
    assert (~sure).mean() <= 0.01 and e_sh <= sh_host.BOUND["sh"] and e_mean <= sh_host.BOUND["points"], (e_sh, e_mean)


@pytest.mark.parametrize("name", SH)
def test_sh_scene_s_pose_gradient_is_finite_and_the_twin_s(tmp_path, name):
    """dL/dworld2view of an SH scene holds -sum over ALL rows of the view-direction share: one NaN row would lose the pose."""
    bad, twin, rep_dev, rep, a, b = _pair(tmp_path, "sh", name)
    W = _W((W_, H_, 3), 5)
    got = {}
    for tag, scene in (("bad", a), ("twin", b)):
        g, im = scene.gaussians, scene.images[1]
        g.sh.requires_grad_(True)
        im.world2view.requires_grad_(True)
        frame = scene.render_image_hip(1, tile_size=TILE, camera_gradients=True)
        (frame * W).sum().backward()
        _, outs, _ = _entry(scene, W, TILE)
        got[tag] = dict(total=im.world2view.grad.detach().clone(), grad_world2view=outs[-2], grad_full_proj=outs[-1], sh=g.sh.grad.reshape(N, -1).clone())
        g.sh.requires_grad_(False)
        g.sh.grad = None
    rep_all = rep_dev
    _hold_pair(name, got["bad"], got["twin"], rep_all)
    assert got["bad"]["total"].abs().max() > 0 and not torch.equal(got["bad"]["total"], got["bad"]["grad_world2view"])


# ================================================================================================ the kernel alone
@pytest.mark.parametrize("stored,active", [(3, 3), (2, 2), (1, 1), (3, 1), (3, 2), (2, 1), (0, 0), (2, 0)])
def test_sh_backward_zero_row_rule_on_rows_without_a_view_direction(stored, active):
    """sh_backward_restatement.CASES-style inputs (257 rows: two blocks) with rows whose mean is NaN, +Inf, -Inf, the centre
    itself, and a finite row with a NaN coefficient, all with dL/dcolour = 0: exact zeros in both outputs; every other row
    keeps the bits it has without those rows' neighbours being bad."""
    import ctypes

    from intro_to_gaussian_splatting_amd import _ffi
    from test_hip_sh_backward import _stream

    lib = _ffi.load()
    n = 257
    pts, sh, gc = shr.case_inputs(n, stored, 0)
    centre = shr.CENTER
    rows = {0: (np.nan, 0), 63: (np.inf, 1), 64: (-np.inf, 2), 255: None, 256: "coefficient", 128: (np.nan, 2)}
    clean = (pts.copy(), sh.copy(), gc.copy())
    for i, what in rows.items():
        gc[i] = 0.0
        clean[2][i] = 0.0
        if what is None:
            pts[i] = centre
        elif what == "coefficient":
            sh[i, 0, 1] = np.nan
        else:
            pts[i, what[1]] = what[0]
    bad_rows = torch.tensor(sorted(rows), device=DEV)
    outs = {}
    for tag, (p, s, g) in (("bad", (pts, sh, gc)), ("clean", clean)):
        tp, ts, tg = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (p, s, g))
        gsh = torch.full((n, (stored + 1) ** 2, 3), float("nan"), device=DEV)
        gview = torch.full((n, 3), float("nan"), device=DEV)
        c = (ctypes.c_float * 3)(*[float(v) for v in centre])
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        _ffi.check(lib.gsx_sh_backward_active(ptr(tp), ptr(ts), stored, active, n, c, ptr(tg), ptr(gsh), ptr(gview), _stream()))
        torch.cuda.synchronize()
        outs[tag] = (gsh, gview)
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[bad_rows] = False
    for a_, b_ in zip(outs["bad"], outs["clean"]):
        assert torch.isfinite(a_).all()
        assert not (_bits(a_)[bad_rows] & 0x7FFFFFFF).any()
        assert torch.equal(_bits(a_)[keep], _bits(b_)[keep])
    assert outs["bad"][0].abs().max() > 0 and (outs["bad"][1].abs().max() > 0) == (active > 0)


# ================================================================================================ a fit
RGB_LR = {"points": 2e-4, "scales": 2e-3, "quaternions": 1e-3, "opacity": 2e-2, "colors": 5e-3}
SH_LR = {"points": 2e-4, "scales": 2e-3, "quaternions": 1e-3, "opacity": 2e-2, "sh": 5e-3}
POSES = dict(lr_rotation=2e-3, lr_translation=5e-3, betas=(0.9, 0.99), eps=1e-9)
FITS = {"rgb ref_cpu, refine_poses": ("rgb", "base", dict(refine_poses=POSES)),
        "sh ref_cpu, refine_poses": ("sh", "sh3", dict(refine_poses=POSES)),
        "sh std_3dgs": ("sh", "sh3_std", dict(semantics="std_3dgs", background=cc.STD_BG))}


@pytest.mark.parametrize("fit", list(FITS))
def test_three_trainer_steps_are_the_twin_s_and_leave_the_unlisted_rows_alone(tmp_path, fit):
    from intro_to_gaussian_splatting_amd import Trainer

    kind, name, kw = FITS[fit]
    bad, twin, rep_dev, rep, a, b = _pair(tmp_path, kind, name)
    render = dict(tile_size=TILE, **{k: v for k, v in kw.items() if k in ("semantics", "background")})
    with torch.no_grad():
        target = (b.render_image_hip(1, **render) * 0.8 + 0.05).clone()
    assert torch.isfinite(target).all()
    names = SH_TRAINED if kind == "sh" else ("points", "scales", "quaternions", "opacity", "colors")
    result = {}
    for tag, scene in (("bad", a), ("twin", b)):
        before = {k: getattr(scene.gaussians, k).detach().clone() for k in names}
        trainer = Trainer(scene, {1: target}, lr=SH_LR if kind == "sh" else RGB_LR, lambda_dssim=0.2, tile_size=TILE,
                          statistic="screen", seed=5, **kw)
        losses = torch.stack([trainer.step()[0] for _ in range(3)])
        assert all(not trainer.events_at(s) for s in (1, 2, 3))
        g, opt, dc = trainer.gaussians, trainer.opt, trainer.density
        state = {k: getattr(g, k).detach().reshape(N, -1) for k in names}
        state.update({"m_" + k: opt.exp_avg[k].reshape(N, -1) for k in names})
        state.update({"v_" + k: opt.exp_avg_sq[k].reshape(N, -1) for k in names})
        result[tag] = dict(losses=losses, state=state, before=before, grad_sum=dc.grad_sum, seen=dc.seen, radius_max=dc.radius_max,
                           pose=scene.images[1].world2view.detach().clone())
    ra, rb = result["bad"], result["twin"]
    print("%s: losses %s" % (fit, ra["losses"][:, 0].tolist()))
    assert torch.isfinite(ra["losses"]).all() and torch.equal(_bits(ra["losses"]), _bits(rb["losses"]))
    keep = ~rep_dev
    for key, v in ra["state"].items():
        assert torch.equal(_bits(v)[keep], _bits(rb["state"][key])[keep]), key
        assert torch.isfinite(v[keep]).all(), key
    for k in names:         # an UNLISTED row keeps its own bits: a NaN stays that NaN, a zero quaternion stays zero
        now, was = _bits(getattr(a.gaussians, k).detach().reshape(N, -1)), _bits(ra["before"][k].reshape(N, -1))
        assert torch.equal(now[rep_dev], was[rep_dev]), k
        assert not torch.equal(now[keep], was[keep]), k
        # (the moments of an UNLISTED row are its own too, and not all zero: the Trainer's Adam steps every row, and the scales'
        # moments are of dL/dlog s = s dL/ds, which is NaN * 0 for the row with a NaN scale.  Nothing reads them.)
    # the screen statistic never counted an UNLISTED row
    for key in ("grad_sum", "seen", "radius_max"):
        v = ra[key]
        assert not (v[rep_dev] != 0).any() and torch.equal(v[keep], rb[key][keep]) and (v[keep] != 0).any(), key
    assert torch.isfinite(ra["pose"]).all() and torch.equal(_bits(ra["pose"]), _bits(rb["pose"]))
    if "refine_poses" in kw:
        with torch.no_grad():
            fresh = _build(tmp_path / "fresh", twin if kind == "rgb" else brc.sh_case(name)[1]).images[1].world2view
        assert not torch.equal(ra["pose"], fresh.detach())
