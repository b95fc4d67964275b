"""The screen-space densification statistic, host side: the header and the binding; every refusal of the three new calls by
name, before any HIP call; the Python surface's ValueErrors; the float64 restatement of dL/d(NDC mean)
(tests/screen_gradient_restatement.py) against the reference's own autograd (tests/golden/screengrad_*.npz,
tools/capture_screen_grad_golden.py) and, through an identity, against the pinned chain of
tests/geometry_backward_restatement.py; exact zeros; the float32 restatements of the two density calls against an independent
float64 composition.

E_REF_SCREEN: the worst per-Gaussian scaled error (geometry_backward_restatement.per_gaussian_error) of the REFERENCE'S OWN
float32 dL/dmean, taken to NDC units, against the float64 restatement over all fourteen screengrad_ fixtures, measured on the
CPU:
    4.308e-08  (tile12_dense_52x40_n900)
and per fixture, error / scale and max-normalised error:
    tile2_40x32_n80          5.756e-09  2.38e-07        tiny_48x48_n600     3.436e-08  1.61e-07
    small_64x48_n300         1.830e-08  2.92e-07        wide_64x64_n400     1.786e-08  1.44e-06
    small_80x64_n120_tile8   9.633e-09  1.78e-07        cull_96x80_n400     1.588e-08  3.38e-07
    tile12_dense_52x40_n900  4.308e-08  2.18e-06        rows1_48x48_n1      3.963e-10  1.09e-08
    tile20_64x64_n300        7.302e-09  3.99e-07        rows3_48x48_n3      2.382e-09  3.85e-07
    tile32_96x96_n400        1.633e-08  5.10e-07        rows1_48x48_n500    3.501e-09  3.17e-07
    needle_160x160_n110      2.873e-09  2.97e-06        rows3_48x48_n500    5.236e-09  2.27e-07
The unit is the Gaussian's own error scale, the formula on absolute values (it adds where the true sums cancel), so these sit
below float32's unit roundoff, as test_geometry_backward_host.py's do.  The kernel is held to 12 E_REF_SCREEN against the
restatement and 13 E_REF_SCREEN against the fixtures (tests/test_hip_screen_statistic.py), the ratio the merged geometry and
colour tests grant.
"""
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_preprocessed, load_golden, oracle_camera

import density_restatement as dr
import geometry_backward_restatement as gbr
import screen_gradient_restatement as sgr
from test_density_host import PTR, RULES, WS, _rules, case
from test_geometry_backward_host import GEOM_SCENES, fixture_inputs, forward_fixture

E_REF_SCREEN = 4.308e-8
BOUND_RESTATEMENT = 12 * E_REF_SCREEN
BOUND_FIXTURE = 13 * E_REF_SCREEN
E_REF_SLACK = 1.001         # the reference against the restatement is E_REF_SCREEN by definition; the last printed digit


@functools.lru_cache(maxsize=None)
def restated(name):
    """Computed once per scene and left unchanged: (pre, n, width, height, tile, (S, Sabs), gn (n,2), scale (n,), reference's
    gradient in NDC units scattered to rows (n,2))."""
    gg, base = fixture_inputs(name)
    pre = golden_preprocessed(forward_fixture(name))
    w, h, tile = int(base["width"]), int(base["height"]), int(base["tile"])
    n = base["points"].shape[0]
    mom = gbr.moments(pre, base["image"], base["W"], w, h, tile)
    gn, scale = sgr.screen_gradient(pre, n, base["image"], base["W"], w, h, tile, moments=mom)
    ref_xy = load_golden("screengrad_" + name)["grad_points_xy"]
    assert ref_xy.dtype == np.float32 and ref_xy.shape == (np.asarray(pre.order).shape[0], 2)
    ref = np.zeros((n, 2))
    ref[np.asarray(pre.order, np.int64)] = ref_xy.astype(np.float64) * np.array(sgr.half_extents(w, h))
    return pre, n, w, h, tile, mom, gn, scale, ref


# ---- C ABI
def test_header_declares_and_ffi_binds_the_three_calls():
    from intro_to_gaussian_splatting_amd import _ffi
    import test_cabi

    hdr = open(os.path.join(ROOT, "include", "gsx.h")).read()
    declared = test_cabi._declared_functions()
    for name, n_args in (("gsx_render_backward_screen", 21), ("gsx_density_accumulate_screen", 7), ("gsx_density_plan_screen", 12)):
        assert re.search(r"GSX_API\s+\w+\s+%s\(" % name, hdr) and name in declared, name
        assert len(_ffi.SIGNATURES[name][1]) == n_args, name
        assert hasattr(_ffi.load(), name)
    assert len(_ffi.SIGNATURES["gsx_render_backward_geometry"][1]) == 19 and len(_ffi.SIGNATURES["gsx_density_plan"][1]) == 10
    assert re.search(r"#define\s+GSX_VERSION\s+305\b", hdr) and _ffi.load().gsx_version() == 305
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    assert "zero gradient or not" in flat and "published denominator counts visibility" in flat      # the stated difference
    assert "gmx = -0.5f * (2.0f * q00 * S1 + (q01 + q10) * S2)" in flat                                  # the operation order


def test_refusals_name_the_argument_and_need_no_gpu():
    from intro_to_gaussian_splatting_amd import _ffi

    lib = _ffi.load()

    def acc(grad=PTR, radius=PTR, n=100, grad_sum=PTR, seen=PTR, radius_max=PTR):
        return lib.gsx_density_accumulate_screen(grad, radius, n, grad_sum, seen, radius_max, None)

    for kw, word in ((dict(grad=None), b"grad_means2d"), (dict(radius=None), b"screen_radius"), (dict(grad_sum=None), b"grad_sum"),
                     (dict(seen=None), b"seen"), (dict(radius_max=None), b"radius_max"), (dict(n=-1), b"n = -1"),
                     (dict(n=2 ** 30 + 1), b"n = ")):
        assert acc(**kw) == _ffi.GSX_ERR_INVALID_ARGUMENT, kw
        assert word in lib.gsx_last_error(), (kw, lib.gsx_last_error())
    assert acc(n=0) == _ffi.GSX_OK and acc(n=0, grad=None, radius=None, grad_sum=None, seen=None, radius_max=None) == _ffi.GSX_OK

    big = lib.gsx_density_workspace_bytes(100)
    counts = (ctypes.c_int64 * 4)(7, 7, 7, 7)

    def plan(grad_sum=PTR, seen=PTR, scales=PTR, opacity=PTR, radius_max=PTR, prune_radius=20.0, n=100, rules=None, ws=WS,
             ws_bytes=big, out=counts):
        rules = ctypes.byref(_rules()) if rules is None else rules
        return lib.gsx_density_plan_screen(grad_sum, seen, scales, opacity, radius_max, prune_radius, n, rules, ws, ws_bytes, out, None)

    nan = float("nan")
    for kw, word in ((dict(prune_radius=nan), b"prune_radius"), (dict(prune_radius=nan, radius_max=None), b"prune_radius"),
                     (dict(grad_sum=None), b"grad_sum"), (dict(seen=None), b"seen"), (dict(scales=None), b"scales"),
                     (dict(opacity=None), b"opacity_logit"), (dict(n=-1), b"n = -1"), (dict(n=2 ** 30 + 1), b"n = "),
                     (dict(rules=ctypes.POINTER(_ffi.GsxDensityRules)()), b"rules"), (dict(ws=None), b"workspace"),
                     (dict(ws=WS + 128), b"256-byte aligned"), (dict(out=None), b"counts_host"),
                     (dict(rules=ctypes.byref(_rules(flags=1))), b"flags"),
                     (dict(rules=ctypes.byref(_rules(split_shrink=nan))), b"split_shrink")):
        assert plan(**kw) == _ffi.GSX_ERR_INVALID_ARGUMENT, kw
        assert word in lib.gsx_last_error(), (kw, lib.gsx_last_error())
    assert plan(ws_bytes=big - 1) == _ffi.GSX_ERR_WORKSPACE_TOO_SMALL
    assert list(counts) == [7, 7, 7, 7]
    for kw in (dict(), dict(radius_max=None), dict(prune_radius=float("inf"))):       # nothing to do; NULL radii and +inf are fine
        counts[:] = [7, 7, 7, 7]
        assert plan(n=0, ws_bytes=lib.gsx_density_workspace_bytes(0), **kw) == _ffi.GSX_OK and list(counts) == [0, 0, 0, 0]

    # gsx_render_backward_screen: gsx_render_backward_geometry's refusals, and its own required output
    cam = _ffi.GsxCamera()

    def screen(camera=True, outs=(PTR,) * 7):      # grad_colors, grad_opacity_logit, three geometry outputs, the two new ones
        return lib.gsx_render_backward_screen(ctypes.byref(cam) if camera else None, *([PTR] * 5), 10, 16, PTR, PTR, *outs, None,
                                              None, WS, 1 << 20, None)

    for kw, word in ((dict(outs=(PTR,) * 5 + (None, PTR)), b"grad_means2d is NULL"), (dict(outs=(PTR, PTR, None) + (PTR,) * 4), b"grad_means3d"),
                     (dict(outs=(PTR,) * 4 + (None, PTR, PTR)), b"grad_quats"), (dict(camera=False), b"camera is NULL")):
        assert screen(**kw) == _ffi.GSX_ERR_INVALID_ARGUMENT, kw
        assert word in lib.gsx_last_error(), (kw, lib.gsx_last_error())
    cam.width = cam.height = 0                # (a NULL screen_radius is not a refusal: the next check, the frame's size, speaks)
    assert lib.gsx_render_backward_screen(ctypes.byref(cam), *([PTR] * 5), 10, 16, PTR, PTR, *([PTR] * 6), None, None, WS, 1 << 20,
                                          None) != _ffi.GSX_OK
    assert b"screen_radius" not in lib.gsx_last_error() and b"grad_means2d" not in lib.gsx_last_error()


# ---- Python surface, as far as it goes without a GPU
def test_python_surface_keywords_and_refusals(tmp_path):
    from intro_to_gaussian_splatting_amd import DensityControl, Gaussians, GaussianScene
    from intro_to_gaussian_splatting_amd.synthetic import make_scene, write_colmap_text

    for fn in (GaussianScene.render_image, GaussianScene.render_image_hip):
        assert inspect.signature(fn).parameters["screen_statistics"].default is False
    p = inspect.signature(DensityControl.__init__).parameters
    assert p["statistic"].default == "points" and p["prune_radius"].default == float("inf")

    sc = make_scene(8, 32, 32, seed=0)
    write_colmap_text(str(tmp_path), sc)
    g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"], device="cpu")
    scene = GaussianScene(str(tmp_path), g)
    assert scene.screen_statistics is None
    for fn in (scene.render_image, scene.render_image_hip):
        with pytest.raises(ValueError, match="screen_statistics=True needs geometry_gradients=True"):
            fn(1, screen_statistics=True)
    scene.screen_statistics = (1, torch.zeros((8, 2)), torch.zeros(8))
    scene.gaussians_changed()
    assert scene.screen_statistics is None
    with pytest.raises(ValueError, match="statistic='screen' needs scene"):
        DensityControl(g, statistic="screen")
    with pytest.raises(ValueError, match="statistic = 'viewspace' is neither"):
        DensityControl(g, scene=scene, statistic="viewspace")
    with pytest.raises(ValueError, match="prune_radius is NaN"):
        DensityControl(g, scene=scene, statistic="screen", prune_radius=float("nan"))
    with pytest.raises(ValueError, match="points is on cpu.*no CPU fallback"):       # past the new checks: the old one
        DensityControl(g, scene=scene, statistic="screen", prune_radius=20.0)
    doc = re.sub(r"\s+", " ", DensityControl.__doc__)
    assert "loss per NDC unit, the published convention" in doc


# ---- the float64 restatement
def test_every_geometry_scene_has_a_fixture_of_data_only():
    for name in GEOM_SCENES:
        path = os.path.join(ROOT, "tests", "golden", "screengrad_%s.npz" % name)
        assert os.path.getsize(path) <= 16 * 1024, path
        z = np.load(path)
        assert sorted(z.files) == ["grad_points_xy", "reference_backward_seconds", "reference_forward_seconds"], name


@pytest.mark.parametrize("name", GEOM_SCENES)
def test_restatement_matches_reference_autograd_per_gaussian(name):
    pre, n, w, h, tile, mom, gn, scale, ref = restated(name)
    assert np.abs(ref).max() > 0
    assert (np.abs(gn) <= scale[:, None] * (1 + 1e-9)).all()         # the scale bounds the gradient itself
    e = gbr.per_gaussian_error(ref, gn, scale)
    rel = np.abs(ref - gn).max() / np.abs(ref).max()
    print("%s: reference autograd vs restatement, max error / scale %.4g, max-normalised %.3g" % (name, e, rel))
    assert e <= E_REF_SCREEN * E_REF_SLACK, (name, e)
    assert rel <= 5e-6, (name, rel)


@pytest.mark.parametrize("name", ["small_64x48_n300", "tiny_48x48_n600", "wide_64x64_n400", "cull_96x80_n400"])
def test_the_pinned_chain_with_only_the_mean_s_moments_is_the_projection_s_jacobian(name):
    """gbr.chain with S[:, 2:] = 0 -- no gradient through the conic -- returns a dL/dpoints that is the restated dL/d(NDC mean)
    pushed through the float64 Jacobian of point -> NDC: the new restatement and the merged one state the same quantity."""
    pre, n, w, h, tile, (S, _), gn, scale, ref = restated(name)
    gg, base = fixture_inputs(name)
    order = np.asarray(pre.order, np.int64)
    st = gbr.stage1(base["points"][order], base["scales"][order], base["quaternions"][order], oracle_camera(forward_fixture(name)))
    S12 = S.copy()
    S12[:, 2:] = 0.0
    gp, gs, gq = gbr.chain(st, np.asarray(pre.inverse_covariance_2d, np.float64), S12)
    want = sgr.through_projection(st, gn[order])
    assert np.abs(want).max() > 0
    err = np.abs(gp - want).max() / np.abs(want).max()
    print("%s: chain(S1, S2 only) vs Jacobian of the restated gradient: %.3g relative" % (name, err))
    assert err <= 1e-12
    assert not gs.any() and not gq.any()


def test_culled_and_unlisted_rows_are_exact_zeros():
    name = "cull_96x80_n400"
    pre, n, w, h, tile, mom, gn, scale, ref = restated(name)
    fwd = load_golden(name)
    on = sgr.listed(pre, w, h, tile)
    order = np.asarray(pre.order, np.int64)
    culled = ~fwd["in_view"]
    listed_rows = np.zeros(n, bool)
    listed_rows[order[on]] = True
    unlisted = ~culled & ~listed_rows
    assert (int(culled.sum()), int(unlisted.sum()), int(listed_rows.sum())) == (112, 44, 244)
    radius = sgr.screen_radius(pre, n, on)
    dead = culled | unlisted
    assert not gn[dead].any() and not scale[dead].any() and not ref[dead].any()
    assert not radius[dead].view(np.uint32).any() and (radius[listed_rows] > 0).all()
    assert np.array_equal(radius[order[on]].view(np.uint32), np.asarray(pre.radius, np.float32)[on].view(np.uint32))
    # every listed Gaussian of this scene is also composited somewhere
    assert (np.abs(gn[listed_rows]).sum(1) > 0).all()


# ---- the two density calls: the float32 restatements against an independent float64 composition
def edge_case(n, seed=0):
    """(grad (n,2), radius (n), grad_sum, seen, radius_max): random rows with every edge row of the contract among the first
    ones -- radius 0, -0, negative, NaN; radius > 0 with a zero gradient; radius > 0 with a NaN gradient."""
    rs = np.random.RandomState(seed + n)
    g = (rs.normal(size=(n, 2)) * np.exp(rs.uniform(-8, 2, size=(n, 1)))).astype(np.float32)
    r = np.ceil(rs.uniform(0.0, 40.0, size=n)).astype(np.float32)
    r[rs.uniform(size=n) < 0.3] = 0.0
    edges = [(0.0, None), (np.nan, None), (3.0, (0.0, -0.0)), (5.0, (np.nan, 1.0)), (-0.0, None), (-2.0, None)]
    for i, (radius, grad) in enumerate(edges):
        if i < n:
            r[i] = radius
            if grad is not None:
                g[i] = grad
    return (g, r, rs.uniform(0, 3, size=n).astype(np.float32), rs.randint(0, 5, size=n).astype(np.uint32),
            np.ceil(rs.uniform(0.0, 40.0, size=n)).astype(np.float32))


def test_restatement_of_accumulate_screen_and_its_edge_rows():
    n = 300
    g, r, s0, c0, m0 = edge_case(n)
    s1, c1, m1 = sgr.accumulate_screen(g, r, s0, c0, m0)
    live = np.nan_to_num(r.astype(np.float64), nan=0.0) > 0
    assert 0 < live.sum() < n
    norm = np.hypot(g[:, 0].astype(np.float64), g[:, 1].astype(np.float64))
    for a, b in ((s1, s0), (c1, c0), (m1, m0)):         # a row that is not listed touches nothing: the bits stay
        assert np.array_equal(a[~live].view(np.uint32), b[~live].view(np.uint32))
    assert np.array_equal(c1[live], c0[live] + 1)
    assert np.array_equal(m1[live], np.maximum(m0[live], r[live]))
    ok = live & np.isfinite(norm)
    # two products, one sum, one root, one sum: at most four roundings of 2^-24 on the norm, one on the total
    assert (np.abs(s1[ok].astype(np.float64) - (s0[ok].astype(np.float64) + norm[ok])) <= 2.0 ** -24 * (4 * norm[ok] + s1[ok])).all()
    # the edge rows: radius 0 / NaN / -0 / negative untouched; a zero gradient still counts; a NaN gradient is added as it is
    assert not live[[0, 1, 4, 5]].any() and live[[2, 3]].all()
    assert c1[2] == c0[2] + 1 and s1[2] == s0[2] and m1[2] == max(m0[2], np.float32(3.0))
    assert c1[3] == c0[3] + 1 and np.isnan(s1[3]) and not np.isnan(m1[3])
    # a NaN radius_max stays a NaN (r > NaN fails)
    m0[2] = np.nan
    assert np.isnan(sgr.accumulate_screen(g, r, s0, c0, m0)[2][2])
    # gsx_density_accumulate, by contrast, does not see the zero-gradient row
    assert dr.accumulate(g[2:3], s0[2:3], c0[2:3])[1][0] == c0[2]


def plan_case(n, seed=0):
    c = case(n, "random", seed)
    rs = np.random.RandomState(seed + 5)
    radius_max = np.ceil(rs.uniform(0.0, 40.0, size=n)).astype(np.float32)
    radius_max[0::7] = 20.0               # exactly at the threshold: not pruned
    radius_max[1::11] = np.nan            # fails the comparison
    radius_max[2::13] = np.inf
    return c, radius_max


@pytest.mark.parametrize("prune_radius", [20.0, float("inf"), 0.0])
def test_restatement_of_plan_screen_against_an_independent_float64_composition(prune_radius):
    n = 1500
    c, radius_max = plan_case(n, 3)
    base_action, _, base_counts = dr.plan(c["grad_sum"], c["seen"], c["scales"], c["opacity"], RULES)
    action, prefix, counts = sgr.plan_screen(c["grad_sum"], c["seen"], c["scales"], c["opacity"], radius_max, prune_radius, RULES)
    with np.errstate(invalid="ignore"):
        big = radius_max.astype(np.float64) > prune_radius
    want = np.where(big, dr.PRUNE, base_action)
    assert np.array_equal(action, want)
    rows = dr.ROWS_OF[want]
    assert np.array_equal(prefix, np.cumsum(rows) - rows)
    assert counts == (int(rows.sum()), int((want == dr.PRUNE).sum()), int((want == dr.CLONE).sum()), int((want == dr.SPLIT).sum()))
    if prune_radius == 20.0:
        at, nan, inf = radius_max == 20.0, np.isnan(radius_max), np.isinf(radius_max)
        assert at.sum() > 100 and nan.sum() > 50 and inf.sum() > 50
        assert not big[at].any() and not big[nan].any() and big[inf].all() and 0 < big.sum() < n
        assert counts[1] > base_counts[1] and (action[big] == dr.PRUNE).all() and (base_action[big] != dr.PRUNE).any()
    if prune_radius == float("inf"):
        assert not big.any() and counts == base_counts
    none = sgr.plan_screen(c["grad_sum"], c["seen"], c["scales"], c["opacity"], None, prune_radius, RULES)
    assert np.array_equal(none[0], base_action) and none[2] == base_counts
