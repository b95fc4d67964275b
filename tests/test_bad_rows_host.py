"""Scenes with non-finite and degenerate rows (tests/bad_row_cases.py), host side: everything that can be fixed before a GPU
run.  The GPU side is tests/test_hip_bad_rows.py; what stage 1 does with each kind of row is in docs/lab_notes/bad_rows.md.

  * The oracles put every UNLISTED row on no tile and every DEGENERATE row on at least one: the C oracle for ref_cpu
    (oracle.c_oracle.preprocess / render), oracle/std3dgs_ref.py and its C port for std_3dgs.  No oracle had to be mended: the C
    oracle's tile range sends a NaN bound to no tile and clamps an infinite one before it converts (clamp_lo / clamp_hi of
    oracle/raster_cpu.c), the reference's own expressions (splat/utils.py:293-310, splat/gaussian_scene.py:209-217) being
    comparisons, which a NaN fails; std3dgs_ref._tile_index does the same.
  * The float64 restatements run on the bad scenes with warnings turned into errors, give exact zeros for the UNLISTED rows
    and, on all other rows, exactly the float64 values they give on the clean twin.  Five of them formed a float64 stage 1 of
    every visible row and multiplied it by a zero moment (0 * NaN); they now evaluate the rows on a tile list only
    (geometry_backward_restatement.listed_only), and sh_backward_restatement.backward applies the zero-row rule.
  * The conditions on the cases (how many rows carry gradient, which arrays of a DEGENERATE row are structurally zero, the std
    gradient mask's cap).
  * E_REF_BAD, the bound's unit.

E_REF_BAD[k] = max(existing E_REF[k], the float32 authority's own error against the float64 restatement on the clean twin).
For ref_cpu the authority is the reference's own autograd on the clean twins (tests/golden/*_badrow_*_twin_64x48_n300.npz,
tools/capture_{geometry,camera,depth,screen,abs}_grad_golden.py: BAD_ROW_TWINS); for std_3dgs and its anti-aliased variant
it is the float32 mirror of the restatement modules.  Measured here on the CPU (worst of the two twins / cases):
                               authority's error on the twins      existing E_REF       E_REF_BAD
    geometry    points         6.934e-09                           2.171e-08            2.171e-08
                scales         9.744e-09                           4.687e-07            4.687e-07
                quaternions    1.167e-09                           3.790e-09            3.790e-09
    camera      world2view     6.277e-11                           2.912e-09            2.912e-09
                full_proj      5.746e-10                           5.530e-09            5.530e-09
    depth       points         5.038e-08                           1.537e-08            5.038e-08   <- the twins set it
                scales         2.182e-08                           3.607e-08            3.607e-08
                quaternions    9.542e-10                           4.223e-09            4.223e-09
                colors         1.617e-07                           1.942e-07            1.942e-07
                opacity        2.776e-08                           4.861e-08            4.861e-08
    screen                     1.703e-08                           4.308e-08            4.308e-08
    abs                        1.378e-08                           2.942e-08            2.942e-08
    colours (frame alone)      1.617e-07                           TOL 8e-6 (test_backward_host.py), which stays the bound
    opacity (frame alone)      6.197e-08                           TOL 8e-6
    std_3dgs    colors 7.152e-08  opacity 1.030e-08  moments 2.235e-08  points 5.287e-09  scales 2.378e-09  means2d 1.077e-08:
                all below test_std3dgs_backward_host.E_REF; quaternions 2.890e-10 against 2.835e-10 <- the twins set it
    anti-aliased   colors 6.397e-08  opacity 6.730e-09  points 1.730e-09  scales 9.159e-10  quaternions 1.134e-10
                means2d 4.973e-09: all below test_antialias_host.E_REF_AA
Two units grow: the depth entry's dL/dpoints, by a factor 3.3 (the reference adds the frame's and the maps' shares in float32),
and the std_3dgs dL/dquaternions, by 2 %.  Which row sets either was not looked into.  The
kernels are held to BOUND_BAD = 12 E_REF_BAD against the restatement (tests/test_hip_bad_rows.py), the project's standing
margin for a summation order that differs from the mirror's.
"""
import functools
import os
import warnings

import numpy as np
import pytest

from conftest import ROOT, load_golden

import abs_gradient_restatement as agr
import antialias_restatement as aar
import backward_restatement
import bad_row_cases as brc
import camera_cases as cc
import camera_gradient_restatement as cgr
import contribution_restatement as cr
import depth_restatement as dr
import geometry_backward_restatement as gbr
import screen_gradient_restatement as sgr
import sh_backward_restatement as shr
import std3dgs_backward_restatement as sbr
import test_abs_statistic_host as abs_host
import test_antialias_host as aa_host
import test_camera_gradient_host as camera_host
import test_depth_host as depth_host
import test_geometry_backward_host as geometry_host
import test_screen_statistic_host as screen_host
import test_std3dgs_backward_host as std_host
from oracle import c_oracle, cpu_ref, std3dgs_ref
from test_backward_host import TOL

W_, H_, TILE, N = brc.WIDTH, brc.HEIGHT, brc.TILE, brc.N
TWINS = {"base": "badrow_base_twin_64x48_n300", "roll": "badrow_roll_twin_64x48_n300"}
FIVE = ("colors", "opacity", "points", "scales", "quaternions")

# The float32 authority's own error on the clean twins, per entry and output, in each restatement's own unit (measured by
# the tests below, which assert these figures within E_REF_SLACK), and E_REF_BAD = max(existing E_REF, that).
MEASURED = {
    "geometry": {"points": 6.934e-9, "scales": 9.744e-9, "quaternions": 1.167e-9},
    "camera": {"world2view": 6.277e-11, "full_proj": 5.746e-10},
    "depth": {"points": 5.038e-8, "scales": 2.182e-8, "quaternions": 9.542e-10, "colors": 1.617e-7, "opacity": 2.776e-8},
    "screen": 1.703e-8,
    "abs": 1.378e-8,
    "colours": 1.617e-7,
    "opacity": 6.197e-8,
    "std": {"colors": 7.152e-8, "opacity": 1.03e-8, "moments": 2.235e-8, "points": 5.287e-9, "scales": 2.378e-9,
            "quaternions": 2.89e-10, "means2d": 1.077e-8},
    "aa": {"colors": 6.397e-8, "opacity": 6.73e-9, "points": 1.73e-9, "scales": 9.159e-10, "quaternions": 1.134e-10,
           "means2d": 4.973e-9},
}
E_REF_SLACK = 1.001
_EXISTING = {"geometry": geometry_host.E_REF, "camera": camera_host.E_REF, "depth": depth_host.E_REF,
             "screen": screen_host.E_REF_SCREEN, "abs": abs_host.E_REF_ABS, "std": std_host.E_REF, "aa": aa_host.E_REF_AA}


def _max(measured, existing):
    return {k: max(v, existing[k]) for k, v in measured.items()} if isinstance(measured, dict) else max(measured, existing)


E_REF_BAD = {entry: _max(MEASURED[entry], _EXISTING[entry]) for entry in _EXISTING}
BOUND_BAD = {entry: ({k: 12 * v for k, v in e.items()} if isinstance(e, dict) else 12 * e) for entry, e in E_REF_BAD.items()}
# colours and opacity logits of the frame alone are held to test_backward_host.py's TOL, as everywhere


# ----------------------------------------------------------------------------- shared, computed once
def host_view(sc):
    """(cpu_ref.Camera, GaussianImage) of a scene dict as the scene object builds them, on the CPU."""
    from intro_to_gaussian_splatting_amd import GaussianImage
    from intro_to_gaussian_splatting_amd.colmap import Camera, Image

    im = GaussianImage(Camera(1, "PINHOLE", int(sc["width"]), int(sc["height"]),
                              np.array([sc["fx"], sc["fy"], sc["cx"], sc["cy"]], np.float64)),
                       Image(1, np.asarray(sc["qvec"]), np.asarray(sc["tvec"]), 1, "v"), device="cpu")
    c = im.gsx_camera()
    return cpu_ref.Camera(im.world2view.numpy(), im.full_proj_transform.numpy(), np.float32(c.tan_fovx), np.float32(c.tan_fovy),
                          np.float32(c.fx), np.float32(c.fy), c.width, c.height), im


def driving(seed, channels=3):
    return np.random.default_rng(seed).standard_normal((W_, H_, channels)).astype(np.float32)


def on_a_list(pre, n):
    """bool (n,), ORIGINAL row order: the row is on at least one tile list of the frame."""
    on = np.zeros(n, bool)
    on[np.asarray(pre.order, np.int64)[sgr.listed(pre, W_, H_, TILE)]] = True
    return on


def sh_colours(sc, degree):
    """The colours the SH forward gives the rows (float32 port, oracle.cpu_ref.sh_to_rgb); a row without a view direction
    or with a NaN coefficient gets NaN, which no list carries."""
    k = (degree + 1) ** 2
    with np.errstate(all="ignore"):
        return cpu_ref.sh_to_rgb(sc["points"], np.ascontiguousarray(sc["sh"][:, :k]), degree, brc.camera_centre(sc)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def forward_of(kind, name):
    """{"bad" / "twin": dict(sc, cam, pre, frame, inst, on)} of an RGB or an SH case under ref_cpu, and the replaced rows."""
    if kind == "rgb":
        bad, twin, rows = brc.rgb_case(name)
        colours = {"bad": bad["colors"], "twin": twin["colors"]}
    else:
        bad, twin, rows, _, active = brc.sh_case(name)
        colours = {"bad": sh_colours(bad, active), "twin": sh_colours(twin, active)}
    cam, _ = host_view(bad)
    out = {}
    for tag, sc in (("bad", bad), ("twin", twin)):
        pre = c_oracle.preprocess(sc["points"], colours[tag], sc["scales"], sc["quaternions"], sc["opacity"], cam)
        frame, _, inst = c_oracle.render(pre, W_, H_, TILE)
        out[tag] = dict(sc=sc, cam=cam, pre=pre, frame=frame, inst=inst, on=on_a_list(pre, N), colours=colours[tag])
    return out, rows


def restate_all(f, W, Wd):
    """Every ref_cpu restatement of one forward_of entry, in ORIGINAL row order: name -> tuple of arrays."""
    sc, cam, pre, frame = f["sc"], f["cam"], f["pre"], f["frame"]
    geo = (sc["points"], sc["scales"], sc["quaternions"], cam)
    out = {}
    out["colour"] = backward_restatement.backward(pre, frame, W, W_, H_, TILE, N, with_scale=True)
    out["geometry"] = gbr.geometry_backward(pre, *geo, frame, W, W_, H_, TILE, with_scale=True)
    out["screen"] = sgr.screen_gradient(pre, N, frame, W, W_, H_, TILE)
    out["abs"] = agr.abs_gradient(pre, N, frame, W, W_, H_, TILE, with_scale=True)
    mom = gbr.moments(pre, frame, W, W_, H_, TILE)
    args = (pre,) + geo + (None, None, W_, H_, TILE)
    out["camera"] = cgr.camera_backward(*args, moments=mom) + cgr.camera_backward(*args, absolute=True, moments=mom)
    fr, D, A, _ = dr.forward(pre, W_, H_, TILE)
    depth = np.stack([D, A], -1).astype(np.float32)
    out["maps"] = (fr, D, A)
    out["depth"] = dr.depth_backward(pre, *geo, frame, W, depth, Wd, W_, H_, TILE, with_scale=True)
    con = cr.ref_cpu(pre, W_, H_, TILE, N)
    out["contribution"] = tuple(np.asarray(x) for x in con)
    return out


@functools.lru_cache(maxsize=None)
def restated(kind, name):
    """(restate_all of the bad scene with warnings as errors, of the twin, the replaced rows' mask)."""
    fwd, rows = forward_of(kind, name)
    W, Wd = driving(5), driving(6, 2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        bad = restate_all(fwd["bad"], W, Wd)
    return bad, restate_all(fwd["twin"], W, Wd), brc.replaced(rows)


@functools.lru_cache(maxsize=None)
def std_built(name, antialiased):
    """{"bad" / "twin": the sibling host file's backward case dict} of a std case, walked on the scene object's camera."""
    bad, twin, rows = brc.std_case(name)
    cam, _ = host_view(bad)
    out = {}
    for tag, sc in (("bad", bad), ("twin", twin)):
        with warnings.catch_warnings():
            if tag == "bad":
                warnings.simplefilter("error")
            args = (sc, TILE, cc.STD_BG)
            out[tag] = (aa_host.build_backward(aa_host.build_case(*args, cam=cam, colors=sc["colors"])) if antialiased else
                        std_host.build_backward(std_host.build_tuple(*args, cam=cam, colors=sc["colors"])))
    return out, rows


RGB, SH, STD = list(brc.RGB_CASES), list(brc.SH_REF_CPU), list(brc.STD_CASES)


# ----------------------------------------------------------------------------- the cases themselves
def test_the_rows_are_written_in_place_at_the_block_edges_and_the_twin_differs_nowhere_else():
    for case, kinds in [(brc.rgb_case(k), brc.UNLISTED) for k in RGB] + [(brc.std_case(k), brc.UNLISTED_STD) for k in STD] + \
                       [(brc.sh_case(k)[:3], brc.UNLISTED_SH) for k in SH] + [(brc.sh_case("sh3_std")[:3], brc.UNLISTED_SH_STD)]:
        bad, twin, rows = case
        assert rows == kinds and bad["points"].shape == twin["points"].shape == (N, 3)
        rep = brc.replaced(rows)
        for key in brc.ARRAYS + (("sh",) if "sh" in bad else ()):
            assert bad[key].dtype == np.float32 and bad[key].tobytes() != twin[key].tobytes() or key in ("opacity", "colors")
            assert np.array_equal(bad[key][~rep].view(np.uint32), twin[key][~rep].view(np.uint32)), key
            assert np.isfinite(twin[key]).all(), key
        for key in ("points", "scales", "quaternions"):
            assert np.isfinite(bad[key][~rep]).all(), key
    assert {0, 1, 63, 64, 127, 128, 255, 256, 299} <= set(brc.UNLISTED_SH.values()) | set(brc.DEGENERATE.values())
    assert not set(brc.UNLISTED_SH.values()) & set(brc.DEGENERATE.values())
    bad = brc.rgb_case("base")[0]
    assert not bad["scales"][brc.DEGENERATE["zero_scales"]].any() and (bad["scales"][brc.DEGENERATE["flat_disc"]] == 0).sum() == 1
    one, zero = np.float32(1) / (np.float32(1) + np.exp(np.float32(-80))), np.float32(1) / (np.float32(1) + np.exp(np.float32(80)))
    assert one == np.float32(1) and zero < np.float32(1e-34)
    q = bad["quaternions"]
    assert (np.abs(q[brc.UNLISTED["huge_quat"]]) == np.float32(3e19)).all()
    with np.errstate(over="ignore"):
        assert np.isinf((q[brc.UNLISTED["huge_quat"]] ** 2).sum(dtype=np.float32))
    for kind in ("quat_tiny", "quat_huge"):     # both normalise to finite values in float32
        v = q[brc.DEGENERATE[kind]]
        assert np.isfinite(v / np.sqrt((v * v).sum(dtype=np.float32))).all() and (v * v).sum(dtype=np.float32) > 0
    # the SH rows: behind the camera with a NaN coefficient; the view's float32 camera centre to the bit
    sh_bad = brc.sh_case("sh3")[0]
    cam, im = host_view(sh_bad)
    assert np.array_equal(sh_bad["points"][brc.UNLISTED_SH["at_centre"]], np.asarray(im.camera_center_host, np.float32))
    assert np.isnan(sh_bad["sh"][brc.UNLISTED_SH["nan_coeff"]]).sum() == 1


# ----------------------------------------------------------------------------- the oracles
@pytest.mark.parametrize("kind,name", [("rgb", k) for k in RGB] + [("sh", k) for k in SH])
def test_the_c_oracle_lists_no_unlisted_row_and_every_degenerate_row(kind, name):
    fwd, rows = forward_of(kind, name)
    b, t = fwd["bad"], fwd["twin"]
    for k, i in rows.items():
        assert not b["on"][i], k
        assert not t["on"][i], k
    for k, i in brc.DEGENERATE.items():
        assert b["on"][i] and t["on"][i], k
    assert np.array_equal(b["on"], t["on"])
    # the same frame, finite, from the same number of pairs; at least four visible rows in both (the rows class)
    assert np.isfinite(b["frame"]).all() and np.array_equal(b["frame"].view(np.uint32), t["frame"].view(np.uint32))
    assert b["inst"] == t["inst"] > 0 and b["frame"].max() > 0.1
    nb, nt = np.asarray(b["pre"].order).size, np.asarray(t["pre"].order).size
    visible_unlisted = sorted(k for k, i in rows.items() if i in set(np.asarray(b["pre"].order).tolist()))
    print("%s %s: %d / %d visible (bad / twin), %d listed, %d pairs; visible and unlisted: %s" % (
        kind, name, nb, nt, int(b["on"].sum()), b["inst"], visible_unlisted))
    assert nt >= 4 and nb == nt + len(visible_unlisted)
    # the listed rows' stage 1 is the twin's, bit for bit
    ob, ot = np.asarray(b["pre"].order), np.asarray(t["pre"].order)
    keep_b, keep_t = b["on"][ob], t["on"][ot]
    assert np.array_equal(ob[keep_b], ot[keep_t])
    for field in ("points_xy", "inverse_covariance_2d", "radius", "min_x", "max_x", "min_y", "max_y", "sigmoid_opacity", "depths"):
        a, c = np.asarray(getattr(b["pre"], field))[keep_b], np.asarray(getattr(t["pre"], field))[keep_t]
        assert np.isfinite(a).all() and np.array_equal(a, c), field


@pytest.mark.parametrize("name", STD)
def test_the_std_oracles_list_no_unlisted_row_and_every_degenerate_row(name):
    bad, twin, rows = brc.std_case(name)
    cam, _ = host_view(bad)
    seen = {}
    for tag, sc in (("bad", bad), ("twin", twin)):
        with np.errstate(all="ignore"):
            st = std3dgs_ref.stage1(sc["points"], sc["scales"], sc["quaternions"], sc["opacity"], cam, TILE)
        for k, i in rows.items():
            assert not st.keep[i], (tag, k)
        for k, i in brc.DEGENERATE.items():
            assert st.keep[i], (tag, k)
        # the C port: its pair count is the numpy port's kept rectangles (a stage-1 row of it is NaN only where the depth
        # test culled, so the lists are read off the count and the frame), its frame finite
        img, nvis, inst, port = c_oracle.render_std3dgs(sc["points"], sc["colors"], sc["scales"], sc["quaternions"], sc["opacity"],
                                                        cam, tile=TILE, background=cc.STD_BG, nthreads=4)
        r = st.rect[st.keep]
        assert inst == int(((r[:, 1] - r[:, 0]) * (r[:, 3] - r[:, 2])).sum()) > 0
        assert np.isfinite(img).all() and st.keep.sum() >= 4 and not np.isnan(port[list(brc.DEGENERATE.values()), 0]).any()
        seen[tag] = (st.keep, inst, img)
    assert np.array_equal(seen["bad"][0], seen["twin"][0]) and seen["bad"][1] == seen["twin"][1]
    assert np.array_equal(seen["bad"][2].view(np.uint32), seen["twin"][2].view(np.uint32))
    # the two rows that are UNLISTED under ref_cpu alone: one normalisation makes the zero quaternion of both, the identity
    sc = {k: v.copy() for k, v in bad.items() if isinstance(v, np.ndarray) and v.ndim}
    i = brc.DEGENERATE["quat_huge"]
    sc["quaternions"][i] = 0.0
    with np.errstate(all="ignore"):
        assert std3dgs_ref.stage1(sc["points"], sc["scales"], sc["quaternions"], bad["opacity"], cam, TILE).keep[i]
    sc["quaternions"][i] = np.float32(3e19)
    with np.errstate(all="ignore"):
        assert std3dgs_ref.stage1(sc["points"], sc["scales"], sc["quaternions"], bad["opacity"], cam, TILE).keep[i]


# ----------------------------------------------------------------------------- the restatements
def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("kind,name", [("rgb", k) for k in RGB] + [("sh", k) for k in SH])
def test_the_ref_cpu_restatements_give_zeros_for_unlisted_rows_and_the_twin_s_values_elsewhere(kind, name):
    bad, twin, rep = restated(kind, name)
    for entry in bad:
        for j, (a, b) in enumerate(zip(bad[entry], twin[entry])):
            a, b = np.asarray(a), np.asarray(b)
            if a.dtype.kind not in "fiu":
                continue
            assert np.isfinite(a).all(), (entry, j)
            if a.ndim and a.shape[0] == N and entry != "maps":
                assert not a[rep].any(), (entry, j)
                assert _same(a[~rep], b[~rep]), (entry, j)
            else:
                assert _same(a, b), (entry, j)


@pytest.mark.parametrize("name", STD)
@pytest.mark.parametrize("antialiased", [False, True])
def test_the_std_restatements_give_zeros_for_unlisted_rows_and_the_twin_s_values_elsewhere(name, antialiased):
    built, rows = std_built(name, antialiased)
    rep = brc.replaced(rows)
    b, t = built["bad"], built["twin"]
    assert np.array_equal(b["img"], t["img"]) if not antialiased else True
    assert b["inst"] == t["inst"]
    for which in ("ref", "mirror"):
        for key, a in getattr(b[which], "arrays").items():
            c = t[which].arrays[key]
            assert np.isfinite(a).all() and not a[rep].any() and _same(a[~rep], c[~rep]), (which, key)
    # the gradient mask's standing cap
    wk = b["fwd"].wk if antialiased else b["wk"]
    print("%s%s: %d of %d pixels masked" % (name, " antialiased" if antialiased else "", int((~b["mask"]).sum()), b["mask"].size))
    assert not wk.left_out and (~b["mask"]).sum() <= std_host.MAX_MASKED_SHARE * b["mask"].size


def sh_link(name, tag):
    """(points, active coefficients, active degree, centre, dL/dcolour of the frame's restatement) of an SH case."""
    bad, twin, rows, stored, active = brc.sh_case(name)
    sc = bad if tag == "bad" else twin
    gc = restated("sh", name)[0 if tag == "bad" else 1]["colour"][0]
    k = (active + 1) ** 2
    return sc["points"], np.ascontiguousarray(sc["sh"][:, :k]), active, brc.camera_centre(sc), gc.astype(np.float32)


@pytest.mark.parametrize("name", SH)
def test_the_sh_restatement_applies_the_zero_row_rule(name):
    rows = brc.sh_case(name)[2]
    rep = brc.replaced(rows)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = shr.backward(*sh_link(name, "bad"))
    want = shr.backward(*sh_link(name, "twin"))
    assert not sh_link(name, "bad")[4][rep].any()
    for a, b in zip(got, want):
        assert np.isfinite(a).all() and not a[rep].any() and _same(a[~rep], b[~rep])
    assert (np.abs(got[0]).reshape(N, -1).sum(1) > 0).sum() >= 100 and (np.abs(got[1]).sum(1) > 0).sum() >= 100
    # what the kernels did before the rule: 0 * NaN.  The float32 port of the old statement sequence on the row at the centre
    p, sh, degree, centre, gc = sh_link(name, "bad")
    i = rows["at_centre"]
    with np.errstate(all="ignore"):
        v = p[i] - centre
        d = v * (np.float32(1) / np.sqrt((v * v).sum(dtype=np.float32)))
    assert not v.any() and np.isnan(d).all() and np.isnan(d[0] * np.float32(0))


# ----------------------------------------------------------------------------- conditions on the cases
@pytest.mark.parametrize("name", RGB)
def test_enough_rows_carry_gradient_and_every_degenerate_row_does_under_ref_cpu(name):
    bad, _, rep = restated("rgb", name)
    arrays = dict(colors=bad["colour"][0], opacity=bad["colour"][1], points=bad["geometry"][0], scales=bad["geometry"][1],
                  quaternions=bad["geometry"][2])
    finite = int((~rep).sum())
    for key, a in arrays.items():
        graded = (np.abs(a).reshape(N, -1).sum(1) > 0)
        print("%s: %s: %d of %d finite rows carry gradient" % (name, key, int(graded.sum()), finite))
        assert graded.sum() >= finite // 2, (name, key, int(graded.sum()))
    for kind, i in brc.DEGENERATE.items():
        zero = [k for k, a in arrays.items() if not np.asarray(a)[i].any()]
        print("%s: %s (row %d): zero arrays %s" % (name, kind, i, zero))
        assert set(zero) == set(EXPLAINED_ZEROS_REF_CPU.get(kind, ())), (kind, zero)


# The arrays of a DEGENERATE row that are zero by construction, and why; every other array of every such row carries gradient.
# ref_cpu applies the sigmoid twice (splat/gaussian_scene.py:143 and :164): alpha's factor is sigma(sigma(logit)), 0.73 at
# +80 and 0.5 at -80, so both rows composite and carry gradient in four arrays; the logit's own gradient holds the factor
# s (1 - s) of the inner sigmoid, which is exactly 0 at +80 (s = 1 in float32) -- and 1e-35 at -80, not zero.
# All three scales 0: the covariance is 0, the determinant is floored and the conic is adj(0) / 1e-3 = 0: alpha is the
# opacity factor on the whole box.  "The adjugate alone carries gradient", but cov = T Sigma T^T with Sigma = (R S)(R S)^T is
# quadratic in the scales: dL/dscales = 2 (...) S = 0, dL/dquaternions goes through M = R S = 0, and dL/dpoints has the two
# shares dL/dmean = -1/2 (Q + Q^T)(S1, S2) = 0 (the conic is 0) and dL/dT Sigma^T = 0.  Colour and opacity carry gradient.
EXPLAINED_ZEROS_REF_CPU = {"logit_hi": ("opacity",), "zero_scales": ("points", "scales", "quaternions")}


@pytest.mark.parametrize("name", STD)
def test_enough_rows_carry_gradient_under_std_3dgs(name):
    for antialiased in (False, True):
        built, rows = std_built(name, antialiased)
        ref, rep = built["bad"]["ref"], brc.replaced(rows)
        finite = int((~rep).sum())
        for key in FIVE:
            graded = np.abs(ref.arrays[key]).reshape(N, -1).sum(1) > 0
            assert graded.sum() >= finite // 2, (name, key, int(graded.sum()))
        for kind, i in brc.DEGENERATE.items():
            zero = [k for k in FIVE if not ref.arrays[k][i].any()]
            print("%s%s: %s (row %d): zero arrays %s" % (name, " aa" if antialiased else "", kind, i, zero))
            assert set(zero) == set((EXPLAINED_ZEROS_AA if antialiased else EXPLAINED_ZEROS_STD).get(kind, ())), (kind, zero)


# std_3dgs: one sigmoid.  +80: sigma = 1 exactly, sigma (1 - sigma) = 0.  -80: alpha < 1/255 everywhere, every pair is skipped
# and the row reaches no array.  Zero scales: Sigma is quadratic in the scales as under ref_cpu, but the 0.3 dilation keeps a
# conic, so dL/dpoints lives.  Anti-aliased, the covariance before the dilation has determinant 0: rho is the constant floor
# 0.005 (no gradient), alpha <= 0.005 < 1/255, every pair is skipped and the row reaches no array.
EXPLAINED_ZEROS_STD = {"logit_hi": ("opacity",), "logit_lo": FIVE, "zero_scales": ("scales", "quaternions")}
EXPLAINED_ZEROS_AA = dict(EXPLAINED_ZEROS_STD, zero_scales=FIVE)


# ----------------------------------------------------------------------------- E_REF_BAD
def _hold(entry, worst):
    """`worst`: output -> the authority's error measured here (None: the entry has one output).  Prints every figure, then
    asserts that the recorded ones are these, within E_REF_SLACK either way."""
    off = []
    for key, w in worst.items():
        measured = MEASURED[entry] if key is None else MEASURED[entry][key]
        existing = (_EXISTING[entry] if key is None else _EXISTING[entry][key]) if entry in _EXISTING else TOL
        print("E_REF_BAD: %-9s %-12s authority's error on the twins %.4g (recorded %.4g), existing E_REF %.4g, E_REF_BAD %.4g" % (
            entry, key or "", w, measured, existing, max(measured, existing)))
        if not (w <= measured * E_REF_SLACK and measured <= w * E_REF_SLACK):
            off.append((entry, key, w, measured))
    assert not off, off


def test_the_twin_fixtures_are_the_twins():
    for name, fixture in TWINS.items():
        twin = brc.rgb_case(name)[1]
        gg = load_golden("geomgrad_" + fixture)
        for key in ("points", "scales", "quaternions", "colors"):
            assert np.array_equal(gg[key], twin[key]), key
        assert np.array_equal(gg["opacity"].reshape(-1), twin["opacity"].reshape(-1)) and int(gg["tile"]) == TILE
        assert int(gg["n_culled"]) >= len(brc.UNLISTED) and np.isfinite(gg["grad_quaternions"]).all()
        sizes = {"geomgrad_": 550, "camgrad_": 4, "screengrad_": 16, "absgrad_": 16, "depthgrad_": 200}     # KB: the sibling caps
        for prefix, cap in sizes.items():
            assert os.path.getsize(os.path.join(ROOT, "tests", "golden", prefix + fixture + ".npz")) <= cap * 1024, prefix


def test_e_ref_bad_geometry_colours_and_opacity_are_the_reference_s_own_error_on_the_twins():
    worst = dict.fromkeys(geometry_host.OUTPUTS, 0.0)
    wc = wo = 0.0
    for fixture in TWINS.values():
        gg, base, fwd, out = geometry_host._restate(fixture)
        for k, key in enumerate(geometry_host.OUTPUTS):
            assert np.abs(gg["grad_" + key]).max() > 0
            worst[key] = max(worst[key], gbr.per_gaussian_error(gg["grad_" + key], out[k], out[3 + k]))
        n = gg["points"].shape[0]
        gc, go, sc, so = backward_restatement.backward(conftest_pre(gg), gg["image"], gg["W"], W_, H_, TILE, n, with_scale=True)
        ec, eo = backward_restatement.per_gaussian_error(gg["grad_colors"], gg["grad_opacity"], gc, go, sc, so)
        wc, wo = max(wc, ec), max(wo, eo)
    _hold("geometry", worst)
    _hold("colours", {None: wc})
    _hold("opacity", {None: wo})
    assert MEASURED["colours"] <= TOL and MEASURED["opacity"] <= TOL


def conftest_pre(gg):
    from conftest import golden_preprocessed

    return golden_preprocessed(gg)


def test_e_ref_bad_camera_is_the_reference_s_own_error_on_the_twins():
    worst = dict.fromkeys(("world2view", "full_proj"), 0.0)
    for fixture in TWINS.values():
        cg, gV, gF, aV, aF = camera_host.restated(fixture)
        for key, got, scale in (("world2view", gV, aV), ("full_proj", gF, aF)):
            worst[key] = max(worst[key], cgr.scaled_error(cg["grad_" + key], got, scale))
    _hold("camera", worst)


def test_e_ref_bad_depth_is_the_reference_s_own_error_on_the_twins():
    worst = dict.fromkeys(dr.OUTPUTS, 0.0)
    for fixture in TWINS.values():
        dg, base, fwd = depth_host.depth_fixture(fixture)
        out = depth_host.restate(fixture)
        n = base["points"].shape[0]
        errs = dr.per_output_errors([dg["grad_" + k].reshape(n, -1) for k in dr.OUTPUTS], out[:5], out[5:])
        for key in dr.OUTPUTS:
            worst[key] = max(worst[key], errs[key])
    _hold("depth", worst)


def test_e_ref_bad_screen_and_abs_are_the_reference_s_own_error_on_the_twins():
    ws = wa = 0.0
    for fixture in TWINS.values():
        pre, n, w, h, tile, mom, gn, scale, ref = screen_host.restated(fixture)
        ws = max(ws, gbr.per_gaussian_error(ref, gn, scale))
        got, signed = abs_host.abs_restated(fixture)
        wa = max(wa, gbr.per_gaussian_error(abs_host.reference_abs(fixture), got, scale))
    _hold("screen", {None: ws})
    _hold("abs", {None: wa})


@pytest.mark.parametrize("antialiased", [False, True])
def test_e_ref_bad_std_is_the_mirror_s_own_error_on_the_twins(antialiased):
    entry, keys = ("aa", aar.KEYS) if antialiased else ("std", sbr.ARRAYS)
    worst = dict.fromkeys(keys, 0.0)
    for name in STD:
        case = std_built(name, antialiased)[0]["twin"]
        for key in keys:
            worst[key] = max(worst[key], sbr.per_gaussian_error(case["mirror"].arrays[key], case["ref"].arrays[key], case["ref"].scales[key]))
    _hold(entry, worst)
