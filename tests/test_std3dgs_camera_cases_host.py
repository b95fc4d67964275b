"""The std_3dgs rule set away from fx = fy = 0.75 width and the Treehill / identity pose, host side: the six cases of
camera_cases.STD_CAMERA_CASES (fx / fy = 0.65, 2.33, 0.69, a pose 140 degrees about an oblique axis, a pose with R00, R11 < 0;
two of them with the EWA clamp's gradient branch at limx != limy), the four that are not off axis also anti-aliased.  The
GPU side is tests/test_hip_camera_cases.py.

Nothing here is a new yardstick.  The checks are the ones tests/test_rule_sets_host.py, tests/test_std3dgs_backward_host.py
and tests/test_antialias_host.py apply to their own cases, and the bounds are theirs: the C port's frame within E_REF of the
float64 walk; the hand-derived restatement within AUTOGRAD_TOL of autograd of the independent float64 forward; and the float32
mirror's error against the float64 restatement AT MOST the recorded E_REF / E_REF_AA per array -- which is what lets the GPU
tests hold the kernels to the unchanged BOUND = 12 E_REF and BOUND_AA = 12 E_REF_AA.  The cases live in tables of their own
(CAMERA_CASES, CAMERA_CASES_AA): the E_REF measurements of the sibling files do not see them.  If a change of the table
pushes a ratio above 1, pick another seed; E_REF stays.

Measured here (CPU), in the table's order aniso, aniso_tall, farpose, roll, offaxis_aniso_tall, offaxis_roll:
  C port's frame, worst decided pixel / E_REF: 0.47 0.38 0.31 0.38 0.43 0.59; no ambiguous pixel, nothing left out, no pixel
  masked out of dL/dframe in any of the ten case / variant pairs.
  restatement vs autograd: at most 1.7e-16 of the scale on every array of every case (bound 1e-9).
  mirror's error / E_REF, worst over the six (std):   colors 0.13 opacity 0.81 moments 0.69 points 0.26 scales 0.27
                                                      quaternions 0.44 means2d 0.73
  mirror's error / E_REF_AA, worst over the four:     colors 0.16 opacity 0.37 points 0.20 scales < 0.01 quaternions 0.09
                                                      means2d 0.51
  Gaussians with a colour gradient per case: 58 .. 109; EWA-clamped ones that carry gradient: 14 (offaxis_aniso_tall) and
  39 (offaxis_roll), some clamped in x alone and some in y alone in both; nearest rho ratio to its floor: 8.1e3 x.

Teeth (test_a_swapped_focal_length_or_clamp_limit_leaves_the_bound...): the float32 mirror's chain handed fx <-> fy,
tan_fovx <-> tan_fovy inside the focal lengths, or limx <-> limy leaves BOUND by the factors that test prints, on an
anisotropic case; on random_64x64_n800_t2 (fx = fy, square frame) each of the three changes no bit of any gradient.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import antialias_restatement as aar  # noqa: E402
import camera_cases as cc  # noqa: E402
import rule_set_restatement as rsr  # noqa: E402
import std3dgs_backward_restatement as sbr  # noqa: E402
import test_antialias_host as aa_host  # noqa: E402
import test_rule_sets_host as rules_host  # noqa: E402
import test_std3dgs_backward_host as std_host  # noqa: E402
from oracle import std3dgs_ref  # noqa: E402

f32 = np.float32


def _factory(name):
    camera, n, seed, kw = cc.STD_CAMERA_CASES[name]
    return lambda: cc.scene(camera, n, seed, **kw)


# name -> (scene factory, tile, background), the shape of STD_CASES' entries
CAMERA_CASES = {name: (_factory(name), cc.TILE, cc.STD_BG) for name in cc.STD_CAMERA_CASES}
CAMERA_CASES_AA = {name: CAMERA_CASES[name] for name in CAMERA_CASES if name not in cc.STD_OFFAXIS}
ANISOTROPIC = [name for name, entry in cc.STD_CAMERA_CASES.items() if entry[0] in cc.ANISOTROPIC]
SQUARE_CASE = "random_64x64_n800_t2"        # of STD_CASES: fx = fy = 48 on 64 x 64


@functools.lru_cache(maxsize=None)
def backward_case(name):
    """test_std3dgs_backward_host.backward_case's dict of a case of CAMERA_CASES."""
    make, tile, bg = CAMERA_CASES[name]
    return std_host.build_backward(std_host.build_tuple(make(), tile, bg))


@functools.lru_cache(maxsize=None)
def backward_case_aa(name):
    """test_antialias_host.backward_case's dict of a case of CAMERA_CASES_AA."""
    make, tile, bg = CAMERA_CASES_AA[name]
    return aa_host.build_backward(aa_host.build_case(make(), tile, bg))


# ----------------------------------------------------------------------------- the table

def test_the_table_is_the_issue_s_and_stays_out_of_the_sibling_tables():
    assert list(cc.STD_CAMERA_CASES) == ["std_aniso_64x48_n120", "std_aniso_tall_48x64_n100", "std_farpose_64x48_n120",
                                         "std_roll_64x48_n100", "std_offaxis_aniso_tall_48x64_n100",
                                         "std_offaxis_roll_64x48_n100"]
    assert cc.STD_BG == rules_host.STD_BG and cc.TILE == 16
    assert len(CAMERA_CASES_AA) == 4 and set(cc.STD_OFFAXIS) == set(CAMERA_CASES) - set(CAMERA_CASES_AA)
    for name in CAMERA_CASES:
        assert name not in rules_host.STD_CASES and name not in std_host.CASES and name not in aa_host.CASES
    for name, (camera, n, seed, kw) in cc.STD_CAMERA_CASES.items():
        c = cc.CAMERAS[camera]
        assert name.endswith("%dx%d_n%d" % (c["width"], c["height"], n)) and c["width"] * c["height"] == 3072
        sc = CAMERA_CASES[name][0]()
        assert sc["points"].shape == (n, 3) and (float(sc["fx"]), float(sc["fy"])) == (c["fx"], c["fy"])
    # every camera of the set is under the rule set, and the clamp's cases sit at cameras with fx != fy
    assert {e[0] for e in cc.STD_CAMERA_CASES.values()} == set(cc.NAMES)
    assert all(cc.STD_CAMERA_CASES[k][0] in cc.ANISOTROPIC for k in cc.STD_OFFAXIS)
    # the square case the swaps must not touch
    sc = rules_host.std_case(SQUARE_CASE)[0]
    assert float(sc["fx"]) == float(sc["fy"]) and int(sc["width"]) == int(sc["height"])


# ----------------------------------------------------------------------------- the forward

@pytest.mark.parametrize("name", list(CAMERA_CASES))
def test_the_c_port_and_the_numpy_port_match_the_float64_walk(name):
    case = backward_case(name)
    sc, wk, bound = case["sc"], case["wk"], rules_host.E_REF["std_3dgs"] * rules_host.E_REF_SLACK
    v = rsr.classify(wk, case["img"], bound)
    print("%s: C port: worst decided pixel / E_REF %.2f, %d ambiguous, %d left out; %d of %d visible, %d instances" % (
        name, v.worst_decided / rules_host.E_REF["std_3dgs"], v.n_ambiguous, v.n_left_out, case["nvis"], case["n"], case["inst"]))
    assert v.n_left_out == 0 and not wk.left_out and not v.unexplained, (name, v.unexplained[:5])
    assert wk.ambiguous.sum() <= rules_host.MAX_AMBIGUOUS_SHARE * wk.ambiguous.size
    img, nvis, inst = std3dgs_ref.render(sc["points"], case["colors"], sc["scales"], sc["quaternions"], sc["opacity"], case["cam"],
                                         tile=case["tile"], background=case["bg"])
    assert (nvis, inst) == (case["nvis"], case["inst"])
    vn = rsr.classify(wk, img, bound)
    assert vn.n_left_out == 0 and not vn.unexplained, (name, vn.unexplained[:5])


# ----------------------------------------------------------------------------- the backward

@pytest.mark.parametrize("name", list(CAMERA_CASES))
def test_the_restatement_agrees_with_autograd_of_an_independent_forward(name):
    std_host.agrees_with_autograd(name, backward_case(name))


@pytest.mark.parametrize("name", list(CAMERA_CASES_AA))
def test_the_antialiased_restatement_agrees_with_autograd_of_an_independent_forward(name):
    aa_host.agrees_with_autograd(name, backward_case_aa(name))


def _mirror_ratios(cases, keys, e_ref):
    worst = {k: (0.0, None) for k in keys}
    for name, case in cases:
        ref, mir = case["ref"], case["mirror"]
        line = {}
        for key in keys:
            scale = ref.scales[key]
            scale2 = scale if scale.ndim == 2 else scale[:, None]
            assert (np.abs(ref.arrays[key]) <= scale2 * (1 + 1e-9) + 1e-300).all(), (name, key)
            assert np.isfinite(mir.arrays[key]).all() and np.isfinite(ref.arrays[key]).all(), (name, key)
            line[key] = sbr.per_gaussian_error(mir.arrays[key], ref.arrays[key], scale) / e_ref[key]
            worst[key] = max(worst[key], (line[key], name))
        print("  %-36s %s" % (name, "  ".join("%s %.3f" % (k, line[k]) for k in keys)))
    for key, (ratio, where) in worst.items():
        print("mirror's error / recorded E_REF: %s %.3f at %s" % (key, ratio, where))
    return worst


def test_the_mirrors_error_stays_within_the_recorded_e_ref():
    """What entitles the GPU tests to BOUND = 12 E_REF at these cameras: the float32 mirror is no worse here than on the
    cases E_REF was measured on."""
    worst = _mirror_ratios([(name, backward_case(name)) for name in CAMERA_CASES], sbr.ARRAYS, std_host.E_REF)
    for key, (ratio, where) in worst.items():
        assert 0 < ratio <= 1.0, (key, ratio, where)


def test_the_antialiased_mirrors_error_stays_within_the_recorded_e_ref_aa():
    worst = _mirror_ratios([(name, backward_case_aa(name)) for name in CAMERA_CASES_AA], aar.KEYS, aa_host.E_REF_AA)
    for key, (ratio, where) in worst.items():
        assert 0 < ratio <= 1.0, (key, ratio, where)


@pytest.mark.parametrize("name", list(CAMERA_CASES) + [name + "/antialiased" for name in CAMERA_CASES_AA])
def test_the_gradient_mask_leaves_out_at_most_one_percent(name):
    case = backward_case_aa(name.split("/")[0]) if name.endswith("/antialiased") else backward_case(name)
    wk, mask = (case["fwd"].wk if "fwd" in case else case["wk"]), case["mask"]
    print("%s: %d of %d pixels masked" % (name, int((~mask).sum()), mask.size))
    assert not wk.left_out, wk.left_out
    assert (~mask).sum() <= std_host.MAX_MASKED_SHARE * mask.size, (name, int((~mask).sum()))
    assert (case["g"][~mask] == 0).all() and np.abs(case["g"][mask]).min() > 0


# ----------------------------------------------------------------------------- what the cases are for

def clamp_axes(case):
    """(clamped in x alone, clamped in y alone) per row, for the rows that carry a geometry gradient: |tx / tz| and
    |ty / tz| of the float64 stage 1 against 1.3 tan_fov."""
    sc = case["sc"]
    with np.errstate(all="ignore"):
        st = sbr.stage1_std(sc["points"], sc["scales"], sc["quaternions"], case["cam"], np.float64)
    live = case["ref"].scales["points"] > 0
    assert np.array_equal(case["ref"].clamped_ewa[live], ~(st["inx"] & st["iny"])[live])
    return live & ~st["inx"] & st["iny"], live & st["inx"] & ~st["iny"]


@pytest.mark.parametrize("name", list(CAMERA_CASES))
def test_every_case_holds_what_it_is_for(name):
    case = backward_case(name)
    ref, culled = case["ref"], np.isnan(case["rows"][:, 0])
    graded = int((ref.scales["colors"] > 0).sum())
    ewa = int((ref.clamped_ewa & (ref.scales["points"] > 0)).sum())
    only_x, only_y = clamp_axes(case)
    print("%s: %d culled rows, %d Gaussians with a colour gradient, %d EWA-clamped with gradient (%d in x alone, %d in y alone)"
          % (name, int(culled.sum()), graded, ewa, int(only_x.sum()), int(only_y.sum())))
    # rows with an exactly zero gradient: culled by stage 1 in the four cases with points behind the camera; in the two
    # off-axis ones (every row passes stage 1: their table entries put nothing behind the camera) the rows that reach no pixel
    dead = ref.scales["colors"] == 0
    assert graded >= 50 and dead.any() and dead[culled].all() and (culled.any() or name in cc.STD_OFFAXIS)
    for key in sbr.ARRAYS:
        assert not ref.arrays[key][dead].any() and not case["mirror"].arrays[key][dead].any(), key
    assert np.abs(ref.arrays["points"]).max() > 0 and np.abs(ref.arrays["quaternions"]).max() > 0
    if name in cc.STD_OFFAXIS:
        assert ewa >= 10 and only_x.any() and only_y.any()
        assert f32(case["cam"].tan_fovx) != f32(case["cam"].tan_fovy)


@pytest.mark.parametrize("name", list(CAMERA_CASES_AA))
def test_the_antialiased_cases_keep_the_mirrors_conditions(name):
    case = backward_case_aa(name)
    aa_host.covariance_is_the_c_ports(case)
    nearest = aa_host.no_gaussian_lies_on_the_clamp(name, case)
    assert nearest > 10.0           # nowhere near the floor: the rho term runs on every row
    assert not case["fwd"].fac32.clamped[~np.isnan(case["rows0"][:, 0])].any()
    ref = case["ref"]
    culled = np.isnan(case["rows0"][:, 0])
    assert culled.any() and (ref.scales["colors"] > 0).sum() >= 50
    for key in aar.KEYS:
        assert not ref.arrays[key][culled].any(), key


# ----------------------------------------------------------------------------- teeth

def _swaps(cam):
    """name -> stage1_std keywords: the float32 values a kernel with that slip would form."""
    tx, ty = f32(cam.tan_fovx), f32(cam.tan_fovy)
    W, H = f32(int(cam.width)), f32(int(cam.height))
    fx, fy = W / (f32(2.0) * tx), H / (f32(2.0) * ty)
    return {"fx <-> fy": dict(focal=(fy, fx)),
            "tan_fovx <-> tan_fovy in the focal lengths": dict(focal=(W / (f32(2.0) * ty), H / (f32(2.0) * tx))),
            "limx <-> limy": dict(limits=(f32(1.3) * ty, f32(1.3) * tx))}


def _mirror_with(case, **kw):
    sc, R = case["sc"], case["R"]
    rows = np.asarray(R.index, np.int64)
    st = sbr.stage1_std(sc["points"][rows], sc["scales"][rows], sc["quaternions"][rows], case["cam"], np.float32, **kw)
    return sbr.backward(R, case["dec"], sc["points"], sc["scales"], sc["quaternions"], case["cam"], case["g"], case["bg"],
                        dtype=np.float32, stage1=st)


GEOMETRY = ("points", "scales", "quaternions", "means2d")


def test_a_swapped_focal_length_or_clamp_limit_leaves_the_bound_here_and_changes_no_bit_at_fx_equal_fy():
    """Why these cases exist, in code.  The float32 mirror's chain with each slip a kernel could hold: outside BOUND on an
    anisotropic case (what a kernel with the slip would show on the GPU), bit-equal on a square frame with fx = fy (what
    every case before these showed)."""
    square = std_host.backward_case(SQUARE_CASE)
    assert f32(square["cam"].tan_fovx) == f32(square["cam"].tan_fovy)
    # the seam is exact: handed the camera's own values the mirror keeps its bits
    own = _mirror_with(square)
    for key in GEOMETRY:
        assert np.array_equal(own.arrays[key], square["mirror"].arrays[key]), key
    caught = {}
    for swap in _swaps(square["cam"]):
        got = _mirror_with(square, **_swaps(square["cam"])[swap])
        for key in GEOMETRY:
            assert np.array_equal(got.arrays[key], square["mirror"].arrays[key]), (swap, key)
        caught[swap] = {}
        for name in ANISOTROPIC:
            case = backward_case(name)
            ref = case["ref"]
            got = _mirror_with(case, **_swaps(case["cam"])[swap])
            factor = {k: sbr.per_gaussian_error(got.arrays[k], ref.arrays[k], ref.scales[k]) / std_host.BOUND[k] for k in GEOMETRY}
            caught[swap][name] = max(factor.values())
            print("%-42s %-36s error / BOUND: %s" % (swap, name, "  ".join("%s %.3g" % (k, factor[k]) for k in GEOMETRY)))
    for swap, by_case in caught.items():
        assert max(by_case.values()) > 1.0, (swap, by_case)
    # the two focal-length slips show on every anisotropic case, the clamp's on the off-axis ones (the clamp must bite)
    for swap in ("fx <-> fy", "tan_fovx <-> tan_fovy in the focal lengths"):
        assert all(v > 1.0 for v in caught[swap].values()), (swap, caught[swap])
    assert all(caught["limx <-> limy"][name] > 1.0 for name in cc.STD_OFFAXIS), caught["limx <-> limy"]
