"""The float32 ports of the two discontinuous rule sets held to the float64 restatement (tests/rule_set_restatement.py),
pixel by pixel, on the CPU: orc_render_std3dgs and std3dgs_ref.render for GSX_SEM_STD_3DGS, orc_render_cuda_semantics for
GSX_SEM_REF_CUDA.  Every decided pixel lies within E_REF of the float64 colour, every ambiguous pixel within E_REF of one
of its alternatives, nothing is left out.

E_REF is MEASURED HERE: the largest error of the float32 C port on decided pixels against the float64 colour, per rule
set, over every case below.  The recorded figures are asserted as an upper bound of what is measured (with the last printed
digit as slack) and the kernels are held to BOUND = 12 E_REF (tests/test_hip_rule_sets.py), the project's multiple.

The cases are the ones the GPU tests render, and the conditions that make them worth rendering are asserted here, from the
restatement alone: few ambiguous pixels, none left out, the knife edge of two clamped alphas decided, single-pixel block
uses, stops on both sides of a batch seam, a block that dies inside a living tile, skip decisions close to 1/255.
"""
import functools

import numpy as np
import pytest

from conftest import golden_preprocessed, load_golden
from intro_to_gaussian_splatting_amd import synthetic
from oracle import c_oracle, cpu_ref, std3dgs_ref
import rule_set_restatement as rsr

NTHREADS = 8
E_REF = {"std_3dgs": 4.489e-7, "ref_cuda": 2.917e-7}      # measured by test_e_ref_is_the_ports_own_error
BOUND = {k: 12 * v for k, v in E_REF.items()}
E_REF_SLACK = 1.001
MAX_AMBIGUOUS_SHARE = 1e-3

f32 = np.float32


# ----------------------------------------------------------------------------- std_3dgs scenes

def _camera_dict(w, h, fx, fy):
    return dict(qvec=np.array([1.0, 0, 0, 0]), tvec=np.zeros(3), fx=np.float64(fx), fy=np.float64(fy),
                cx=np.float64(w / 2), cy=np.float64(h / 2), width=np.int64(w), height=np.int64(h))


def stack_scene(n, logit_value, colors_0_255, z0=2.0):
    """The coincident stack of tests/test_std3dgs_oracle.py::_stack as a scene dict: 16x16 frame, footprints far larger
    than the frame."""
    pts = np.tile(np.array([[0.0, 0.0, z0]], f32), (n, 1))
    pts[:, 2] += np.arange(n, dtype=f32) * f32(0.01)
    sc = dict(points=pts, colors_0_255=np.asarray(colors_0_255, f32), scales=np.full((n, 3), 2.0, f32),
              quaternions=np.tile(np.array([[1.0, 0, 0, 0]], f32), (n, 1)), opacity=np.full((n, 1), logit_value, f32))
    sc.update(_camera_dict(16, 16, 8.0, 8.0))
    return sc


def _opaque_stack():
    colors = np.tile(np.array([[40.0, 80.0, 200.0]], f32), (10, 1))
    colors[0], colors[1] = (256.0, 0.0, 0.0), (0.0, 256.0, 0.0)
    return stack_scene(10, 20.0, colors)


def _half_stack():
    return stack_scene(20, 0.0, np.full((20, 3), 256.0, f32))


def dense_scene():
    """Opaque and large: most pixels saturate, tile lists run past two 64-record batches."""
    sc = synthetic.make_scene(2600, 96, 96, seed=11, sigma_scale=2.0)
    sc["opacity"] = (sc["opacity"] + f32(3.0)).astype(f32)
    return sc


RING_W, RING_H, RING_R2 = 40, 24, 25


def ring_scene():
    """One isotropic Gaussian per 8x8 cell of a 40x24 frame (partial edge tiles on both axes at tile 16), centred on a
    pixel, its opacity chosen so that alpha at the twelve pixels at squared distance 25 is 1/255 (1 +- 5e-4): the
    alpha = 1/255 contour passes between pixel centres, alternately just outside and just inside that ring of pixels.
    A long focal length keeps the footprints isotropic to 1e-6 off axis."""
    w, h, fx = RING_W, RING_H, 20000.0
    cxs, cys = np.arange(4, w, 8), np.arange(4, h, 8)
    gx, gy = [a.reshape(-1) for a in np.meshgrid(cxs, cys, indexing="ij")]
    n = gx.size
    z = 4.0 + 0.125 * np.arange(n)                               # distinct depths: the order is by depth
    # pixel = ((ndc + 1) W - 1) / 2 with ndc = x fx / (z W / 2)  ->  x = (pixel + 0.5 - W/2) z / fx
    pts = np.stack([(gx + 0.5 - w / 2) * z / fx, (gy + 0.5 - h / 2) * z / fx, z], axis=1).astype(f32)
    sigma_px = np.sqrt(2.3)                                      # + 0.3 dilation: 25 / (2 * 2.6) = 4.8 = ln(255 * 0.476)
    sc = dict(points=pts, colors_0_255=np.tile(np.array([[250.0, 120.0, 30.0]], f32), (n, 1)),
              scales=np.tile((sigma_px * z / fx)[:, None], (1, 3)).astype(f32),
              quaternions=np.tile(np.array([[1.0, 0, 0, 0]], f32), (n, 1)), opacity=np.zeros((n, 1), f32))
    sc.update(_camera_dict(w, h, fx, fx))
    cam = cpu_ref.build_camera(sc["qvec"], sc["tvec"], sc["fx"], sc["fy"], w, h)
    st = std3dgs_ref.stage1(sc["points"], sc["scales"], sc["quaternions"], sc["opacity"], cam, 16)
    ring = [(dx, dy) for dx in range(-5, 6) for dy in range(-5, 6) if dx * dx + dy * dy == RING_R2]
    logit = np.zeros((n, 1), f32)
    for i in range(n):
        A, B, C = st.conic[i].astype(np.float64)
        x, y = st.xy[i].astype(np.float64)
        g = []
        for dx, dy in ring:
            ex, ey = x - (gx[i] + dx), y - (gy[i] + dy)
            g.append(np.exp(-0.5 * (A * ex * ex + C * ey * ey) - B * ex * ey))
        g = np.array(g)
        assert g.max() / g.min() - 1.0 < 2e-4, (i, g)              # the ring of pixels is one alpha level
        op = rsr.STD_3DGS.skip_threshold * (1.0 + (5e-4 if i % 2 else -5e-4)) / g.mean()
        logit[i, 0] = np.log(op / (1.0 - op))
    sc["opacity"] = logit
    return sc


STD_BG = (0.25, 0.5, 0.75)
# name -> (scene factory, tile, background)
STD_CASES = {
    "random_256x256_n2000_t16": (lambda: synthetic.make_scene(2000, 256, 256, seed=0), 16, STD_BG),
    "random_130x70_n1500_t8": (lambda: synthetic.make_scene(1500, 130, 70, seed=2, behind_fraction=0.1), 8, STD_BG),
    "random_96x80_n1000_t32": (lambda: synthetic.make_scene(1000, 96, 80, seed=3), 32, STD_BG),
    "random_64x64_n800_t2": (lambda: synthetic.make_scene(800, 64, 64, seed=4), 2, STD_BG),
    "stack_opaque_16x16": (_opaque_stack, 16, (0.2, 0.3, 1.0)),
    "stack_half_16x16": (_half_stack, 16, (0.0, 0.0, 0.0)),
    "dense_96x96": (dense_scene, 16, STD_BG),
    "ring_40x24": (ring_scene, 16, (0.1, 0.6, 0.3)),
}
RANDOM_CASES = [k for k in STD_CASES if k.startswith("random")]


def std_reference(sc, cam, colors, tile, background):
    """(C port's frame, n_visible, instances, records, walk) of one std_3dgs frame."""
    img, nvis, inst, rows = c_oracle.render_std3dgs(sc["points"], colors, sc["scales"], sc["quaternions"], sc["opacity"],
                                                    cam, tile=tile, background=background, nthreads=NTHREADS)
    R = rsr.records_std3dgs(rows, colors, int(cam.width), int(cam.height), tile)
    return img, nvis, inst, R, rsr.walk(rsr.STD_3DGS, R, int(cam.width), int(cam.height), background)


@functools.lru_cache(maxsize=None)
def std_case(name):
    """(scene dict, tile, background, camera, colours, C port's frame, n_visible, instances, records, walk); computed once."""
    make, tile, bg = STD_CASES[name]
    sc = make()
    w, h = int(sc["width"]), int(sc["height"])
    cam = cpu_ref.build_camera(sc["qvec"], sc["tvec"], sc["fx"], sc["fy"], w, h)
    colors = (sc["colors_0_255"] / f32(256.0)).astype(f32)
    return (sc, tile, bg, cam, colors) + std_reference(sc, cam, colors, tile, bg)


# ----------------------------------------------------------------------------- ref_cuda scenes

CUDA_FIXTURES = ["small_64x48_n300", "cull_96x80_n400", "c1_256x256_n2000"]
CUDA_STACK_W, CUDA_STACK_H = 40, 24


def cuda_stack_pre():
    """Preprocessed arrays (the stage-2 entry's input) of 12 wide, mostly opaque Gaussians over a 40x24 frame, in order:
    T falls below 0.001 under most of the frame.  Bounding boxes end inside the frame on every side."""
    rs = np.random.RandomState(5)
    n, w, h = 12, CUDA_STACK_W, CUDA_STACK_H
    mean = np.stack([rs.uniform(8, w - 8, n), rs.uniform(6, h - 6, n)], axis=1).astype(f32)
    var = rs.uniform(150.0, 400.0, (n, 2))
    cov = np.zeros((n, 2, 2), f32)
    cov[:, 0, 0], cov[:, 1, 1] = var[:, 0], var[:, 1]
    cov[:, 0, 1] = cov[:, 1, 0] = (rs.uniform(-0.5, 0.5, n) * np.sqrt(var[:, 0] * var[:, 1])).astype(f32)
    inv = np.linalg.inv(cov.astype(np.float64)).astype(f32)
    half = rs.uniform(14.0, 30.0, (n, 2)).astype(f32)
    op = rs.uniform(0.55, 1.0, (n, 1)).astype(f32)
    op[::4] = f32(0.999)                                          # clamped alphas at their centres
    colors = rs.uniform(0.0, 1.0, (n, 3)).astype(f32)
    return cpu_ref.Preprocessed(mean, colors, cov, np.arange(n, dtype=f32) + f32(1.0), inv, half.max(axis=1), mean,
                                mean[:, 0] - half[:, 0], mean[:, 1] - half[:, 1], mean[:, 0] + half[:, 0],
                                mean[:, 1] + half[:, 1], op, np.arange(n))


CUDA_CASES = CUDA_FIXTURES + ["stack_40x24"]


@functools.lru_cache(maxsize=None)
def cuda_case(name):
    """(preprocessed arrays, width, height, C port's frame (H,W,3), records, walk); computed once."""
    if name == "stack_40x24":
        pre, w, h = cuda_stack_pre(), CUDA_STACK_W, CUDA_STACK_H
    else:
        g = load_golden(name)
        pre, w, h = golden_preprocessed(g), int(g["width"]), int(g["height"])
    img = c_oracle.render_cuda_semantics(pre, w, h, nthreads=NTHREADS)
    R = rsr.records_ref_cuda(pre, w, h)
    return pre, w, h, img, R, rsr.walk(rsr.REF_CUDA, R, w, h)


# ----------------------------------------------------------------------------- the ports against the restatement

def _report(tag, wk, v):
    print("%s: decided pixels within %.4g, ambiguous %d (%.4g from an alternative, at most %d decisions a pixel), "
          "left out %d" % (tag, v.worst_decided, v.n_ambiguous, v.worst_ambiguous, wk.max_ambiguous, v.n_left_out))


def _conditions(tag, wk):
    assert not wk.left_out, (tag, wk.left_out)
    assert wk.ambiguous.sum() <= MAX_AMBIGUOUS_SHARE * wk.ambiguous.size, (tag, int(wk.ambiguous.sum()))


def test_e_ref_is_the_ports_own_error():
    """E_REF per rule set = the C port's largest error on a decided pixel over all cases; every ambiguous pixel of the
    port matches an alternative to E_REF; nothing is left out."""
    worst = {"std_3dgs": (0.0, None), "ref_cuda": (0.0, None)}
    for name in STD_CASES:
        img, wk = std_case(name)[5], std_case(name)[9]
        v = rsr.classify(wk, img, E_REF["std_3dgs"] * E_REF_SLACK)
        _report("std_3dgs " + name, wk, v)
        _conditions(name, wk)
        assert not v.unexplained, (name, v.unexplained[:5])
        worst["std_3dgs"] = max(worst["std_3dgs"], (v.worst_decided, name))
    for name in CUDA_CASES:
        img, wk = cuda_case(name)[3], cuda_case(name)[5]
        v = rsr.classify(wk, img, E_REF["ref_cuda"] * E_REF_SLACK)
        _report("ref_cuda " + name, wk, v)
        _conditions(name, wk)
        assert not v.unexplained, (name, v.unexplained[:5])
        worst["ref_cuda"] = max(worst["ref_cuda"], (v.worst_decided, name))
    for key, (val, where) in worst.items():
        print("E_REF %s = %.4g at %s (recorded %.4g, kernels held to %.4g)" % (key, val, where, E_REF[key], BOUND[key]))
        assert E_REF[key] / 1.5 <= val <= E_REF[key] * E_REF_SLACK, (key, val)


@pytest.mark.parametrize("name", list(STD_CASES))
def test_numpy_port_matches_the_restatement(name):
    """oracle/std3dgs_ref.render (numpy float32, numpy's exp) is held to the same restatement."""
    sc, tile, bg, cam, colors, _, nvis, inst, _, wk = std_case(name)
    img, nvis_n, inst_n = std3dgs_ref.render(sc["points"], colors, sc["scales"], sc["quaternions"], sc["opacity"], cam,
                                             tile=tile, background=bg)
    assert (nvis_n, inst_n) == (nvis, inst)
    v = rsr.classify(wk, img, E_REF["std_3dgs"] * E_REF_SLACK)
    _report("numpy port " + name, wk, v)
    assert not v.unexplained, (name, v.unexplained[:5])


# ----------------------------------------------------------------------------- what the scenes must reach

@pytest.mark.parametrize("name", RANDOM_CASES)
def test_random_scenes_use_records_at_single_pixels_of_a_block(name):
    wk = std_case(name)[9]
    print("%s: %d (record, 8x8 block) combinations use the record at exactly one pixel" % (name, wk.single_pixel_blocks))
    assert wk.single_pixel_blocks >= 50


def test_knife_edge_of_two_clamped_alphas_is_decided_and_stops_after_one():
    """T = 1 - 0.99f exactly, then T (1 - 0.99f) = 9.99998e-5 against 9.9999997e-5: every float32 order stops, so the
    decision is decided although it sits 1.7e-6 (relative) from the threshold."""
    sc, tile, bg, cam, colors, img, _, _, R, wk = std_case("stack_opaque_16x16")
    test = (1.0 - rsr.CLAMP) ** 2
    assert 0 < 1.0 - test / rsr.STD_3DGS.stop_threshold < 2e-6
    for y, x in ((7, 7), (7, 8), (8, 7), (8, 8)):                  # both alphas clamp here: exp(power) > 0.99
        assert wk.n_ambiguous[y, x] == 0 and wk.stopped[y, x] and wk.composited[y, x] == 1 and wk.stop_position[y, x] == 1
        expect = rsr.CLAMP * colors[0].astype(np.float64) + (1.0 - rsr.CLAMP) * np.asarray(bg)
        np.testing.assert_allclose(wk.colour[y, x], expect, rtol=0, atol=1e-12)
    assert colors[1:].any(axis=1).all() and any(bg)                # coloured Gaussians behind, a coloured background
    assert not wk.ambiguous.any() and wk.stopped[6:10].all() and not wk.stopped[0, 0]   # the corners never saturate


def test_half_opaque_stack_composites_thirteen_and_stops():
    wk = std_case("stack_half_16x16")[9]
    assert wk.composited[8, 8] == 13 and wk.stopped[8, 8] and wk.stop_position[8, 8] == 13
    assert wk.n_ambiguous[8, 8] == 0


def test_dense_scene_reaches_the_stop_rule_the_batch_seam_and_a_dying_block():
    sc, tile, bg, cam, colors, img, _, _, R, wk = std_case("dense_96x96")
    assert tile == 16 and max(int(sc["width"]), int(sc["height"])) <= 96
    share = wk.stopped.mean()
    longest = int(wk.list_length.max())
    early, late = int((wk.stopped & (wk.stop_position < 64)).sum()), int((wk.stopped & (wk.stop_position >= 64)).sum())
    # a block dies at the end of the 64-record batch in which its last pixel stops; others of its tile go on
    h, w = wk.stopped.shape
    dying = 0
    for ty in range(0, h, 16):
        for tx in range(0, w, 16):
            batches = (int(wk.list_length[ty, tx]) + 63) // 64
            last = []
            for by in (0, 8):
                for bx in (0, 8):
                    s = (slice(ty + by, ty + by + 8), slice(tx + bx, tx + bx + 8))
                    last.append(int(wk.stop_position[s].max()) // 64 if wk.stopped[s].all() else batches)
            dying += sum(1 for b in last if b + 1 < batches and max(last) > b)
    print("dense: %.1f %% of the pixels stop, longest list %d, stops before / after the first seam %d / %d, %d blocks die "
          "inside a living tile" % (100 * share, longest, early, late, dying))
    assert share >= 0.25 and longest > 128 and early > 0 and late > 0 and dying > 0


def test_ring_puts_decided_skip_decisions_next_to_the_threshold():
    sc, tile, bg, cam, colors, img, _, _, R, wk = std_case("ring_40x24")
    assert int(sc["width"]) % 16 and int(sc["height"]) % 16        # partial edge tiles on both axes
    print("ring: %d decided skip decisions within %g of 1/255 below it, %d above" % (
        wk.near_skip_below, rsr.NEAR, wk.near_skip_above))
    assert wk.near_skip_below + wk.near_skip_above >= 100 and wk.near_skip_below >= 30 and wk.near_skip_above >= 30


def test_cuda_stack_breaks_under_a_quarter_of_the_frame():
    wk = cuda_case("stack_40x24")[5]
    print("ref_cuda stack: %.1f %% of the pixels break" % (100 * wk.stopped.mean()))
    assert wk.stopped.mean() >= 0.25


# ----------------------------------------------------------------------------- the classifier itself

def test_an_ambiguous_decision_yields_both_colours():
    """One record whose alpha is 1/255 to a rounding at one pixel: ambiguous there, alternatives = with and without it."""
    thr = rsr.STD_3DGS.skip_threshold
    R = rsr.Records(np.array([3.0]), np.array([2.0]), np.array([0.5]), np.array([0.0]), np.array([0.5]),
                    np.array([thr * (1 + 1e-8)]), np.array([[1.0, 0.5, 0.25]]), np.array([[0, 8, 0, 8]]), np.array([0]))
    wk = rsr.walk(rsr.STD_3DGS, R, 8, 8, (0.0, 0.0, 1.0))
    assert wk.ambiguous.sum() == 1 and wk.ambiguous[2, 3] and not wk.left_out
    alts = wk.alternatives[(2, 3)]
    assert alts.shape == (2, 3)
    np.testing.assert_allclose(alts[0], wk.colour[2, 3])
    np.testing.assert_allclose(alts[1], [0.0, 0.0, 1.0])
    good = wk.colour.copy()
    assert not rsr.classify(wk, good, 1e-9).unexplained
    good[2, 3] = (0.0, 0.0, 1.0)
    assert not rsr.classify(wk, good, 1e-9).unexplained
    good[2, 4] += 1e-6                                             # a decided pixel gets no such allowance
    assert rsr.classify(wk, good, 1e-9).unexplained == [(2, 4, pytest.approx(1e-6, rel=1e-3))]
    good[2, 4] -= 1e-6
    good[2, 3] = (0.0, 0.0, 1.0 - 1e-6)                            # nor does an ambiguous one away from its alternatives
    assert rsr.classify(wk, good, 1e-9).unexplained == [(2, 3, pytest.approx(1e-6, rel=1e-3))]
    # the count-based tests' question: two frames that differ by more than their bar somewhere
    a, b = wk.colour.copy(), wk.colour.copy()
    b[2, 3] = (0.0, 0.0, 1.0)                                      # one side skipped the record: explained
    assert np.abs(a - b).max() > 1e-4 and rsr.explain_excursions(wk, a, b, 1e-4, 1e-9) == []
    b[2, 3] = (0.0, 0.0, 1.0 - 1e-6)                               # ... but not if it then misses the alternative
    assert [e[:2] for e in rsr.explain_excursions(wk, a, b, 1e-4, 1e-9)] == [(2, 3)]
    b[2, 3] = a[2, 3]
    b[5, 5] += 2e-4                                                # a decided pixel beyond the bar is never explained
    assert [(e[0], e[1], e[3]) for e in rsr.explain_excursions(wk, a, b, 1e-4, 1e-9)] == [(5, 5, "decided")]


def test_pixel_decisions_list_the_margins_the_walk_counted():
    """pixel_decisions (what a failing GPU test is read with) agrees with the frame walk on every ambiguous pixel, and on a
    decided one every distance exceeds its bound."""
    for name in ("dense_96x96", "random_256x256_n2000_t16"):
        R, wk = std_case(name)[8], std_case(name)[9]
        assert wk.ambiguous.any()
        for y, x in zip(*np.nonzero(wk.ambiguous)):
            decs = rsr.pixel_decisions(rsr.STD_3DGS, R, int(x), int(y))
            amb = [d for d in decs if d.ambiguous]
            print("%s (%d, %d): %s" % (name, y, x, ["%s %.3g within %.3g" % (d.kind, d.distance, d.bound) for d in amb]))
            assert len(amb) == wk.n_ambiguous[y, x] and all(d.distance <= d.bound for d in amb)
        decs = rsr.pixel_decisions(rsr.STD_3DGS, R, 40, 40)
        assert wk.n_ambiguous[40, 40] == 0 and decs and all(d.distance > d.bound or d.bound == 0 for d in decs)
        assert sum(d.kind == "stop" and not d.taken for d in decs) == wk.composited[40, 40]


def test_more_than_three_ambiguous_decisions_leave_the_pixel_out():
    thr = rsr.STD_3DGS.skip_threshold
    n = 4
    R = rsr.Records(np.full(n, 1.0), np.full(n, 1.0), np.full(n, 0.5), np.zeros(n), np.full(n, 0.5),
                    np.full(n, thr * (1 + 1e-8)), np.ones((n, 3)), np.tile(np.array([[0, 4, 0, 4]]), (n, 1)), np.arange(n))
    wk = rsr.walk(rsr.STD_3DGS, R, 4, 4)
    assert wk.left_out == [(1, 1)]
    wk3 = rsr.walk(rsr.STD_3DGS, rsr.Records(*[a[:3] for a in R]), 4, 4)
    assert not wk3.left_out and wk3.alternatives[(1, 1)].shape == (8, 3)
