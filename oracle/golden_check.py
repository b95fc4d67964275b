"""Holds an implementation's stage 1 against what the REFERENCE computed at a benchmark size.

TEST INFRASTRUCTURE ONLY (tests/, bench.py's reference check): the fixtures ``tests/golden/stage1_*.npz`` are made
by ``oracle/capture_golden.py`` from the reference's own ``GaussianScene.preprocess`` (splat/gaussian_scene.py:70-144)
on BASELINE's configurations C2 (1e5 Gaussians) and C3 (1e6), 1080p.  Nothing here reads /root/reference.
"""
from __future__ import annotations

import ast
import hashlib
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
STAGE1_FIELDS = ("points_xy", "covariance_2d", "depths", "inverse_covariance_2d", "radius", "min_x", "max_x", "min_y",
                 "max_y", "colors")


def sha256(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load(name: str):
    return np.load(os.path.join(GOLDEN_DIR, name + ".npz"))


def stage1_scene(g):
    """The inputs of a stage-1 fixture, regenerated from its generator arguments (a frozen numpy stream) and checked
    against the hash of what the reference was given."""
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    sc = make_scene(**dict(ast.literal_eval(str(g["generator"]))))
    got = sha256(np.concatenate([sc[k].reshape(-1) for k in ("points", "colors_0_255", "scales", "quaternions", "opacity")]))
    assert got == str(g["inputs_sha256"]), "the synthetic generator no longer produces the scene the fixture was made from"
    return sc


def compare_stage1_with_reference(g, fields, order, strict: bool = True, sigmoid=None) -> dict:
    """``fields``: the PreprocessedScene arrays of an implementation in ITS depth order, ``order``: the original index
    of each of its rows.  Holds them against what the REFERENCE computed for the same scene (a stage-1 fixture):
    every array, put back in original Gaussian order, bit for bit (SHA-256 of 1e5 / 1e6 rows; where the fixture holds
    the array itself, also entry by entry), and the permutation -- equal to the reference's except inside runs of
    EQUAL depths, where the reference's unstable argsort (splat/gaussian_scene.py:117) leaves the order to its sort
    library and this build takes the original index.  Returns the counts a report wants; ``strict``: any difference
    outside equal depths is an AssertionError (tests), otherwise it is only counted (bench.py)."""
    n = int(g["n"])
    order = np.asarray(order, np.int64)
    report = dict(n=n, n_visible_ref=int(g["n_visible"]), n_visible=int(order.size), arrays_differing=[],
                  depth_bit_diffs=0, radius_flips=0, bbox_flips=0, order_diffs_outside_ties=0)
    if order.size != int(g["n_visible"]):
        assert not strict, "visible Gaussians: %d, the reference has %d" % (order.size, int(g["n_visible"]))
        report["arrays_differing"] = ["n_visible"]
        return report
    stored = {"points_xy": "points_xy", "covariance_2d": "covariance_2d", "depths": "depths", "radius": "radius"}
    for f in STAGE1_FIELDS:
        a = np.ascontiguousarray(fields[f])
        full = np.zeros((n,) + a.shape[1:], a.dtype)
        full[order] = a
        if sha256(full) == str(g["sha256_" + f]):
            continue
        count = -1                      # (unknown: the compact fixture holds only the hash)
        if f in stored and stored[f] in g:
            count = int(np.count_nonzero(full.view(np.uint32) != np.asarray(g[stored[f]], np.float32).view(np.uint32)))
        elif f in ("min_x", "max_x", "min_y", "max_y") and "bbox" in g:
            count = int(np.count_nonzero(full != g["bbox"][:, ("min_x", "max_x", "min_y", "max_y").index(f)].astype(np.float32)))
        report["arrays_differing"].append(f)
        key = {"depths": "depth_bit_diffs", "radius": "radius_flips"}.get(f, "bbox_flips" if f in ("min_x", "max_x", "min_y", "max_y") else None)
        if key:
            report[key] = count if report[key] == 0 or count < 0 else report[key] + count
    if sigmoid is not None and "sha256_sigmoid_opacity" in g:
        # sigmoid(opacity) in sorted order, put back by index: the restatements follow torch's SIMD sigmoid down to the
        # libm tails of its threads' chunks (a kernel cannot know those: it is held to 1 ulp on < 32 values per thread)
        full = np.zeros((n, 1), np.float32)
        full[order] = np.asarray(sigmoid, np.float32).reshape(-1, 1)
        if sha256(full) != str(g["sha256_sigmoid_opacity"]):
            report["arrays_differing"].append("sigmoid_opacity")
    assert not (strict and report["arrays_differing"]), "arrays that differ from the reference's: %r" % report
    # the permutation: ours with the reference's choice inside every tie run == the reference's
    pos, ref_members = g["tie_positions"].astype(np.int64), g["tie_order"].astype(np.int64)
    depths = np.ascontiguousarray(fields["depths"], np.float32).reshape(-1).view(np.uint32)
    in_run = np.zeros(order.size, bool)
    in_run[pos] = True
    same_next = np.concatenate([depths[1:] == depths[:-1], [False]])
    runs_match = bool(np.array_equal(in_run, same_next | np.concatenate([[False], same_next[:-1]])))
    ours = order[pos] if runs_match else np.zeros(0, np.int64)
    if runs_match:
        run_start = np.concatenate([[True], depths[pos][1:] != depths[pos][:-1]])
        by_index = bool(np.all((np.diff(ours) > 0) | run_start[1:]))      # inside a run: original-index order (stable sort)
        patched = order.copy()
        patched[pos] = ref_members
        outside_ok = sha256(patched.astype(np.int32)) == str(g["order_sha256"])
    else:
        by_index = outside_ok = False
    if strict:
        assert runs_match, "runs of equal depths are elsewhere than in the reference's output"
        assert by_index, "equal depths are not in original-index order"
        assert outside_ok, "the permutation differs from the reference's outside equal depths"
    report.update(tied=int(pos.size), order_diffs_inside_ties=int(np.count_nonzero(ours != ref_members)) if runs_match else -1,
                  order_diffs_outside_ties=0 if outside_ok else -1)
    return report


# ----------------------------------------------------------------- reference-rendered tiles at the metric's configuration
TILE_FIXTURE_NAMES = ("tiles_c2_1080p_n100000", "tiles_c3_1080p_n1000000", "tiles_c4_4k_n5000000", "tiles_c3_clustered_1080p_n1000000",
                      "tiles_c3_trainedlike_1080p_n1000000")


def tiles_scene(g):
    """The inputs of a ``tiles_*`` fixture (oracle/capture_golden.py: capture_tiles), regenerated from its generator
    arguments and checked against the hash of what the reference was given.  The reference has no spherical harmonics:
    the trained-like scene is rendered with its base colours."""
    from intro_to_gaussian_splatting_amd import synthetic

    gen = {"scene": synthetic.make_scene, "trained": synthetic.make_trained_like_scene}[str(g["generator_name"])]
    sc = gen(**dict(ast.literal_eval(str(g["generator"]))))
    sc.pop("sh", None)
    sc.pop("sh_degree", None)
    got = sha256(np.concatenate([sc[k].reshape(-1) for k in ("points", "colors_0_255", "scales", "quaternions", "opacity")]))
    assert got == str(g["inputs_sha256"]), "the synthetic generator no longer produces the scene the fixture was made from"
    return sc


def tile_lists(g):
    """Per tile of a ``tiles_*`` fixture: ((tx, ty), original Gaussian indices in the REFERENCE's compositing order)."""
    off = np.concatenate([[0], np.cumsum(g["list_len"])]).astype(np.int64)
    return [((int(t[0]), int(t[1])), g["list_indices"][off[k]:off[k + 1]].astype(np.int64)) for k, t in enumerate(g["tiles"])]


def compare_tiles_with_reference(g, image_whc) -> dict:
    """``image_whc``: a frame (W, H, 3) indexed [x, y] of the fixture's scene.  Its 16x16 blocks at the fixture's tiles
    against what the REFERENCE's own ``render_tile`` (splat/gaussian_scene.py:173-198) returned for them."""
    t = int(g["tile"])
    image_whc = np.asarray(image_whc)
    per_tile = []
    for k, (tx, ty) in enumerate(g["tiles"]):
        blk = image_whc[tx * t:(tx + 1) * t, ty * t:(ty + 1) * t]
        per_tile.append(float(np.abs(blk - g["blocks"][k]).max()))
    return dict(tiles=int(len(per_tile)), max_abs=float(max(per_tile)), per_tile=per_tile,
                pixels_over_1e4=int(sum(int((np.abs(image_whc[tx * t:(tx + 1) * t, ty * t:(ty + 1) * t] - g["blocks"][k]).max(axis=2) > 1e-4).sum())
                                        for k, (tx, ty) in enumerate(g["tiles"]))),
                longest_list=int(g["list_len"].max()), tie_swapped_entries=int(g["tie_swapped"].sum()))


def rows_in_reference_order(pre_order, g):
    """Rows of a depth-sorted stage 1 (``pre_order``: original index of each row; ties by index) rearranged into the
    REFERENCE's permutation: a stage-1 fixture records what torch.argsort did inside every run of equal depths
    (``tie_positions`` / ``tie_order``).  Returns the row numbers in the reference's compositing order."""
    order = np.asarray(pre_order, np.int64)
    patched = order.copy()
    patched[g["tie_positions"].astype(np.int64)] = g["tie_order"].astype(np.int64)
    inv = np.full(int(g["n"]), -1, np.int64)
    inv[order] = np.arange(order.size)
    rows = inv[patched]
    assert (rows >= 0).all() and np.array_equal(np.sort(rows), np.arange(order.size))
    return rows


FUZZ_TILE_FIXTURE_NAMES = ["fuzz_tiles_seeds_8000"]


def fuzz_stage1_cases(g):
    """Per case of a ``fuzz_stage1_*`` fixture (oracle/capture_golden.py: capture_fuzz_stage1 -- the reference's own preprocess of
    random scenes): (seed, whether the numpy restatement is held against it too, the scene's arrays regenerated from the seed and
    checked against the hash of what the reference was given, the reference's camera as a cpu_ref.Camera, the case's record: its row
    and its ``s<seed>_*`` arrays under their names without the prefix)."""
    from oracle import cpu_ref, fuzz_vs_reference

    cols = [str(c) for c in g["columns"]]
    for r in g["rows"]:
        rec = dict(zip(cols, (int(v) for v in r)))
        p = "s%d_" % rec["seed"]
        rec.update({k[len(p):]: g[k] for k in g.files if k.startswith(p)})
        case = fuzz_vs_reference.random_case(rec["seed"], False)
        sc = case["gen"](**case["args"])
        sc.pop("sh", None)
        sc.pop("sh_degree", None)
        assert sha256(np.concatenate([sc[k].reshape(-1) for k in ("points", "colors_0_255", "scales", "quaternions", "opacity")])) \
            == str(rec["inputs_sha256"]), "the generator no longer makes the scene the reference was given (seed %d)" % rec["seed"]
        cam = cpu_ref.Camera(rec["world2view"], rec["full_proj_transform"], rec["tan_fovX"][0], rec["tan_fovY"][0], rec["f_x"][0],
                             rec["f_y"][0], rec["width"], rec["height"])
        yield rec["seed"], bool(rec["numpy_too"]), sc, cam, rec


def fuzz_tiles_cases(g):
    """Per scene of a ``fuzz_tiles_*`` fixture (oracle/capture_golden.py: capture_fuzz_tiles -- random scenes whose tiles the REFERENCE's
    own ``render_tile`` composited): (seed, the scene's arrays regenerated from the seed, its row dict, [(tx, ty, list length, block)])."""
    from oracle import fuzz_vs_reference

    cols = [str(c) for c in g["columns"]]
    rows = [dict(zip(cols, (int(v) for v in r))) for r in g["rows"]]
    for seed in sorted({r["seed"] for r in rows}):
        case = fuzz_vs_reference.random_case(seed, "tiles")
        sc = case["gen"](**case["args"])
        sc.pop("sh", None)
        sc.pop("sh_degree", None)
        mine = [(k, r) for k, r in enumerate(rows) if r["seed"] == seed]
        yield seed, sc, mine[0][1], [(r["tx"], r["ty"], r["list_len"], g["blocks"][k]) for k, r in mine]

