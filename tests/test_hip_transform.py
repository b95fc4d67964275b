"""gsx_transform_gaussians on the GPU (csrc/gsx_transform.hip), Gaussians.transform, GaussianScene.transform and normalize().

Bits: the four arrays equal the float32 restatement (tests/transform_restatement.py) bit for bit, from a 16-byte aligned base,
from a base one row further (which at 3 K = 12 and 48 floats per row is still 16-byte aligned) and from a base one float
further (where no array is); every array lies between two 64-element margins of a sentinel that must survive.

Frames: the transformed scene seen from the transformed cameras is the frame that was rendered before, to the project's pixel
tolerance of 1e-4 at every pixel, with the rotations of tests/transform_cases.py (chosen on the CPU, by the oracle alone).
D of render_image_depth_hip is a sum of T alpha z with z up to Z = the largest view depth where a colour is a sum of
T alpha c with c up to 1, so the tolerance of D / s is 1e-4 Z; coverage is held to 1e-4.

Printed on an MI355X:
    SH invariance, device / float32 mirror (s = 1, s = 2.5): degree 1 1.00, 1.08; degree 2 0.99, 0.70; degree 3 1.22, 0.79
      (absolute 2.9e-07 .. 9.2e-07 on the device, 2.9e-07 .. 1.1e-06 in the mirror)
    frames before / after, max|dpixel| (coverage, D / s): small 1.1e-06 and 1.5e-06 (1.5e-06, 1.2e-05); dense 1.0e-06 and
      1.1e-06 (1.0e-06, 5.3e-06); trained-like SH 5.8e-06 and 1.1e-05 (2.5e-06, 4.0e-05)
    normalize: extent ((0.871, 0.809, -3.450), 1.204320) -> (|c| <= 5.8e-08, 1.00000001); five views within 1.8e-06
      (coverage 2.7e-06, D / s 2.6e-05); round trip: worst |dp| / bound 0.518, worst error 4.00 ulp of max(|p_k|, |c_k|)
"""
import ctypes
import os
import shutil

import numpy as np
import pytest
import torch

import sh_backward_restatement as sr
import transform_cases as tc
import transform_restatement as tr
from test_hip_density import Guarded
from test_kernel_resources import HIPCC, _resources
from test_transform_host import _struct, rotation

from intro_to_gaussian_splatting_amd import transform as T

gpu = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 3, 255, 256, 257, 1000]
STORED = ["rgb", 0, 1, 2, 3]                 # an RGB container (sh NULL), and SH containers stored at degree 0..3
BASES = ["aligned", "row", "float"]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _inputs(n, stored, seed=0):
    rs = np.random.RandomState(977 * n + seed)
    p = (rs.normal(size=(n, 3)) * 4).astype(np.float32)
    c = np.exp(rs.normal(size=(n, 3))).astype(np.float32)
    q = rs.normal(size=(n, 4)).astype(np.float32)
    sh = None
    if stored != "rgb":
        sh = rs.normal(size=(n, (stored + 1) ** 2, 3)).astype(np.float32)
        sh[1::5, 4:] = 0.0              # a tail of zeros, as an SH degree schedule leaves it ...
        sh[3::5, 4:] = -0.0             # ... of either sign
    return p, c, q, sh


def _call(p, c, q, sh, degree, sim, base):
    """One library call on guarded copies; returns (the four outputs as numpy, sh None for an RGB container)."""
    from intro_to_gaussian_splatting_amd import _ffi

    n = p.shape[0]
    held = []
    for a in (p, c, q, sh):
        if a is None:
            held.append(None)
            continue
        width = a.size // n
        g = Guarded(a.size, lead={"aligned": 0, "row": width, "float": 1}[base])
        g.view.copy_(torch.from_numpy(a.reshape(-1)))
        held.append(g)
    ptr = [None if g is None else g.view.data_ptr() for g in held]
    if base == "aligned":
        assert all(v is None or v % 16 == 0 for v in ptr)
    if base == "float":
        assert all(v is None or v % 16 == 4 for v in ptr)
    t = _struct(sim)
    rc = _ffi.load().gsx_transform_gaussians(ptr[0], ptr[1], ptr[2], ptr[3], degree, n, ctypes.byref(t), _stream())
    assert rc == 0, _ffi.load().gsx_last_error()
    torch.cuda.synchronize()
    for g in held:
        assert g is None or g.intact(), "a margin was written"
    return [None if g is None else g.view.cpu().numpy().reshape(a.shape) for g, a in zip(held, (p, c, q, sh))]


@gpu
@pytest.mark.parametrize("stored", STORED)
@pytest.mark.parametrize("n", SIZES)
def test_the_arrays_are_the_restatements_bit_for_bit_from_any_base(n, stored):
    p, c, q, sh = _inputs(n, stored)
    degree = 0 if stored == "rgb" else stored
    sim = T.similarity(rotation(n + degree)[0], 2.5, [1.5, -0.75, 2.0])
    want = tr.transform(p, c, q, sh, degree, tr.host_arguments(sim))
    if sh is not None:
        assert _same(want[3][:, 0], sh[:, 0]) and (degree == 0 or not _same(want[3], sh))
        assert not want[3][1::5, 4:].any() and not want[3][3::5, 4:].any()
    first = None
    for base in BASES:
        got = _call(p, c, q, sh, degree, sim, base)
        for name, g, w in zip(("points", "scales", "quaternions", "sh"), got, want):
            assert (g is None) == (w is None), name
            assert g is None or _same(g, w), "%s differs from the restatement, n = %d, stored %r, base %s" % (name, n, stored, base)
        if first is None:
            first = got
        for g, f in zip(got, first):
            assert g is None or _same(g, f)


def _container(n=1000, degree=3, seed=1):
    from intro_to_gaussian_splatting_amd import Gaussians

    p, c, q, sh = _inputs(n, degree, seed)
    rs = np.random.RandomState(seed)
    g = Gaussians.from_arrays(p, rs.uniform(0, 255, (n, 3)).astype(np.float32), c, q, rs.normal(size=(n, 1)).astype(np.float32),
                              device=DEV)
    g.sh = torch.from_numpy(sh).to(DEV).contiguous()
    g.sh_degree = degree
    return g, (p, c, q, sh)


@gpu
def test_gaussians_transform_is_the_one_call_and_leaves_the_rest_alone():
    g, (p, c, q, sh) = _container()
    g.active_sh_degree = 1                  # every STORED band is rotated, whatever is active
    g.points.requires_grad_(True)
    g.points.grad = torch.full_like(g.points, 7.0)
    opacity, colors = g.opacity.clone(), g.colors.clone()
    versions = [a._version for a in (g.points, g.scales, g.quaternions, g.sh)]
    ptrs = [a.data_ptr() for a in (g.points, g.scales, g.quaternions, g.sh)]
    R = rotation(11)[0]
    assert g.transform(R, 2.5, [1.5, -0.75, 2.0]) is None
    sim = T.similarity(R, 2.5, [1.5, -0.75, 2.0])
    want = tr.transform(p, c, q, sh, 3, tr.host_arguments(sim))
    for a, w, v, ptr in zip((g.points, g.scales, g.quaternions, g.sh), want, versions, ptrs):
        assert _same(a.detach().cpu().numpy(), w) and a._version > v and a.data_ptr() == ptr
    assert torch.equal(g.opacity, opacity) and torch.equal(g.colors, colors)
    assert g.points.requires_grad and bool((g.points.grad == 7.0).all()) and g.active_sh_degree == 1
    # refused: arrays that are not leaves while gradients are enabled -- and nothing is written
    before = g.scales.clone()
    leaf = g.scales
    g.scales = (leaf.requires_grad_(True) * 1.0)
    with pytest.raises(ValueError, match="scales is not a leaf"):
        g.transform(R)
    with torch.no_grad():
        g.transform(np.eye(3))              # the identity, allowed without gradients
    assert torch.equal(g.scales.detach(), before)
    # an empty container is a no-op
    from intro_to_gaussian_splatting_amd import Gaussians

    Gaussians(torch.zeros(0, 3), torch.zeros(0, 3), device=DEV).transform(R, 2.0)


@gpu
@pytest.mark.parametrize("degree", [1, 2, 3])
def test_sh_invariance_is_held_to_the_float32_mirrors_own_error(degree):
    """gsx_sh_to_rgb on the transformed coefficients and means, from the transformed camera centre, against the float64
    colour of the ORIGINAL scene; the numpy float32 mirror of the same chain (restated transform, then
    transform_restatement.sh_colors_float32) errs against the same float64 colours on the same data.  The device may err at
    most 4 x the mirror: the margin covers the device's direction normalisation (a reciprocal and three products where the
    mirror divides) and nothing else.  Measured on an MI355X: see the module docstring."""
    from intro_to_gaussian_splatting_amd import _ffi

    n = 1000
    worst = 0.0
    for seed, (s, t) in enumerate([(1.0, [0.0, 0.0, 0.0]), (2.5, [1.5, -0.75, 2.0])]):
        p, c, q, sh = _inputs(n, degree, seed)
        center = np.array([0.3, -0.2, 9.0], np.float32)
        sim = T.similarity(rotation(40 + seed)[0], s, t)
        exact = sr.colors(p, sh, degree, center)                              # float64, the original scene
        center2 = sim.apply(center.astype(np.float64)).astype(np.float32)
        P, _, _, S = tr.transform(p, c, q, sh, degree, tr.host_arguments(sim))
        mirror = np.abs(tr.sh_colors_float32(P, S, degree, center2).astype(np.float64) - exact).max()
        got = _call(p, c, q, sh, degree, sim, "aligned")
        dp, ds = torch.from_numpy(got[0]).to(DEV), torch.from_numpy(got[3]).to(DEV)
        out = torch.empty((n, 3), dtype=torch.float32, device=DEV)
        cc = (ctypes.c_float * 3)(*[float(v) for v in center2])
        _ffi.check(_ffi.load().gsx_sh_to_rgb(dp.data_ptr(), ds.data_ptr(), degree, n, cc, out.data_ptr(), _stream()))
        device = np.abs(out.cpu().numpy().astype(np.float64) - exact).max()
        print("degree %d, s = %g: device %.3g, float32 mirror %.3g, ratio %.2f" % (degree, s, device, mirror, device / mirror))
        assert mirror > 0.0 and exact.max() > 1.0
        assert device <= 4.0 * mirror
        worst = max(worst, device / mirror)
    print("degree %d: worst ratio %.2f" % (degree, worst))


def _gpu_scene(path, name, extra_poses=None, ordered=False):
    from intro_to_gaussian_splatting_amd import GaussianScene, Gaussians
    from intro_to_gaussian_splatting_amd.synthetic import write_colmap_text

    sc = tc.scene_arrays(name)
    write_colmap_text(str(path), sc, extra_poses=extra_poses)
    g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"], device=DEV)
    if "sh" in sc:
        g.sh = torch.from_numpy(sc["sh"]).to(DEV).contiguous()
        g.sh_degree = int(sc["sh_degree"])
    return GaussianScene(str(path), g.spatially_ordered() if ordered else g), sc


def _frames(scene, tile, views=(1,)):
    out = []
    with torch.no_grad():
        for v in views:
            frame, depth = scene.render_image_depth_hip(v, tile_size=tile)
            assert torch.equal(frame, scene.render_image_hip(v, tile_size=tile))
            out.append((frame.clone(), depth.clone()))
    return out


def _assert_same_frames(before, after, s, zmax, what):
    for (f0, d0), (f1, d1) in zip(before, after):
        assert float(f0.max()) > 0.5
        ef = float((f1 - f0).abs().max())
        ea = float((d1[..., 1] - d0[..., 1]).abs().max())
        ed = float((d1[..., 0] / s - d0[..., 0]).abs().max())
        print("%s: max|dpixel| %.3g, coverage %.3g, D / s %.3g (D up to %.3g, tolerance %.3g)"
              % (what, ef, ea, ed, float(d0[..., 0].max()), tc.PIXEL_TOLERANCE * zmax))
        assert ef <= tc.PIXEL_TOLERANCE and ea <= tc.PIXEL_TOLERANCE and ed <= tc.PIXEL_TOLERANCE * zmax


@gpu
@pytest.mark.parametrize("name,kind", tc.CASES)
def test_the_transformed_scene_from_the_transformed_camera_is_the_same_frame(tmp_path, name, kind):
    scene, sc = _gpu_scene(tmp_path, name)
    if scene.gaussians.sh is not None:
        scene.gaussians.sh.requires_grad_(True)     # render_image_depth_hip takes an SH scene only when it is differentiable
    tile = tc.SCENES[name]["tile"]
    zmax = float(tc.view_depths(sc["points"], scene.images[1].world2view.cpu().numpy()).max())
    before = _frames(scene, tile)
    sim = tc.triple(kind, tc.SEEDS[(name, kind)])
    got = scene.transform(*sim)
    assert np.array_equal(got.R, sim.R) and got.s == sim.s and np.array_equal(got.t, sim.t)
    want = tr.transform(sc["points"], sc["scales"], sc["quaternions"], sc.get("sh"), int(sc.get("sh_degree", 0)),
                        tr.host_arguments(sim))
    assert _same(scene.gaussians.points.cpu().numpy(), want[0])
    assert not _same(want[0], sc["points"])
    _assert_same_frames(before, _frames(scene, tile), sim.s, zmax, "%s, %s" % (name, kind))


@gpu
def test_normalize_gives_unit_extent_the_same_frames_and_comes_back(tmp_path):
    """After normalize(): cameras_extent() == (0, 1) to 1e-5 and every view's frame is what it was.  Then
    transform(*inverse(triple)) brings the means back.  With R = I a coordinate goes p -> fl(fl(s p) + t) -> fl(fl(s' p') +
    t'), t = -s c: four roundings of values no larger than |p| + |c| in world units (e = 2^-24 each: e (|p| + 2 (|p| + |c|) +
    |p|)), and s, s', t, t' are themselves rounded (s s' = 1 and t' = c only to 2 e: 2 e |p| + 2 e |c|) -- at most
    e (6 |p| + 4 |c|) <= 10 x 2^-24 max(|p_k|, |c_k|) per coordinate.  Measured on an MI355X: see the module docstring."""
    scene, sc = _gpu_scene(tmp_path, tc.NORMALIZE_SCENE, extra_poses=tc.normalize_poses())
    tile = tc.SCENES[tc.NORMALIZE_SCENE]["tile"]
    views = sorted(scene.images)
    assert len(views) == tc.NORMALIZE_VIEWS
    center, radius = scene.cameras_extent()
    assert radius > 0.5 and np.abs(center).max() > 0.5
    zmax = max(float(tc.view_depths(sc["points"], scene.images[v].world2view.cpu().numpy()).max()) for v in views)
    before = _frames(scene, tile, views)
    triple = scene.normalize()
    assert np.array_equal(triple.R, np.eye(3)) and triple.s == 1.0 / radius and np.array_equal(triple.t, -center / radius)
    c1, r1 = scene.cameras_extent()
    print("normalize: extent (%s, %.6f) -> (%s, %.8f)" % (center, radius, c1, r1))
    assert np.abs(c1).max() <= 1e-5 and abs(r1 - 1.0) <= 1e-5
    _assert_same_frames(before, _frames(scene, tile, views), triple.s, zmax, "normalize, %d views" % len(views))
    scene.transform(*T.inverse(triple))
    back = scene.gaussians.points.cpu().numpy().astype(np.float64)
    p = sc["points"].astype(np.float64)
    bound = 10.0 * 2.0 ** -24 * np.maximum(np.abs(p), np.abs(center)[None, :])
    ratio = np.abs(back - p) / bound
    ulps = np.abs(back - p) / np.spacing(np.maximum(np.abs(sc["points"]), np.abs(center).astype(np.float32)[None, :]))
    print("round trip: worst |dp| / bound %.3f, worst error %.2f ulp of max(|p_k|, |c_k|)" % (ratio.max(), ulps.max()))
    assert ratio.max() <= 1.0
    c2, r2 = scene.cameras_extent()
    assert np.abs(c2 - center).max() <= 1e-5 * radius and abs(r2 - radius) <= 1e-5 * radius


@gpu
def test_a_spatially_ordered_container_follows_the_transform(tmp_path):
    """After transform the bounds a frame reads are the fresh ones (the kernel wrote through raw pointers: the version bump
    is what current_block_bounds() sees), and the ordered scene's frames -- whole and a tile window, whose projection drops
    blocks by those bounds -- are the unordered scene's bit for bit, as before the transform."""
    name, kind = "trainedlike_sh_128x128_n3000", "similarity"
    plain, _ = _gpu_scene(tmp_path, name)
    ordered, _ = _gpu_scene(tmp_path, name, ordered=True)
    g = ordered.gaussians
    assert g.original_index is not None
    tile, win = tc.SCENES[name]["tile"], (2, 6, 1, 5)
    with torch.no_grad():
        assert torch.equal(plain.render_image_hip(1, tile_size=tile, tile_window=win),
                           ordered.render_image_hip(1, tile_size=tile, tile_window=win))
    stale = g.current_block_bounds().clone()
    sim = tc.triple(kind, tc.SEEDS[(name, kind)])
    plain.transform(*sim)
    ordered.transform(*sim)
    assert torch.equal(g.points, plain.gaussians.points[g.original_index.long()])
    current = g.current_block_bounds().clone()
    g.refresh_block_bounds()
    assert torch.equal(current, g.block_bounds) and not torch.equal(current, stale)
    lo, hi = current[:, 0:3], current[:, 4:7]
    rows = g.points.reshape(-1, 3)
    for b in (0, current.shape[0] - 1):
        blk = rows[256 * b:256 * (b + 1)]
        assert torch.equal(lo[b], blk.amin(dim=0)) and torch.equal(hi[b], blk.amax(dim=0))
    with torch.no_grad():
        assert torch.equal(plain.render_image_hip(1, tile_size=tile), ordered.render_image_hip(1, tile_size=tile))
        a = plain.render_image_hip(1, tile_size=tile, tile_window=win)
        assert float(a.max()) > 0.1
        assert torch.equal(a, ordered.render_image_hip(1, tile_size=tile, tile_window=win))


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_the_kernel_uses_no_scratch():
    """From the compiler's own report (tools/kres.py's source; hipcc cross-compiles, no GPU): every instance of
    transform_kernel compiles for gfx950 without scratch, with the LDS of the padded 256 x (3 K + 1) coefficient block, and
    at the occupancy DESIGN.md section 8b "Scene transforms" records."""
    table = _resources("gsx_transform.hip")
    assert sorted(table) == ["transform_kernel<%d>" % d for d in range(4)], sorted(table)
    for d in range(4):
        r = table["transform_kernel<%d>" % d]
        print(d, r)
        k = (d + 1) ** 2
        assert r["ScratchSize"] == 0, r
        assert r["LDS"] == (4 * 256 * (3 * k + 1) if d else 0), r
        assert r["VGPRs"] <= 80 and r["Occupancy"] >= (8, 8, 5, 3)[d], r
