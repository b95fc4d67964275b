"""Geometry-gradient fixtures: the REFERENCE ITSELF under autograd, with its one graph cut mended.  Data only.

Build container only, like tools/capture_grad_golden.py, whose recipe this follows (oracle.capture_golden's
_import_reference and _generate; nothing under oracle/ is changed).  Everything in the reference's preprocess is
differentiable torch; only compute_gaussian_weight ends in `.item()`.  The name compute_gaussian_weight in the
reference's gaussian_scene module is rebound at run time to `_weight` below, which returns the same value as a tensor.
For every scene: L = sum(image * W) and torch.autograd.grad(L, [points, scales, quaternions, colors, opacity]) of the
reference's own render_image.

Before anything is written the tool ASSERTS that the rebinding changed nothing else: the image, grad_colors and
grad_opacity must equal the committed tests/golden/grad_<scene>.npz bit for bit.  The scenes of STANDALONE have no
grad_ fixture; their image is asserted against the committed forward fixture tests/golden/<scene>.npz instead, and
their file also holds the scene arguments, W, the image, grad_colors and grad_opacity.  The scenes of OWN_STAGE1 (one to
three visible Gaussians, each on a rendered tile) have no forward fixture either: the reference renders them a second
time with its ORIGINAL compute_gaussian_weight under no_grad, the two images must be equal bit for bit, and their file
also holds the reference's camera constants and PreprocessedScene arrays under the keys of oracle/capture_golden.py.
The scenes of CAMERA_SCENES (unequal focal lengths, far poses: the cameras of tests/camera_cases.py) are treated likewise.

    python tools/capture_geometry_grad_golden.py            # all scenes
    python tools/capture_geometry_grad_golden.py tile2      # only those whose name contains "tile2"
    python tools/capture_geometry_grad_golden.py --check    # recount the branch table over the committed files

Writes tests/golden/geomgrad_<scene>.npz: grad_points (N,3), grad_scales (N,3), grad_quaternions (N,4) and the three
branch counts (floored determinant, active clamp, culled) recounted from the reference's own stage 1.  A full run
refuses to finish if one of the three branches is hit by no scene of the set.
"""
from __future__ import annotations

import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.capture_golden import FIXTURES, OUT_DIR, _generate, _import_reference  # noqa: E402

SCENES = ["tile2_40x32_n80", "small_64x48_n300", "small_80x64_n120_tile8", "tile12_dense_52x40_n900",
          "tile20_64x64_n300", "tile32_96x96_n400", "needle_160x160_n110", "tiny_48x48_n600",
          "wide_64x64_n400", "cull_96x80_n400"]
# Not in the set: trainedlike_128x128_n3000.  The graph through the geometry is several times the colour-only one (needle,
# 110 Gaussians: over 21 GB); name it on the command line on a machine with the memory and an hour to spare.
EXTRA = ["trainedlike_128x128_n3000"]
STANDALONE = ("wide_64x64_n400", "cull_96x80_n400")     # no grad_ fixture: the file carries its own inputs
# No forward fixture and no grad_ fixture: name -> generator arguments (the table of oracle/capture_golden.py's FIXTURES).
# The row classes of one to three visible Gaussians (GSX_FLAG_ONE_VISIBLE / GSX_FLAG_SMALL_BATCH), every visible Gaussian
# on a rendered tile; the forward fixtures single_48x48_n1 and onevisible_48x48_n7 have theirs on no rendered pixel.
OWN_STAGE1 = {
    "rows1_48x48_n1": dict(n=1, width=48, height=48, seed=40, tile=16),
    "rows3_48x48_n3": dict(n=3, width=48, height=48, seed=40, tile=16),
    "rows1_48x48_n500": dict(n=500, width=48, height=48, seed=41, tile=16, generator="few", visible=1),
    "rows3_48x48_n500": dict(n=500, width=48, height=48, seed=43, tile=16, generator="few", visible=3),
}
# The cameras of tests/camera_cases.py (unequal focal lengths, far poses); treated like OWN_STAGE1.  Each scene lies in its
# camera's own frustum.  aniso: floored determinants (footprints of a quarter of the usual size); aniso_tall: the clamp
# with limx != limy; farpose: the cull.  roll keeps the usual footprints: the central differences of tests/test_depth_host.py step by 5e-5 of
# a world unit, which a footprint well below a pixel does not resolve to their 1e-7.
CAMERA_SCENES = {
    "cam_aniso_64x48_n120": dict(n=120, width=64, height=48, seed=75, tile=16, fx=40.0, fy=62.0, sigma_scale=0.25,
                                 sigma_ln=0.8),
    "cam_aniso_tall_48x64_n100": dict(n=100, width=48, height=64, seed=73, tile=16, fx=70.0, fy=30.0,
                                      qvec=(0.8, 0.3, -0.45, 0.25), tvec=(-0.7, 0.2, 2.1), spread=2.0, sigma_scale=3.0),
    "cam_farpose_64x48_n120": dict(n=120, width=64, height=48, seed=79, tile=16, fx=48.0, fy=48.0,
                                   qvec=(0.35, 0.6, -0.55, 0.46), tvec=(0.4, -0.9, 1.5), behind_fraction=0.25),
    "cam_roll_64x48_n100": dict(n=100, width=64, height=48, seed=89, tile=16, fx=36.0, fy=52.0,
                                qvec=(0.05, 0.1, -0.08, 0.99), tvec=(-0.3, 0.5, 2.0)),
}
# the two of them that also get camera, depth, screen and abs fixtures (tools/capture_{camera,depth,screen,abs}_grad_golden.py)
CAMERA_ENTRY_SCENES = ["cam_aniso_tall_48x64_n100", "cam_roll_64x48_n100"]
OWN_STAGE1.update(CAMERA_SCENES)
SCENES += list(OWN_STAGE1)
# The clean twins of tests/bad_row_cases.py's RGB cases (every non-finite row replaced by a culled finite one; the
# degenerate rows -- zero scales, logits of +-80, colours of 0 and 4, quaternions times 1e-18 and 1e18 -- stay): the
# reference runs on finite rows only.  fixture -> case; the arrays come from that module, treated like OWN_STAGE1.
BAD_ROW_TWINS = {"badrow_base_twin_64x48_n300": "base", "badrow_roll_twin_64x48_n300": "roll"}
SCENES += list(BAD_ROW_TWINS)
BRANCHES = ("n_floored_det", "n_clamped", "n_culled")


def _weight(pixel_coord, point_mean, inverse_covariance):
    """exp(-0.5 d Q d^T) as a (1, 1) tensor: the reference's value without its `.item()`."""
    import torch

    d = point_mean - pixel_coord
    return torch.exp(-0.5 * d @ inverse_covariance @ d.T)


def scene_arrays(name: str):
    """(scene dict, tile, own) of a scene of any of the gradient capture tools.  own: the scene has no forward fixture
    and no grad_ fixture (OWN_STAGE1, BAD_ROW_TWINS): its geomgrad_ file carries its inputs and the reference's stage 1."""
    own = name in OWN_STAGE1 or name in BAD_ROW_TWINS
    if name in BAD_ROW_TWINS:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import bad_row_cases

        return dict(bad_row_cases.rgb_case(BAD_ROW_TWINS[name])[1]), bad_row_cases.TILE, own
    spec = dict(OWN_STAGE1[name] if own else FIXTURES[name])
    tile = spec.pop("tile")
    assert not spec.pop("defaults", False)
    return _generate(spec), tile, own


def reference_colors(sc, g):
    """The colour array the reference renders: its own (colors_0_255 / 256) unless the scene dict carries one."""
    import torch

    return (torch.from_numpy(sc["colors"]) if "colors" in sc else g.colors.detach()).clone()


def branch_counts(scene, g) -> dict:
    """How many Gaussians take each piecewise branch of the reference's stage 1 (its own functions, no gradient)."""
    import torch
    from splat.utils import in_view_frustum

    with torch.no_grad():
        im = scene.images[1]
        in_view = in_view_frustum(points=g.points, view_matrix=im.world2view)
        pts = g.points[in_view]
        pv = (torch.cat([pts, torch.ones(pts.shape[0], 1)], dim=1) @ im.world2view)[:, :3]
        clamped = ((pv[:, 0] / pv[:, 2]).abs() > 1.3 * im.tan_fovX) | ((pv[:, 1] / pv[:, 2]).abs() > 1.3 * im.tan_fovY)
        c = scene.get_2d_covariance(image_idx=1, points=pts, covariance_3d=g.get_3d_covariance_matrix()[in_view])
        det = c[:, 0, 0] * c[:, 1, 1] - c[:, 0, 1] * c[:, 1, 0]
        return dict(n_floored_det=np.int64((det < 1e-3).sum().item()), n_clamped=np.int64(clamped.sum().item()),
                    n_culled=np.int64((~in_view).sum().item()))


def own_stage1(scene, g) -> dict:
    """The reference's camera constants and PreprocessedScene arrays (no gradient), keyed as oracle/capture_golden.py
    keys them: what conftest.oracle_camera and conftest.golden_preprocessed read."""
    import torch
    from splat.utils import in_view_frustum

    with torch.no_grad():
        cam = scene.images[1]
        in_view = in_view_frustum(points=g.points, view_matrix=cam.world2view)
        pre = scene.preprocess(1)
        hom = torch.cat([g.points[in_view], torch.ones(int(in_view.sum()), 1)], dim=1)
        depth_unsorted = (hom @ cam.world2view)[:, 2]
        perm = torch.argsort(depth_unsorted)
        assert torch.equal(depth_unsorted[perm], pre.depths), "argsort is not reproducible"
    num = lambda t: t.detach().numpy()  # noqa: E731
    return dict(
        world2view=num(cam.world2view), full_proj_transform=num(cam.full_proj_transform), tan_fovX=num(cam.tan_fovX),
        tan_fovY=num(cam.tan_fovY), f_x=num(cam.f_x), f_y=num(cam.f_y), in_view=num(in_view),
        order=np.nonzero(num(in_view))[0][num(perm)].astype(np.int64),
        pre_points=num(pre.points), pre_colors=num(pre.colors), pre_covariance_2d=num(pre.covariance_2d),
        pre_depths=num(pre.depths), pre_inverse_covariance_2d=num(pre.inverse_covariance_2d), pre_radius=num(pre.radius),
        pre_points_xy=num(pre.points_xy), pre_min_x=num(pre.min_x), pre_min_y=num(pre.min_y), pre_max_x=num(pre.max_x),
        pre_max_y=num(pre.max_y), pre_sigmoid_opacity=num(pre.sigmoid_opacity))


def capture(name: str, GaussianScene, Gaussians, original_weight=None) -> None:
    import torch

    from intro_to_gaussian_splatting_amd.synthetic import write_colmap_text

    sc, tile, own = scene_arrays(name)
    with tempfile.TemporaryDirectory() as tmp:
        write_colmap_text(os.path.join(tmp, "colmap"), sc)
        g = Gaussians(torch.from_numpy(sc["points"]), torch.from_numpy(sc["colors_0_255"]), model_path=tmp)
        points = torch.from_numpy(sc["points"]).float().clone().requires_grad_(True)
        scales = torch.from_numpy(sc["scales"]).float().clone().requires_grad_(True)
        quats = torch.from_numpy(sc["quaternions"]).float().clone().requires_grad_(True)
        colors = reference_colors(sc, g).requires_grad_(True)
        opacity = torch.from_numpy(np.ascontiguousarray(sc["opacity"], dtype=np.float32)).clone().requires_grad_(True)
        g.points, g.scales, g.quaternions, g.colors, g.opacity = points, scales, quats, colors, opacity
        scene = GaussianScene(os.path.join(tmp, "colmap"), g)
        counts = branch_counts(scene, g)
        stage1 = {}
        if own:     # the reference as it is, once: its `.item()` weight, no graph
            import splat.gaussian_scene as ref_scene

            stage1 = own_stage1(scene, g)
            ref_scene.compute_gaussian_weight = original_weight
            try:
                with torch.no_grad():
                    untouched = scene.render_image(1, tile_size=tile).numpy().copy()
            finally:
                ref_scene.compute_gaussian_weight = _weight
        t0 = time.time()
        image = scene.render_image(1, tile_size=tile)
        t_fwd = time.time() - t0
        W = torch.from_numpy(np.random.default_rng(1000 + len(name)).standard_normal(tuple(image.shape)).astype(np.float32))
        loss = (image * W).sum()
        t0 = time.time()
        grads = torch.autograd.grad(loss, [points, scales, quats, colors, opacity], allow_unused=True)
        t_bwd = time.time() - t0
    n = sc["points"].shape[0]
    gp, gs, gq, gc, go = [np.zeros(tuple(t.shape), np.float32) if v is None else v.numpy()
                          for v, t in zip(grads, [points, scales, quats, colors, opacity])]
    image = image.detach().numpy()
    out = dict(grad_points=gp, grad_scales=gs, grad_quaternions=gq, reference_forward_seconds=np.float64(t_fwd),
               reference_backward_seconds=np.float64(t_bwd), **counts)
    if name in STANDALONE or own:
        if own:
            assert loss.grad_fn is not None and untouched.any(), name + ": no visible Gaussian on a rendered pixel"
            assert np.array_equal(image.view(np.uint32), untouched.view(np.uint32)), \
                name + ": the rebinding changed the reference's image"
            out.update(stage1)
        else:
            fwd = np.load(os.path.join(OUT_DIR, name + ".npz"))
            assert np.array_equal(image, fwd["image"]), name + ": the rebinding changed the reference's image"
        out.update(sc)
        out.update(opacity=np.asarray(sc["opacity"], np.float32), colors=colors.detach().numpy(), tile=np.int64(tile),
                   W=W.numpy(), image=image, grad_colors=gc, grad_opacity=go)
    else:
        com = np.load(os.path.join(OUT_DIR, "grad_" + name + ".npz"))
        for key, got in (("image", image), ("grad_colors", gc), ("grad_opacity", go), ("W", W.numpy())):
            assert np.array_equal(got, com[key]), "%s: %s differs from the committed grad_ fixture" % (name, key)
    for arr in (gp, gs, gq):
        assert np.isfinite(arr).all(), name
    path = os.path.join(OUT_DIR, "geomgrad_" + name + ".npz")
    np.savez_compressed(path, **out)
    visible = np.abs(gc).sum(1) > 0
    qdot = np.abs((sc["quaternions"].astype(np.float64) * gq).sum(1)).max()
    print("geomgrad_%s: N=%d visible=%d geometry rows non-zero=%d floored=%d clamped=%d culled=%d max|gp|=%.3g "
          "max|gs|=%.3g max|gq|=%.3g max|q.gq|=%.2g fwd=%.1fs bwd=%.1fs (%.0f KB)" % (
              name, n, int(visible.sum()), int(((np.abs(gp).sum(1) > 0) & (np.abs(gs).sum(1) > 0)).sum()),
              counts["n_floored_det"], counts["n_clamped"], counts["n_culled"], np.abs(gp).max(), np.abs(gs).max(),
              np.abs(gq).max(), qdot, t_fwd, t_bwd, os.path.getsize(path) / 1024), flush=True)


def check_branches(names=None) -> None:
    """Every branch of the table must be hit by at least one committed file of ``names`` (all scenes unless given)."""
    total = dict.fromkeys(BRANCHES, 0)
    for name in names or SCENES:
        path = os.path.join(OUT_DIR, "geomgrad_" + name + ".npz")
        if os.path.exists(path):
            z = np.load(path)
            for b in BRANCHES:
                total[b] += int(z[b])
            print("%-28s floored=%4d clamped=%4d culled=%4d" % (name, *[int(z[b]) for b in BRANCHES]))
    empty = [b for b in BRANCHES if total[b] == 0]
    if empty:
        raise SystemExit("refused: no scene of the set hits " + ", ".join(empty))


def main() -> None:
    only = sys.argv[1] if len(sys.argv) > 1 else ""
    if only != "--check":
        GaussianScene, Gaussians = _import_reference()
        import splat.gaussian_scene as ref_scene

        original_weight = ref_scene.compute_gaussian_weight
        ref_scene.compute_gaussian_weight = _weight
        for name in SCENES + [e for e in EXTRA if only and only in e]:
            if only in name:
                capture(name, GaussianScene, Gaussians, original_weight)
    if only in ("", "--check"):
        check_branches()
        check_branches(list(CAMERA_SCENES))         # the camera scenes hit every branch on their own


if __name__ == "__main__":
    main()
