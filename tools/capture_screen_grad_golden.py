"""Screen-space gradient fixtures: dL/d(pixel mean) of the REFERENCE ITSELF under autograd.  Data only.

Build container only; the recipe is tools/capture_geometry_grad_golden.py's (its scene set, its `_weight` rebinding of the
reference's compute_gaussian_weight, its L = sum(image * W) with W = default_rng(1000 + len(name))).  The one addition:
the scene's `preprocess` is wrapped at run time so that the PreprocessedScene the reference's render_image composites
from is kept, and torch.autograd.grad(L, [pre.points, g.points]) is asked for.  pre.points is the (m,2) tensor of pixel
means, in depth order, that render_image indexes per tile: its gradient is what the published trainer reads as
viewspace_points.grad, here in PIXEL units (the NDC convention multiplies by (width - 1) / 2 and (height - 1) / 2).

Before anything is written the tool ASSERTS that the wrap changed nothing: dL/dpoints must equal grad_points of the
committed tests/golden/geomgrad_<scene>.npz bit for bit.

    python tools/capture_screen_grad_golden.py            # all scenes
    python tools/capture_screen_grad_golden.py tile2      # only those whose name contains "tile2"

Writes tests/golden/screengrad_<scene>.npz: grad_points_xy (m,2) float32, the reference's own, and the two times.
"""
from __future__ import annotations

import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from capture_geometry_grad_golden import CAMERA_ENTRY_SCENES, CAMERA_SCENES, OWN_STAGE1, _weight  # noqa: E402
from capture_geometry_grad_golden import BAD_ROW_TWINS, reference_colors, scene_arrays  # noqa: E402
from capture_geometry_grad_golden import SCENES as GEOMETRY_SCENES  # noqa: E402
from oracle.capture_golden import FIXTURES, OUT_DIR, _generate, _import_reference  # noqa: E402

# of the scenes at the cameras of tests/camera_cases.py only the two that get camera, depth and abs fixtures as well
SCENES = [s for s in GEOMETRY_SCENES if s not in CAMERA_SCENES or s in CAMERA_ENTRY_SCENES]


def capture(name: str, GaussianScene, Gaussians) -> None:
    import torch

    from intro_to_gaussian_splatting_amd.synthetic import write_colmap_text

    sc, tile, _ = scene_arrays(name)
    with tempfile.TemporaryDirectory() as tmp:
        write_colmap_text(os.path.join(tmp, "colmap"), sc)
        g = Gaussians(torch.from_numpy(sc["points"]), torch.from_numpy(sc["colors_0_255"]), model_path=tmp)
        points = torch.from_numpy(sc["points"]).float().clone().requires_grad_(True)
        g.points = points
        g.scales = torch.from_numpy(sc["scales"]).float().clone().requires_grad_(True)
        g.quaternions = torch.from_numpy(sc["quaternions"]).float().clone().requires_grad_(True)
        g.colors = reference_colors(sc, g).requires_grad_(True)
        g.opacity = torch.from_numpy(np.ascontiguousarray(sc["opacity"], dtype=np.float32)).clone().requires_grad_(True)
        scene = GaussianScene(os.path.join(tmp, "colmap"), g)
        kept = []
        preprocess = scene.preprocess

        def keeping(image_idx):
            kept.append(preprocess(image_idx))
            return kept[-1]

        scene.preprocess = keeping
        t0 = time.time()
        image = scene.render_image(1, tile_size=tile)
        t_fwd = time.time() - t0
        assert len(kept) == 1, name + ": render_image preprocessed %d times" % len(kept)
        pre = kept[0]
        W = torch.from_numpy(np.random.default_rng(1000 + len(name)).standard_normal(tuple(image.shape)).astype(np.float32))
        loss = (image * W).sum()
        t0 = time.time()
        g_xy, g_points = torch.autograd.grad(loss, [pre.points, points])
        t_bwd = time.time() - t0
    g_xy, g_points = g_xy.numpy(), g_points.numpy()
    com = np.load(os.path.join(OUT_DIR, "geomgrad_" + name + ".npz"))
    assert np.array_equal(g_points.view(np.uint32), com["grad_points"].view(np.uint32)), \
        name + ": grad_points differs from the committed geomgrad_ fixture"
    assert g_xy.dtype == np.float32 and g_xy.ndim == 2 and g_xy.shape[1] == 2 and np.isfinite(g_xy).all(), name
    path = os.path.join(OUT_DIR, "screengrad_" + name + ".npz")
    np.savez_compressed(path, grad_points_xy=g_xy, reference_forward_seconds=np.float64(t_fwd),
                        reference_backward_seconds=np.float64(t_bwd))
    print("screengrad_%s: m=%d non-zero rows=%d max|g|=%.3g fwd=%.1fs bwd=%.1fs (%.1f KB)" % (
        name, g_xy.shape[0], int((np.abs(g_xy).sum(1) > 0).sum()), np.abs(g_xy).max(), t_fwd, t_bwd,
        os.path.getsize(path) / 1024), flush=True)


def main() -> None:
    only = sys.argv[1] if len(sys.argv) > 1 else ""
    GaussianScene, Gaussians = _import_reference()
    import splat.gaussian_scene as ref_scene

    ref_scene.compute_gaussian_weight = _weight
    for name in SCENES:
        if only in name:
            capture(name, GaussianScene, Gaussians)


if __name__ == "__main__":
    main()
