"""The scenes and the committed transforms of the frame-invariance tests of scene transforms, shared by the host test that
holds the choice to its rule (tests/test_transform_seeds_host.py) and the GPU tests (tests/test_hip_transform.py).

A similarity transform leaves a frame unchanged up to rounding -- and up to the discrete decisions rounding can flip: the
edge of a tile rectangle (floor / ceil of mean +- radius), the z_view >= 0.2 cull, the order of two Gaussians whose depths
round to one float.  Which rotations flip none of them in a given scene is a property of the scene and the rule set, not of
the kernel under test, so it is decided on the CPU: SEEDS holds, for every (scene, kind), the first rotation seed (counting
from 0) for which the ORACLE'S OWN before / after pair of frames -- the C restatement of the reference on the restated
transform, no GPU code involved -- stays within the project's pixel tolerance of 1e-4 at every pixel.
"""
import numpy as np

PIXEL_TOLERANCE = 1e-4

# name -> the generator call (intro_to_gaussian_splatting_amd/synthetic.py) and the tile size; the fixtures of the same sizes
# in tests/golden (small_64x48_n300, tile12_dense_52x40_n900, trainedlike_128x128_n3000) come from the same calls
SCENES = {
    "small_64x48_n300": dict(n=300, width=64, height=48, seed=3, tile=16, trained=False),
    "dense_52x40_n900": dict(n=900, width=52, height=40, seed=61, tile=12, trained=False),
    "trainedlike_sh_128x128_n3000": dict(n=3000, width=128, height=128, seed=0, tile=16, trained=True),
}
# kind -> (s, t)
KINDS = {"rotation": (1.0, (0.0, 0.0, 0.0)), "similarity": (2.5, (1.5, -0.75, 2.0))}
# (scene, kind) -> rotation seed; chosen by the rule above (test_transform_seeds_host.py re-derives every one of them)
SEEDS = {
    ("small_64x48_n300", "rotation"): 0,                 # the oracle's own pair: 1.2e-6
    ("small_64x48_n300", "similarity"): 0,               # 1.5e-6
    ("dense_52x40_n900", "rotation"): 0,                 # 1.2e-6
    ("dense_52x40_n900", "similarity"): 0,               # 9.5e-7
    ("trainedlike_sh_128x128_n3000", "rotation"): 0,     # 6.6e-6
    ("trainedlike_sh_128x128_n3000", "similarity"): 0,   # 1.1e-5
}
CASES = sorted(SEEDS)


def scene_arrays(name):
    from intro_to_gaussian_splatting_amd.synthetic import make_scene, make_trained_like_scene

    a = SCENES[name]
    make = make_trained_like_scene if a["trained"] else make_scene
    return make(a["n"], a["width"], a["height"], seed=a["seed"])


def rotation(seed):
    """A proper rotation, uniformly distributed, from a seeded unit quaternion (the R[i][j] table of include/gsx.h)."""
    q = np.random.RandomState(20000 + seed).normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def triple(kind, seed):
    from intro_to_gaussian_splatting_amd.transform import similarity

    s, t = KINDS[kind]
    return similarity(rotation(seed), s, t)


def view_depths(points, world2view):
    """float64 z_view of every mean under the (4, 4) row-vector ``world2view``."""
    p = np.asarray(points, np.float64)
    V = np.asarray(world2view, np.float64)
    return p @ V[:3, 2] + V[3, 2]


def oracle_frame(scene, sc, arrays, tile):
    """The oracle's frame of view 1 of ``scene`` (a GaussianScene, any device: only its camera is read) over ``arrays`` =
    (points, scales, quaternions, sh or None) and the scene dict's opacity and colours: (W, H, 3) float32."""
    from oracle import c_oracle, cpu_ref

    im = scene.images[1]
    c = im.gsx_camera()
    cam = cpu_ref.Camera(im.world2view.detach().cpu().numpy(), im.full_proj_transform.cpu().numpy(), np.float32(c.tan_fovx),
                         np.float32(c.tan_fovy), np.float32(c.fx), np.float32(c.fy), c.width, c.height)
    points, scales, quats, sh = arrays
    if sh is None:
        colors = np.asarray(sc["colors_0_255"], np.float32) / np.float32(256)
    else:
        colors = cpu_ref.sh_to_rgb(points, sh, int(sc["sh_degree"]), im.camera_center_host)
    pre = c_oracle.preprocess(points, colors, scales, quats, sc["opacity"], cam)
    return c_oracle.render(pre, c.width, c.height, tile)[0]


NORMALIZE_SCENE = "small_64x48_n300"      # normalize() is tried on this scene, seen from NORMALIZE_VIEWS poses on an orbit
NORMALIZE_VIEWS = 5


def normalize_poses():
    """The extra poses of the normalize() scene: the base view is image 1, these are images 2 .. NORMALIZE_VIEWS."""
    from intro_to_gaussian_splatting_amd.synthetic import orbit_poses

    return orbit_poses(NORMALIZE_VIEWS - 1, step_deg=7.0)


def normalize_triple(scene):
    """What GaussianScene.normalize() applies, written out from cameras_extent()."""
    from intro_to_gaussian_splatting_amd.transform import similarity

    center, radius = scene.cameras_extent()
    return similarity(np.eye(3), 1.0 / radius, -center / radius)


def oracle_pair(name, kind, seed, tmp_path):
    """(before, after, depths before, depths after) of the oracle for one candidate: the restated transform
    (tests/transform_restatement.py) of the scene's arrays, the cameras moved by GaussianScene._move_views on a CPU scene.
    ``kind`` "normalize": the scene with the orbit's views and normalize()'s own triple (``seed`` is not used)."""
    import torch

    import transform_restatement as tr
    from intro_to_gaussian_splatting_amd import GaussianScene, Gaussians
    from intro_to_gaussian_splatting_amd.synthetic import write_colmap_text

    sc = scene_arrays(name)
    tile = SCENES[name]["tile"]
    write_colmap_text(str(tmp_path), sc, extra_poses=normalize_poses() if kind == "normalize" else None)
    scene = GaussianScene(str(tmp_path), Gaussians(torch.zeros(1, 3), torch.zeros(1, 3), device="cpu"))
    sh = sc.get("sh")
    degree = int(sc["sh_degree"]) if sh is not None else 0
    arrays = (sc["points"], sc["scales"], sc["quaternions"], sh)
    before = oracle_frame(scene, sc, arrays, tile)
    z0 = view_depths(sc["points"], scene.images[1].world2view.numpy())
    sim = normalize_triple(scene) if kind == "normalize" else triple(kind, seed)
    moved = tr.transform(sc["points"], sc["scales"], sc["quaternions"], sh, degree, tr.host_arguments(sim))
    scene._move_views(sim)
    after = oracle_frame(scene, sc, moved, tile)
    z1 = view_depths(moved[0], scene.images[1].world2view.numpy())
    return before, after, z0, z1
