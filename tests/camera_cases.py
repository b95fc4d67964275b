"""The cameras of the gradient tests away from the one camera family the other fixtures see (fx = fy = 0.75 width, the
Treehill pose), shared by the host tests (tests/test_camera_cases_host.py) and the GPU tests
(tests/test_hip_camera_cases.py).

What the set must keep, whatever its values become (the host test asserts it): fx / fy <= 2/3 in one camera and >= 3/2 in
another; one rotation of at least 120 degrees about an axis more than 20 degrees from every coordinate axis; one camera
with R00 < 0 and R11 < 0.  The principal point is the frame centre in all of them: the render path reads none (like the
reference), which the host and GPU tests hold with OFF_CENTRE.
"""
import numpy as np

from intro_to_gaussian_splatting_amd.synthetic import TREEHILL_QVEC, TREEHILL_TVEC

# name -> frame, focal lengths in pixels, COLMAP pose (qvec w x y z, tvec)
CAMERAS = {
    # fx against fy alone: the pose of every other gradient fixture
    "aniso": dict(width=64, height=48, fx=40.0, fy=62.0, qvec=TREEHILL_QVEC, tvec=TREEHILL_TVEC),
    # fx > fy with a wide vertical field (tan_fovy = 32 / 30 > 1), the pose of pose_70x50_n250
    "aniso_tall": dict(width=48, height=64, fx=70.0, fy=30.0, qvec=(0.8, 0.3, -0.45, 0.25), tvec=(-0.7, 0.2, 2.1)),
    # the contractions with world2view alone: about 140 degrees about an oblique axis, fx = fy
    "farpose": dict(width=64, height=48, fx=48.0, fy=48.0, qvec=(0.35, 0.6, -0.55, 0.46), tvec=(0.4, -0.9, 1.5)),
    # both at once: about 174 degrees about z, so R00 and R11 are negative
    "roll": dict(width=64, height=48, fx=36.0, fy=52.0, qvec=(0.05, 0.1, -0.08, 0.99), tvec=(-0.3, 0.5, 2.0)),
}
NAMES = tuple(CAMERAS)
ANISOTROPIC = tuple(k for k, c in CAMERAS.items() if c["fx"] != c["fy"])
TILE = 16

# camera -> the scene of its fixtures tests/golden/{geomgrad,camgrad,depthgrad,screengrad,absgrad}_<scene>.npz; the generator
# arguments are tools/capture_geometry_grad_golden.py's CAMERA_SCENES (the files carry them: qvec, tvec, fx, fy, width, height)
FIXTURES = {"aniso": "cam_aniso_64x48_n120", "aniso_tall": "cam_aniso_tall_48x64_n100",
            "farpose": "cam_farpose_64x48_n120", "roll": "cam_roll_64x48_n100"}
# the cameras whose scene also has camera, depth, screen and abs fixtures
ENTRY_CAMERAS = ("aniso_tall", "roll")

# a principal point off the frame centre, as a real COLMAP camera has one (pixels added to cx, cy)
OFF_CENTRE = (5.25, -3.5)

# The std_3dgs rule set at these cameras (tests/test_std3dgs_camera_cases_host.py, tests/test_hip_camera_cases.py):
# name -> (camera, n, seed, make_scene keywords); every case at TILE over STD_BG, built with scene(camera, n, seed, **kw).
# The first four carry culled rows; the two off-axis ones put centres up to 1.8 frustum half-widths off axis with
# footprints that reach back into the frame, so the EWA clamp's gradient branch runs with limx != limy and fx != fy
# (seeds 21 and 22 each give Gaussians clamped in x alone and in y alone that carry gradient: the host test asserts it).
STD_BG = (0.25, 0.5, 0.75)
STD_CAMERA_CASES = {
    "std_aniso_64x48_n120": ("aniso", 120, 11, dict(behind_fraction=0.1)),
    "std_aniso_tall_48x64_n100": ("aniso_tall", 100, 12, dict(behind_fraction=0.1)),
    "std_farpose_64x48_n120": ("farpose", 120, 13, dict(behind_fraction=0.1)),
    "std_roll_64x48_n100": ("roll", 100, 14, dict(behind_fraction=0.1)),
    "std_offaxis_aniso_tall_48x64_n100": ("aniso_tall", 100, 21, dict(spread=1.8, sigma_scale=3.0)),
    "std_offaxis_roll_64x48_n100": ("roll", 100, 22, dict(spread=1.8, sigma_scale=3.0)),
}
STD_OFFAXIS = tuple(k for k in STD_CAMERA_CASES if "offaxis" in k)


def rotation(qvec):
    """R of a COLMAP qvec (camera = R world + t)."""
    from intro_to_gaussian_splatting_amd.synthetic import _rotation

    return _rotation(qvec)


def angle_and_axis(qvec):
    """(degrees in [0, 180], unit axis) of the rotation of ``qvec``."""
    q = np.asarray(qvec, np.float64)
    q = q / np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    s = np.linalg.norm(q[1:])
    return float(np.degrees(2 * np.arctan2(s, q[0]))), q[1:] / s


def scene(name, n, seed, make=None, **kw):
    """A synthetic scene in camera ``name``'s own frustum: ``make`` (make_scene unless given) with the camera's keywords."""
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    return (make or make_scene)(n=n, seed=seed, **CAMERAS[name], **kw)


def off_centre(sc):
    """The scene dict with its principal point moved by OFF_CENTRE."""
    out = dict(sc)
    out["cx"] = np.float64(float(sc["cx"]) + OFF_CENTRE[0])
    out["cy"] = np.float64(float(sc["cy"]) + OFF_CENTRE[1])
    return out
