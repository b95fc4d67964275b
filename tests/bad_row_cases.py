"""Scenes with non-finite and degenerate rows, shared by the host tests (tests/test_bad_rows_host.py) and the GPU tests
(tests/test_hip_bad_rows.py).  No tests inside.

A fit does not stay made of healthy rows: one bad Adam step, a log-space scale that underflows to 0, a quaternion that
collapses to 0, a logit driven to +-80.  Every base scene here gets such rows written IN PLACE at fixed indices (n and every
other row's index stay what they were; rows 255 and 256 straddle a 256-row block), and comes with its CLEAN TWIN: the same
arrays with every UNLISTED row replaced by a plainly culled finite row (a point 1.0 behind the camera along its view axis,
unit scales, identity quaternion).  The frame's tile lists of a scene and of its twin are the same lists, so every output of
every entry must carry the same bits in both, in all rows but the replaced ones.

UNLISTED   the frame lists the row on no tile (what stage 1 does with each kind is in docs/lab_notes/bad_rows.md):
    nan_point      one NaN coordinate                          inf_pos / inf_neg   one +Inf / one -Inf coordinate
    nan_scale      one NaN scale                               nan_quat            one NaN quaternion component
    zero_quat      the all-zero quaternion                     huge_quat           components 3e19: the squared norm overflows
  on SH scenes also
    nan_coeff      a row behind the camera with a NaN coefficient
    at_centre      a mean that is the view's float32 camera centre to the bit (the view direction is 0 / 0)
  zero_quat and huge_quat are UNLISTED under the ref_cpu rule set only: the reference normalises a quaternion twice
  (F.normalize, then build_rotation's own division, splat/gaussians.py:54-69, splat/utils.py:132-155), which makes 0 / 0 of
  both.  The std_3dgs rule set normalises once: both become the zero quaternion, whose rotation is the identity -- a finite,
  listed row (the published rule; csrc/gsx_project.hip covariance3d, oracle/std3dgs_ref.py).  The std cases therefore carry
  the other five kinds only.
DEGENERATE finite, listed, with a well-defined gradient:
    zero_scales    all three scales 0 (the determinant floor)  flat_disc           one scale 0
    logit_hi / logit_lo   logit +80 / -80 (float32 sigmoid exactly 1 / exactly 0)
    colour_zero / colour_four   a colour of 0 / of 4.0
    quat_tiny / quat_huge   the row's quaternion times 1e-18 / 1e18: both normalise to finite values
"""
import functools

import numpy as np

import camera_cases as cc
from intro_to_gaussian_splatting_amd.synthetic import TREEHILL_QVEC, TREEHILL_TVEC, make_scene, make_trained_like_scene

N, WIDTH, HEIGHT, TILE = 300, 64, 48, 16
f32 = np.float32

# kind -> row.  0, 1, 63, 64, 127, 128, 255, 256, 299: the ends of the array, of a wavefront, of a 128-row and a 256-row block.
UNLISTED = {"nan_point": 0, "inf_pos": 64, "inf_neg": 191, "nan_scale": 127, "nan_quat": 255, "zero_quat": 256, "huge_quat": 299}
UNLISTED_STD = {k: v for k, v in UNLISTED.items() if k not in ("zero_quat", "huge_quat")}
UNLISTED_SH = dict(UNLISTED, nan_coeff=1, at_centre=128)
UNLISTED_SH_STD = dict(UNLISTED_STD, nan_coeff=1, at_centre=128)
DEGENERATE = {"zero_scales": 63, "flat_disc": 100, "logit_hi": 150, "logit_lo": 200, "colour_zero": 30, "colour_four": 31,
              "quat_tiny": 220, "quat_huge": 280}

# case -> (camera of camera_cases.CAMERAS or None for the Treehill camera of every older fixture, seed).  The seeds are
# chosen so that every DEGENERATE row is listed and the conditions of tests/test_bad_rows_host.py hold.
RGB_CASES = {"base": (None, 26), "roll": ("roll", 63)}
# (camera, seed, active degree, the UNLISTED kinds); sh3_std is the SH scene of the std_3dgs fit
SH_CASES = {"sh3": ("farpose", 19, 3, UNLISTED_SH), "sh3_active1": ("farpose", 19, 1, UNLISTED_SH),
            "sh3_std": ("farpose", 19, 3, UNLISTED_SH_STD)}
SH_REF_CPU = ("sh3", "sh3_active1")
STD_CASES = {"std_base": (None, 26), "std_roll": ("roll", 63)}                     # each plain and anti-aliased, over cc.STD_BG
ARRAYS = ("points", "scales", "quaternions", "opacity", "colors")


def camera_of(name):
    if name is None:
        return dict(width=WIDTH, height=HEIGHT, fx=0.75 * WIDTH, fy=0.75 * WIDTH, qvec=TREEHILL_QVEC, tvec=TREEHILL_TVEC)
    return cc.CAMERAS[name]


def behind(camera, depth=1.0):
    """The world point `depth` behind the camera centre along its view axis (float32)."""
    c = camera_of(camera)
    R, t = cc.rotation(c["qvec"]), np.asarray(c["tvec"], np.float64)
    return (R.T @ (np.array([0.0, 0.0, -depth]) - t)).astype(f32)


def camera_centre(sc):
    """The view's float32 ``camera_center_host`` as the scene object derives it (a GaussianImage built on the CPU), which is
    what the SH kernels subtract from a mean."""
    from intro_to_gaussian_splatting_amd import GaussianImage
    from intro_to_gaussian_splatting_amd.colmap import Camera, Image

    im = GaussianImage(Camera(1, "PINHOLE", int(sc["width"]), int(sc["height"]),
                              np.array([sc["fx"], sc["fy"], sc["cx"], sc["cy"]], np.float64)),
                       Image(1, np.asarray(sc["qvec"]), np.asarray(sc["tvec"]), 1, "v"), device="cpu")
    return np.asarray(im.camera_center_host, f32)


def _write_degenerate(sc):
    p, s, q, o, c = (sc[k] for k in ARRAYS)
    s[DEGENERATE["zero_scales"]] = 0.0
    s[DEGENERATE["flat_disc"], 1] = 0.0
    o[DEGENERATE["logit_hi"]] = 80.0
    o[DEGENERATE["logit_lo"]] = -80.0
    c[DEGENERATE["colour_zero"]] = 0.0
    c[DEGENERATE["colour_four"]] = 4.0
    q[DEGENERATE["quat_tiny"]] *= f32(1e-18)
    q[DEGENERATE["quat_huge"]] *= f32(1e18)


def _write_unlisted(sc, kinds, camera):
    p, s, q = sc["points"], sc["scales"], sc["quaternions"]
    for kind, i in kinds.items():
        if kind == "nan_point":
            p[i, 1] = np.nan
        elif kind == "inf_pos":
            p[i, 0] = np.inf
        elif kind == "inf_neg":
            p[i, 2] = -np.inf
        elif kind == "nan_scale":
            s[i, 2] = np.nan
        elif kind == "nan_quat":
            q[i, 1] = np.nan
        elif kind == "zero_quat":
            q[i] = 0.0
        elif kind == "huge_quat":
            q[i] = f32(3e19) * np.sign(q[i] + (q[i] == 0))
        elif kind == "nan_coeff":
            p[i] = behind(camera, 2.5)
            sc["sh"][i, 2, 1] = np.nan          # band 1: read at every active degree >= 1
        elif kind == "at_centre":
            p[i] = camera_centre(sc)
        else:
            raise KeyError(kind)


def _twin(sc, kinds, camera):
    out = {k: (v.copy() if isinstance(v, np.ndarray) and v.ndim else v) for k, v in sc.items()}
    for i in kinds.values():
        out["points"][i] = behind(camera)
        out["scales"][i] = 1.0
        out["quaternions"][i] = (1.0, 0.0, 0.0, 0.0)
        if "sh" in out:
            out["sh"][i] = np.where(np.isfinite(out["sh"][i]), out["sh"][i], f32(0.0))
    return out


def _finish(sc, kinds, camera):
    """(bad scene, clean twin, the UNLISTED kinds' rows) of a base scene dict; `colors` is what Gaussians.from_arrays makes
    of colors_0_255, overwritten for the two colour kinds (the tests hand it to the scene as the colour array)."""
    sc = dict(sc)
    sc["colors"] = (sc["colors_0_255"] / f32(256.0)).astype(f32)
    for k in ARRAYS + (("sh",) if "sh" in sc else ()):
        sc[k] = np.array(sc[k], f32)
    _write_degenerate(sc)
    _write_unlisted(sc, kinds, camera)
    return sc, _twin(sc, kinds, camera), dict(kinds)


@functools.lru_cache(maxsize=None)
def rgb_case(name):
    camera, seed = RGB_CASES[name]
    c = camera_of(camera)
    base = make_scene(n=N, seed=seed, behind_fraction=0.1, **c)
    return _finish(base, UNLISTED, camera)


@functools.lru_cache(maxsize=None)
def std_case(name):
    camera, seed = STD_CASES[name]
    base = make_scene(n=N, seed=seed, behind_fraction=0.1, **camera_of(camera))
    return _finish(base, UNLISTED_STD, camera)


@functools.lru_cache(maxsize=None)
def sh_case(name):
    """(bad, twin, rows, stored degree 3, active degree)."""
    camera, seed, active, kinds = SH_CASES[name]
    base = cc.scene(camera, N, seed, make=make_trained_like_scene, sh_degree=3)
    return _finish(base, kinds, camera) + (3, active)


def replaced(rows, n=N):
    """Boolean mask of the rows the twin replaces."""
    m = np.zeros(n, bool)
    m[list(rows.values())] = True
    return m
