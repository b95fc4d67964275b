"""The host side of scene transforms (intro_to_gaussian_splatting_amd/transform.py), the argument checks of
gsx_transform_gaussians and the numpy restatement of its kernel (tests/transform_restatement.py).  No GPU.

The SH rotation matrices are held to their defining property, Y_l(R d)^T M_l c = Y_l(d)^T c, against the basis the tests
already have (tests/sh_backward_restatement.py).  That basis carries the float32 constants the kernels hold, each a factor
kappa_k = float32(C) / C, |kappa_k - 1| <= 2^-24, away from the orthonormal function; an ORTHOGONAL M_l (asked for to
1e-12) belongs to the orthonormal functions.  So the property is asserted twice: to 1e-12 against the basis with every
column divided by its kappa_k, and against the basis as the kernels hold it to 2 x 2^-24 sum_k |Y_k| |c_k| -- the two
constants a matrix entry connects are each off by at most 2^-24.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import sh_backward_restatement as sr
import transform_restatement as tr
from conftest import GOLDEN_DIR

from intro_to_gaussian_splatting_amd import transform as T

SEEDS = [0, 1, 2, 3, 4]
# csrc/gsx_sh_device.h as written there (double literals), one per basis function k = 0..15
EXACT = [0.28209479177387814, -0.4886025119029199, 0.4886025119029199, -0.4886025119029199,
         1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396,
         -0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435]
KAPPA = np.array([float(np.float32(c)) / c for c in EXACT])


def rotation(seed):
    """A proper rotation from a seeded unit quaternion (the R[i][j] table of include/gsx.h), and the quaternion."""
    q = np.random.RandomState(1000 + seed).normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return R, q


def block_diagonal(R):
    M = np.eye(16)
    for l, Ml in zip((1, 2, 3), T.sh_rotation_matrices(R)):
        M[l * l:(l + 1) ** 2, l * l:(l + 1) ** 2] = Ml
    return M


@pytest.mark.parametrize("seed", SEEDS)
def test_sh_rotation_matrices_are_orthogonal_and_a_representation(seed):
    R1, _ = rotation(seed)
    R2, _ = rotation(seed + 50)
    for l, (M, A, B, I) in enumerate(zip(T.sh_rotation_matrices(R1 @ R2), T.sh_rotation_matrices(R1),
                                          T.sh_rotation_matrices(R2), T.sh_rotation_matrices(np.eye(3))), start=1):
        assert A.shape == (2 * l + 1, 2 * l + 1) and A.dtype == np.float64
        assert np.abs(A @ A.T - np.eye(2 * l + 1)).max() <= 1e-12
        assert np.abs(I - np.eye(2 * l + 1)).max() <= 1e-12
        assert np.abs(M - A @ B).max() <= 1e-12


@pytest.mark.parametrize("seed", SEEDS)
def test_sh_rotation_matrices_have_the_defining_property(seed):
    R, _ = rotation(seed)
    rs = np.random.RandomState(seed)
    d = rs.normal(size=(1000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = rs.normal(size=(1000, 16))
    M = block_diagonal(R)
    rd = d @ R.T
    rotated = c @ M.T                                   # M c per direction
    # the orthonormal functions: the tests' basis with the float32 rounding of its constants divided out
    Y, Yr = sr.basis(d, 3) / KAPPA[None, :], sr.basis(rd, 3) / KAPPA[None, :]
    worst = np.abs((Yr * rotated).sum(1) - (Y * c).sum(1)).max()
    print("seed %d: max residual against the orthonormal basis %.3g" % (seed, worst))
    assert worst <= 1e-12
    # the basis as the kernels hold it
    Y, Yr = sr.basis(d, 3), sr.basis(rd, 3)
    residual = np.abs((Yr * rotated).sum(1) - (Y * c).sum(1))
    bound = 2.0 * 2.0 ** -24 * (np.abs(Yr) * np.abs(rotated)).sum(1)
    print("seed %d: max residual / bound against the kernels' basis %.3g" % (seed, (residual / bound).max()))
    assert (residual <= bound).all()


def test_similarity_validates_and_refuses():
    R, q = rotation(7)
    sim = T.similarity(R, 2.5, [1.0, -2.0, 3.0])
    assert isinstance(sim, tuple) and len(sim) == 3
    Rb, s, t = sim
    assert np.array_equal(Rb, R) and s == 2.5 and np.array_equal(t, [1.0, -2.0, 3.0])
    assert np.array_equal(T.similarity(R).t, np.zeros(3)) and T.similarity(R).s == 1.0
    assert np.array_equal(T.similarity(R, 1.0, None).t, np.zeros(3))
    bad = R.copy()
    bad[0, 0] += 1e-5
    flip = R.copy()
    flip[:, 0] = -flip[:, 0]
    nan = R.copy()
    nan[1, 1] = np.nan
    for args, word in (((bad,), "orthonormal"), ((flip,), "reflection"), ((nan,), "finite"), ((R, 0.0), "positive"),
                       ((R, -1.0), "positive"), ((R, np.inf), "finite"), ((R, np.nan), "finite"),
                       ((R, 1.0, [0.0, np.inf, 0.0]), "finite"), ((R, 1.0, [0.0, 1.0]), "3 numbers"),
                       ((np.eye(4),), "3 x 3")):
        with pytest.raises(ValueError, match=word):
            T.similarity(*args)
    within = R.copy()
    within[0, 0] += 2e-7            # a float32 rotation matrix is orthonormal to ~1e-7: accepted
    T.similarity(within)


@pytest.mark.parametrize("seed", SEEDS + [100, 101, 102, 103])
def test_the_quaternion_is_the_rotations_with_w_not_negative(seed):
    if seed >= 100:                 # half turns about an axis: w = 0, where the trace formula alone would lose everything
        axis = np.eye(3)[(seed - 100) % 3] if seed < 103 else np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
        R = 2.0 * np.outer(axis, axis) - np.eye(3)
    else:
        R, _ = rotation(seed)
    q = T.similarity(R).q
    assert q.shape == (4,) and q[0] >= 0.0 and abs(np.linalg.norm(q) - 1.0) <= 1e-15
    w, x, y, z = q
    back = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    assert np.abs(back - R).max() <= 1e-14


def test_compose_and_inverse():
    a = T.similarity(rotation(1)[0], 2.5, [1.0, -2.0, 3.0])
    b = T.similarity(rotation(2)[0], 0.3, [-4.0, 0.5, 0.25])
    x = np.random.RandomState(0).normal(size=(50, 3))
    ab = T.compose(a, b)
    assert np.abs(ab.apply(x) - a.apply(b.apply(x))).max() <= 1e-13
    assert np.abs(ab.R @ ab.R.T - np.eye(3)).max() <= 1e-14
    inv = T.inverse(a)
    assert np.abs(inv.apply(a.apply(x)) - x).max() <= 1e-13 and np.abs(a.apply(inv.apply(x)) - x).max() <= 1e-13
    ident = T.compose(inv, a)
    assert np.abs(ident.R - np.eye(3)).max() <= 1e-14 and abs(ident.s - 1.0) <= 1e-15 and np.abs(ident.t).max() <= 1e-14
    assert T.inverse((a.R, a.s, a.t)).s == inv.s           # plain tuples are taken too
    with pytest.raises(ValueError):
        T.inverse((a.R, -1.0, a.t))


def _fixture_poses():
    g = np.load(os.path.join(GOLDEN_DIR, "colmap_model.npz"))
    return [(g["txt_img%d_qvec" % i].astype(np.float64), g["txt_img%d_tvec" % i].astype(np.float64)) for i in g["txt_image_ids"]]


def _cpu_scene(tmp_path, poses, n=4):
    from intro_to_gaussian_splatting_amd import GaussianScene, Gaussians
    from intro_to_gaussian_splatting_amd.synthetic import write_colmap_text

    sc = dict(width=64, height=48, fx=48.0, fy=48.0, cx=32.0, cy=24.0, qvec=poses[0][0], tvec=poses[0][1])
    write_colmap_text(str(tmp_path), sc, extra_poses=poses[1:])
    return GaussianScene(str(tmp_path), Gaussians(torch.zeros(n, 3), torch.zeros(n, 3), device="cpu"))


def test_cameras_extent_on_the_colmap_fixture(tmp_path):
    """The poses of tests/golden/colmap_model (its four images, whose cameras are not all PINHOLE, under one PINHOLE camera):
    centre_i = -R_i^T t_i, the mean of the centres, 1.1 x the largest distance to it -- written out in float64.  The scene's
    centres come from a float32 matrix inverse: 1e-5 of the extent."""
    from intro_to_gaussian_splatting_amd.synthetic import _rotation

    poses = _fixture_poses()
    assert len(poses) == 4
    scene = _cpu_scene(tmp_path, poses)
    centers = np.array([-_rotation(q).T @ t for q, t in poses])
    mean = centers.mean(axis=0)
    radius = 1.1 * max(float(np.linalg.norm(c - mean)) for c in centers)
    center, r = scene.cameras_extent()
    assert center.shape == (3,) and center.dtype == np.float64 and isinstance(r, float) and radius > 0
    assert np.abs(center - mean).max() <= 1e-5 * radius and abs(r - radius) <= 1e-5 * radius


def test_views_follow_the_world_and_view_space_scales_by_s(tmp_path):
    """GaussianScene._move_views, the host half of GaussianScene.transform: for every view and any world point,
    view(x') = s view(x); the new pose is rigid (orthonormal rotation, last column (0, 0, 0, 1)); the camera centre is the
    transformed centre."""
    scene = _cpu_scene(tmp_path, _fixture_poses())
    sim = T.similarity(rotation(3)[0], 2.5, [0.5, -1.5, 2.0])
    x = np.random.RandomState(1).normal(size=(20, 3)) * 3.0
    before = {i: (im.world2view.numpy().astype(np.float64), np.array(im.camera_center_host)) for i, im in scene.images.items()}
    versions = {i: im.pose_version for i, im in scene.images.items()}
    scene._move_views(sim)
    hom = lambda p: np.concatenate([p, np.ones((len(p), 1))], axis=1)  # noqa: E731
    for i, im in scene.images.items():
        V0, c0 = before[i]
        V1 = im.world2view.numpy().astype(np.float64)
        assert im.pose_version == versions[i] + 1
        assert np.array_equal(V1[:, 3], [0.0, 0.0, 0.0, 1.0])
        assert np.abs(V1[:3, :3] @ V1[:3, :3].T - np.eye(3)).max() <= 5e-7
        scale = np.abs(hom(x) @ V0).max() * sim.s
        assert np.abs(hom(sim.apply(x)) @ V1 - sim.s * (hom(x) @ V0))[:, :3].max() <= 1e-6 * scale
        assert np.abs(np.array(im.camera_center_host) - sim.apply(c0)).max() <= 1e-5 * np.abs(sim.apply(c0)).max()


def test_the_restatement_is_the_transform():
    """tests/transform_restatement.py against float64: the means move by the similarity, the scales by s, the rotation of
    q' is R times the rotation of q and |q'| = |q|, and the rotated coefficients give the old colour along the rotated
    direction -- all to float32 rounding of values of the size involved."""
    rs = np.random.RandomState(5)
    n = 300
    p = rs.normal(size=(n, 3)).astype(np.float32) * 4
    c = np.exp(rs.normal(size=(n, 3))).astype(np.float32)
    q = rs.normal(size=(n, 4)).astype(np.float32)
    sh = rs.normal(size=(n, 16, 3)).astype(np.float32)
    sim = T.similarity(rotation(4)[0], 2.5, [1.0, -2.0, 3.0])
    a = tr.host_arguments(sim)
    assert all(v.dtype == np.float32 for v in a.values())
    P, C, Q, S = tr.transform(p, c, q, sh, 3, a)
    assert np.abs(P - sim.apply(p)).max() <= 4e-7 * np.abs(sim.apply(p)).max()
    assert np.array_equal(C, np.float32(2.5) * c)
    from oracle.cpu_ref import rotation_from_quaternion

    Rq, Rq2 = rotation_from_quaternion(q).astype(np.float64), rotation_from_quaternion(Q).astype(np.float64)
    assert np.abs(Rq2 - sim.R[None] @ Rq).max() <= 2e-6
    assert np.abs(np.linalg.norm(Q, axis=1) / np.linalg.norm(q, axis=1) - 1.0).max() <= 1e-6
    assert np.array_equal(S[:, 0], sh[:, 0])
    center = np.array([0.3, -0.2, 0.1])
    before = sr.forward(p, sh, 3, center)[0]
    after = sr.forward(sim.apply(p), S, 3, sim.apply(center))[0]
    assert np.abs(after - before).max() <= 2e-6 * np.abs(sh).sum(axis=1).max()
    # lower stored degrees rotate the same bands; an RGB container has no coefficients
    for degree in (0, 1, 2):
        k = (degree + 1) ** 2
        Sd = tr.transform(p, c, q, sh[:, :k], degree, a)[3]
        assert np.array_equal(Sd, S[:, :k])
    assert tr.transform(p, c, q, None, 0, a)[3] is None
    # a tail of zeros stays zero, of either sign
    z = sh.copy()
    z[:, 4:] = 0.0
    z[::2, 9:] = -0.0
    Z = tr.transform(p, c, q, z, 3, a)[3]
    assert not Z[:, 4:].any() and np.array_equal(Z[:, :4], S[:, :4])


def _struct(sim):
    from intro_to_gaussian_splatting_amd import _ffi

    a = tr.host_arguments(sim)
    t = _ffi.GsxTransform()
    t.R[:] = a["R"].reshape(-1).tolist()
    t.s = float(a["s"])
    t.t[:] = a["t"].tolist()
    t.q_R[:] = a["q"].tolist()
    for name in ("M1", "M2", "M3"):
        getattr(t, name)[:] = a[name].reshape(-1).tolist()
    return t


def test_argument_errors_need_no_gpu():
    """Every refusal of gsx_transform_gaussians comes before any HIP call: this runs on a machine without a GPU, with
    pointers that are never followed."""
    from intro_to_gaussian_splatting_amd import _ffi

    lib = _ffi.load()
    assert ctypes.sizeof(_ffi.GsxTransform) == 400
    sim = T.similarity(rotation(0)[0], 2.0, [1.0, 2.0, 3.0])
    ptr = ctypes.c_void_p(4096)

    def call(points=ptr, scales=ptr, quats=ptr, sh=ptr, degree=3, n=10, t=None, edit=None):
        t = _struct(sim) if t is None else t
        if edit:
            edit(t)
        return lib.gsx_transform_gaussians(points, scales, quats, sh, degree, n, ctypes.byref(t), None)

    def refused(word, **kw):
        assert call(**kw) == _ffi.GSX_ERR_INVALID_ARGUMENT
        assert word in lib.gsx_last_error(), lib.gsx_last_error()

    refused(b"n = -1", n=-1)
    refused(b"sh_degree", degree=4)
    refused(b"sh_degree", degree=-1)
    refused(b"points", points=None)
    refused(b"scales", scales=None)
    refused(b"quaternions", quats=None)
    refused(b"sh is NULL", sh=None)
    assert lib.gsx_transform_gaussians(ptr, ptr, ptr, ptr, 3, 10, None, None) == _ffi.GSX_ERR_INVALID_ARGUMENT
    assert b"transform is NULL" in lib.gsx_last_error()

    def setter(field, index, value):
        def edit(t):
            if field == "s":
                t.s = value
            else:
                getattr(t, field)[index] = value
        return edit

    for field, index in (("R", 4), ("s", 0), ("t", 2), ("q_R", 3), ("M1", 8), ("M2", 24), ("M3", 48)):
        for value in (float("nan"), float("inf"), float("-inf")):
            refused(("transform->%s[%d]" % (field, index)).encode(), edit=setter(field, index, value))
    refused(b"not positive", edit=setter("s", 0, 0.0))
    refused(b"not positive", edit=setter("s", 0, -2.0))
    # n == 0 is GSX_OK whatever the pointers are; an invalid transform is refused even then
    assert call(points=None, scales=None, quats=None, sh=None, n=0) == _ffi.GSX_OK
    refused(b"not positive", n=0, edit=setter("s", 0, 0.0))


def test_a_cpu_container_is_refused_in_the_words_of_the_other_kernels():
    from intro_to_gaussian_splatting_amd import Gaussians

    g = Gaussians(torch.zeros(4, 3), torch.zeros(4, 3), device="cpu")
    with pytest.raises(ValueError, match="runs only as a HIP kernel on an AMD GPU .*no CPU fallback"):
        g.transform(np.eye(3))
    with pytest.raises(ValueError, match="reflection"):          # the triple is validated first
        g.transform(np.diag([1.0, 1.0, -1.0]))
