"""Scale initialisation without a GPU: the header and the binding, every refusal of gsx_knn3 by name (before any HIP call), the
Python surface's ValueErrors, and the float32 restatement (tests/knn_restatement.py) against the reference's own results
(tests/golden/knn_*.npz, tools/capture_knn_golden.py) and against a float64 brute force.

The bars are derived, against exact arithmetic on the float32 inputs (eps = 2^-24, relative):
a distance carries <= 3.5 eps -- the difference eps, the square eps, two sums eps each, half of these four through the root
(2 eps), the root's own half eps rounded up to a whole one, and half an eps for the second order; the mean of three carries
<= 3 eps more (two sums and the divide), and the product with the old scale eps.  Each of two float32 computations is
therefore within 8 eps of the exact value, and the two within 16 eps ~ 9.5e-7 of each other: the bar of the restatement
against the reference (whose torch.linalg.norm sums in another order: not bit for bit).  Against float64: 4 eps for a distance,
8 eps for a scale.  Distances of the fixtures' clouds are far above the square root of the smallest normal float32, so no
square underflows; a duplicate's distance is 0 in every arithmetic.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

import knn_restatement as kr

EPS = 2.0 ** -24
F = np.float32


def _golden(kind, n):
    return np.load(os.path.join(GOLDEN_DIR, kr.fixture_name(kind, n) + ".npz"))


def _close(a, b, rel):
    """|a - b| <= rel * |b| elementwise, with equal infinities equal."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    same_inf = np.isinf(a) & np.isinf(b) & (a == b)
    with np.errstate(invalid="ignore"):
        ok = np.abs(a - b) <= rel * np.abs(b)
    return bool((ok | same_inf).all())


# ---- C ABI
def test_header_declares_both_symbols_and_the_binding_matches():
    from intro_to_gaussian_splatting_amd import _ffi
    import test_cabi

    hdr = open(os.path.join(ROOT, "include", "gsx.h")).read()
    declared = test_cabi._declared_functions()
    for name, n_args in (("gsx_knn3_workspace_bytes", 1), ("gsx_knn3", 10)):
        assert re.search(r"GSX_API\s+\w+\s+%s\(" % name, hdr) and name in declared, name
        assert len(_ffi.SIGNATURES[name][1]) == n_args, name
        assert hasattr(_ffi.load(), name)
    assert _ffi.SIGNATURES["gsx_knn3"][0] is ctypes.c_int and _ffi.SIGNATURES["gsx_knn3_workspace_bytes"][0] is ctypes.c_size_t
    for name in ("GSX_KNN_RULE_REFERENCE", "GSX_KNN_RULE_PUBLISHED"):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(_ffi, name), name
    assert (kr.REFERENCE, kr.PUBLISHED) == (_ffi.GSX_KNN_RULE_REFERENCE, _ffi.GSX_KNN_RULE_PUBLISHED)


def test_workspace_bytes_is_monotone_and_zero_on_bad_arguments():
    from intro_to_gaussian_splatting_amd import _ffi

    f = _ffi.load().gsx_knn3_workspace_bytes
    sizes = [f(n) for n in (0, 1, 255, 256, 257, 8195, 10 ** 6, 2 ** 30)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[-1] >= 16 * 2 ** 30 and f(10 ** 6) >= 16 * 10 ** 6 + 32 * 3907          # an entry per row, a box per block
    assert f(10 ** 6) <= 17 * 10 ** 6
    assert f(-1) == 0 and f(2 ** 30 + 1) == 0 and f(-2 ** 40) == 0


WS, PTR = 1 << 20, 4096           # a 256-byte aligned "workspace" and "arrays": never dereferenced


def test_refusals_name_the_argument_and_need_no_gpu():
    from intro_to_gaussian_splatting_amd import _ffi

    lib = _ffi.load()
    big = lib.gsx_knn3_workspace_bytes(100)
    counted = ctypes.c_int64(77)

    def knn(points=PTR, n=100, order=None, rule=0, dist3=PTR * 2, scale=PTR * 3, candidates=None, ws=WS, ws_bytes=big):
        return lib.gsx_knn3(points, n, order, rule, dist3, scale, candidates, ws, ws_bytes, None)

    for kw, word in ((dict(points=None), b"points is NULL"), (dict(dist3=None, scale=None), b"dist3 and scale are both NULL"),
                     (dict(n=-1), b"n = -1"), (dict(n=2 ** 30 + 1), b"n = "), (dict(rule=2), b"rule = 2"), (dict(rule=-1), b"rule = -1"),
                     (dict(ws=None), b"workspace is NULL"), (dict(ws=WS + 128), b"256-byte aligned"),
                     (dict(n=0, dist3=None, scale=None), b"both NULL"), (dict(n=0, rule=7), b"rule = 7")):
        assert knn(candidates=ctypes.byref(counted), **kw) == _ffi.GSX_ERR_INVALID_ARGUMENT, kw
        assert word in lib.gsx_last_error(), (kw, lib.gsx_last_error())
        assert counted.value == 77
    assert knn(ws_bytes=big - 1) == _ffi.GSX_ERR_WORKSPACE_TOO_SMALL and b"gsx_knn3_workspace_bytes" in lib.gsx_last_error()
    # n = 0 succeeds, looks at no pointer and writes nothing but the count
    assert knn(n=0, points=None, ws=None, ws_bytes=0, candidates=ctypes.byref(counted)) == _ffi.GSX_OK and counted.value == 0
    assert knn(n=0, scale=None) == _ffi.GSX_OK and knn(n=0, dist3=None) == _ffi.GSX_OK


# ---- Python surface, as far as it goes without a GPU
def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    import intro_to_gaussian_splatting_amd as pkg
    from intro_to_gaussian_splatting_amd import Gaussians, nearest3

    assert "nearest3" in pkg.__all__ and callable(Gaussians.initialize_scale)
    p = torch.rand((8, 3))
    with pytest.raises(ValueError, match="points is on cpu.*no CPU fallback"):
        nearest3(p)
    with pytest.raises(ValueError, match="contiguous float32"):
        nearest3(p.double())
    with pytest.raises(ValueError, match="contiguous float32"):
        nearest3(torch.rand((3, 8)).t())
    with pytest.raises(ValueError, match="shape \\(n, 3\\)"):
        nearest3(torch.rand((8, 4)))
    with pytest.raises(ValueError, match="rule"):
        nearest3(p, rule="mean")
    g = Gaussians(p, torch.zeros((8, 3)), device="cpu")
    before = g.scales.clone()
    with pytest.raises(ValueError, match="no CPU fallback"):
        g.initialize_scale()
    with pytest.raises(ValueError, match="rule"):
        g.initialize_scale(rule="paper")
    assert torch.equal(g.scales, before)


def test_spatially_ordered_is_the_permutation_of_the_shared_morton_helper():
    """spatially_ordered() shares knn.morton_permutation: ten bits by default, ties by row, and a 21-bit curve refines it."""
    from intro_to_gaussian_splatting_amd import Gaussians
    from intro_to_gaussian_splatting_amd.knn import morton_permutation

    p = torch.from_numpy(kr.cloud("clustered", 1500))
    g = Gaussians(p, torch.zeros((1500, 3)), device="cpu").spatially_ordered()
    assert torch.equal(g.original_index.long(), morton_permutation(p, 10))
    fine = morton_permutation(p, 21)
    assert sorted(fine.tolist()) == list(range(1500))
    lattice = torch.from_numpy(kr.cloud("lattice", 900))
    assert sorted(morton_permutation(lattice, 21).tolist()) == list(range(900))


# ---- the restatement against the reference's own results
@pytest.mark.parametrize("kind,n", kr.FIXTURES)
def test_restatement_against_the_reference(kind, n):
    g = _golden(kind, n)
    c = kr.case(kind, n)
    assert np.array_equal(g["points"].view(np.uint32), c["points"].view(np.uint32)), "the cloud generator moved: capture again"
    assert g["scales"].shape == (n, 3) and g["dist3"].shape == (n, 3)
    mine = F(0.001) * c["scale_reference"]                                  # scales = 0.001 ones; scales *= scale
    assert mine.dtype == F
    for axis in range(3):
        assert _close(mine[:, 0], g["scales"][:, axis], 16 * EPS), (kind, n, axis)
    assert _close(c["dist3"], g["dist3"], 8 * EPS)                          # two distances, 3.5 eps each, and the second order
    if n < 4:
        assert np.isinf(c["dist3"][:, n - 1:]).all() and np.isinf(mine).all() and np.isinf(g["scales"]).all()
        assert np.isfinite(c["dist3"][:, :n - 1]).all()
    else:
        assert np.isfinite(c["dist3"]).all() and (mine > 0).all()
    if kind == "clustered":
        assert (c["dist3"][:, 0] == 0).sum() >= n // 8                      # the duplicates count, at distance 0
        assert np.array_equal(c["dist3"][:, 0] == 0, g["dist3"][:, 0] == 0)
    if kind == "lattice":
        assert (c["dist3"] == F(0.25)).mean() > 0.5                         # ties: most rows have three neighbours at the pitch


# ---- the restatement against float64
@pytest.mark.parametrize("kind,n", kr.FIXTURES)
def test_restatement_against_a_float64_brute_force(kind, n):
    c = kr.case(kind, n)
    p = c["points"].astype(np.float64)
    d = np.sqrt(((p[None, :, :] - p[:, None, :]) ** 2).sum(axis=2))
    d[np.arange(n), np.arange(n)] = np.inf
    d3 = np.sort(d, axis=1)[:, :3]
    if n < 4:
        d3 = np.concatenate([d3, np.full((n, 3 - d3.shape[1]), np.inf)], axis=1)
    assert _close(c["dist3"], d3, 4 * EPS)
    with np.errstate(invalid="ignore"):
        ref = np.maximum(d3.sum(axis=1) / 3.0, 1e-5)
        pub = np.sqrt(np.maximum((d3 ** 2).sum(axis=1) / 3.0, 1e-7))
    assert _close(c["scale_reference"][:, 0], ref, 8 * EPS)
    assert _close(c["scale_published"][:, 0], pub, 8 * EPS)
    assert (np.diff(c["q3"], axis=1) >= 0).all() if n >= 4 else True


def test_restatement_does_not_depend_on_the_order_of_the_rows():
    """Only the values of the three smallest q enter: a permuted cloud gives the permuted rows, bit for bit."""
    c = kr.case("clustered", 1500)
    perm = np.random.RandomState(3).permutation(1500)
    q3 = kr.nearest3_sq(c["points"][perm])
    assert np.array_equal(q3.view(np.uint32), c["q3"][perm].view(np.uint32))
    assert np.array_equal(np.sort(kr.morton_order(c["points"])), np.arange(1500))
