"""gsx_knn3 on the GPU (csrc/gsx_knn.hip), knn.nearest3 and Gaussians.initialize_scale on top.

Bits: dist3 and scale under both rules equal the float32 restatement (tests/knn_restatement.py, a brute force over all pairs)
bit for bit, at every size from one point to 32 blocks and a tail, on every cloud of the host tests, and whatever the `order`
in which the rows are blocked: as given, along a Morton curve, at random.  Every output, and the workspace at exactly
gsx_knn3_workspace_bytes(n), lies between two 64-element margins of a sentinel that must survive (no GPU sanitizer); points
is unchanged afterwards.  Pruning is a condition: on eight far-apart clusters the call evaluates at most n^2 / 4 pairs.

Printed on an MI355X:
    eight clusters of 1024 (+3) points under the Morton order: candidates 5832285 = n^2 / 11.51, 712 per query
    tools/bench_knn.py, 10^6 points: C3 2.809 ms, 1951 candidates per query; trained-like 3.178 ms, 2383 per query (no cliff:
      22 % more evaluations, 13 % more time); cdist + topk in chunks on the same GPU 12.3 s
    past 256 boxes (65 536, 65 537, 65 795 points; the oracle there is the restatement's brute force in torch on the device,
      first held to the numpy one bit for bit): under the Morton order n^2 / 42.5 .. n^2 / 44.8 candidates on `uniform` and
      `clustered`; as given and at random n^2 / 1.00 .. 1.01
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import knn_restatement as kr
from test_hip_density import DEV, Guarded
from test_knn_host import EPS, _close, _golden

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [1, 2, 3, 4, 5, 63, 64, 255, 256, 257, 513, 8195]        # 8195: 32 blocks and a tail of three


def _lib():
    from intro_to_gaussian_splatting_amd import _ffi

    return _ffi, _ffi.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _orders(points):
    """None, the Morton order, a random permutation."""
    n = points.shape[0]
    return (("given", None), ("morton", kr.morton_order(points)),
            ("random", np.random.RandomState(n).permutation(n).astype(np.int32)))


def _call(points, order, rule, want_dist3=True, want_scale=True, count=False):
    """One gsx_knn3 between margins; returns (dist3 or None, scale or None, candidates or None), all checked for overruns."""
    _ffi, lib = _lib()
    n = points.shape[0]
    p = torch.from_numpy(np.array(points)).to(DEV)           # (a copy: the shared cases are read only)
    before = p.clone()
    o = None if order is None else torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(DEV)
    need = int(lib.gsx_knn3_workspace_bytes(n))
    assert need > 0 and need % 4 == 0
    ws = Guarded(need // 4)
    assert ws.view.data_ptr() % 256 == 0 and ws.view.numel() * 4 == need
    d = Guarded(3 * n) if want_dist3 else None
    s = Guarded(n) if want_scale else None
    counted = ctypes.c_int64(-1)
    rc = lib.gsx_knn3(p.data_ptr(), n, None if o is None else o.data_ptr(), rule, d.view.data_ptr() if d else None,
                      s.view.data_ptr() if s else None, ctypes.byref(counted) if count else None, ws.view.data_ptr(), need,
                      _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.gsx_last_error()
    assert ws.intact() and (d is None or d.intact()) and (s is None or s.intact()), "a write outside an array"
    assert torch.equal(p.view(torch.int32), before.view(torch.int32)), "points was written"         # (bits: a NaN stays a NaN)
    return (d.view.cpu().numpy().reshape(n, 3) if d else None, s.view.cpu().numpy().reshape(n, 1) if s else None,
            int(counted.value) if count else None)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", kr.CLOUDS)
def test_bits_equal_the_restatement_in_every_order(kind, n):
    c = kr.case(kind, n)
    for label, order in _orders(c["points"]):
        dist3, scale, counted = _call(c["points"], order, kr.REFERENCE, count=True)
        assert np.array_equal(_bits(dist3), _bits(c["dist3"])), (kind, n, label)
        assert np.array_equal(_bits(scale), _bits(c["scale_reference"])), (kind, n, label)
        assert 0 <= counted <= n * (n - 1) and (n > 256 or counted == n * (n - 1)), (kind, n, label, counted)
        none, scale, _ = _call(c["points"], order, kr.PUBLISHED, want_dist3=False)
        assert none is None and np.array_equal(_bits(scale), _bits(c["scale_published"])), (kind, n, label)
    dist3, none, _ = _call(c["points"], None, kr.PUBLISHED, want_scale=False)
    assert none is None and np.array_equal(_bits(dist3), _bits(c["dist3"]))


# ---- more than 256 boxes: knn_search_kernel tests the boxes 256 at a time (`for (b0 = 0; b0 < nb; b0 += 256)`), refreshes
# r3max and rebuilds list[] per pass.  256 boxes are one pass exactly; 257 a second pass over one box of one point; 258 a
# second pass over two, the last a tail of three.
LARGE_SIZES = [256 * 256, 256 * 256 + 1, 257 * 256 + 3]
LARGE_CLOUDS = ("uniform", "clustered")


@functools.lru_cache(maxsize=None)
def _large_case(kind, n):
    """The cloud and its three smallest q by the torch brute force on the device, computed once and shared."""
    p = kr.cloud(kind, n)
    q3 = kr.nearest3_sq_torch(p, DEV)
    for a in (p, q3):
        a.setflags(write=False)
    return p, q3


@pytest.mark.parametrize("kind", LARGE_CLOUDS)
def test_the_torch_brute_force_is_the_numpy_restatement_bit_for_bit(kind):
    """What makes kr.nearest3_sq_torch an oracle at the large sizes: at 8195 points it is kr.nearest3_sq, bit for bit."""
    c = kr.case(kind, 8195)
    assert np.array_equal(_bits(kr.nearest3_sq_torch(c["points"], DEV)), _bits(c["q3"]))
    assert np.array_equal(_bits(kr.nearest3_sq_torch(c["points"], DEV, chunk=1000)), _bits(c["q3"]))     # a partial last chunk


@pytest.mark.parametrize("n", LARGE_SIZES)
@pytest.mark.parametrize("kind", LARGE_CLOUDS)
def test_bits_equal_the_brute_force_past_256_boxes(kind, n):
    p, q3 = _large_case(kind, n)
    assert -(-n // 256) == {256 * 256: 256, 256 * 256 + 1: 257, 257 * 256 + 3: 258}[n] and np.isfinite(q3).all()
    want_dist3, want_scale = np.sqrt(q3), kr.scale_of(q3, kr.REFERENCE)
    for label, order in _orders(p):
        dist3, scale, counted = _call(p, order, kr.REFERENCE, count=True)
        assert np.array_equal(_bits(dist3), _bits(want_dist3)), (kind, n, label)
        assert np.array_equal(_bits(scale), _bits(want_scale)), (kind, n, label)
        assert 0 <= counted <= n * (n - 1), (kind, n, label, counted)
        print("%s n = %d, %s order: candidates %d = n^2 / %.2f" % (kind, n, label, counted, n * n / max(counted, 1)))
        if label == "morton":
            if kind == "uniform":
                assert counted <= n * n // 4, counted          # pruning still happens across the passes
            none, scale, _ = _call(p, order, kr.PUBLISHED, want_dist3=False)
            assert none is None and np.array_equal(_bits(scale), _bits(kr.scale_of(q3, kr.PUBLISHED))), (kind, n)


def test_a_cloud_of_identical_points_stays_linear_and_n_zero_writes_nothing():
    """Skip on bound >= r3: every distance is 0 after the own block, every other box's bound is 0, nothing else is scanned."""
    n = 8195
    p = np.full((n, 3), 1.25, dtype=F)
    dist3, scale, counted = _call(p, None, kr.REFERENCE, count=True)
    assert not dist3.any() and np.array_equal(_bits(scale), _bits(np.full((n, 1), 1e-5, dtype=F)))
    # (the tail's three lanes have two neighbours at home: they scan one more block, then their r3 is 0 as well)
    assert counted == 32 * 256 * 255 + 3 * (2 + 256)
    # 258 boxes, two passes over them: the 257 full blocks find their three at home (255 pairs per lane) and list nothing in
    # either pass (every bound is 0 = r3max).  The tail's three lanes have two neighbours at home (2 pairs each) and r3 = inf,
    # so the first pass lists its 256 boxes; they scan the first of them (256 pairs each), after which r3 = 0 >= every
    # other box's distance: the other 255 are staged and scanned by nobody, and in the second pass r3max = 0 lists nothing.
    n = 257 * 256 + 3
    p = np.full((n, 3), 1.25, dtype=F)
    dist3, scale, counted = _call(p, None, kr.REFERENCE, count=True)
    assert not dist3.any() and np.array_equal(_bits(scale), _bits(np.full((n, 1), 1e-5, dtype=F)))
    assert counted == 257 * 256 * 255 + 3 * (2 + 256)
    _ffi, lib = _lib()
    d = Guarded(3)
    assert lib.gsx_knn3(None, 0, None, 0, d.view.data_ptr(), None, None, None, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert d.intact() and bool((d.view == d.fill).all())


def test_non_finite_points_end_and_stay_inside_the_arrays():
    """Finite coordinates are the precondition; without it the values are unspecified, the call still ends in bounds."""
    p = kr.cloud("uniform", 513).copy()
    p[5, 0], p[300, 2], p[512, 1], p[77] = np.nan, np.inf, -np.inf, np.nan
    for label, order in _orders(np.nan_to_num(p, nan=0.0, posinf=9.0, neginf=-9.0)):
        dist3, scale, counted = _call(p, order, kr.REFERENCE, count=True)
        assert dist3.shape == (513, 3) and 0 <= counted <= 513 * 512, label


@functools.lru_cache(maxsize=None)
def _corner_clusters():
    rs = np.random.RandomState(11)
    corners = np.array([[a, b, c] for a in (0.0, 100.0) for b in (0.0, 100.0) for c in (0.0, 100.0)])
    p = np.concatenate([corners[k] + 0.1 * rs.normal(size=(1024 + (3 if k == 7 else 0), 3)) for k in range(8)]).astype(F)
    p = p[rs.permutation(p.shape[0])]
    return p, kr.nearest3_sq(p)


def test_pruning_happens_on_far_apart_clusters():
    """Eight clusters of 1024 points, sigma 0.1, at the corners of a cube of side 100, three more points in the last, under the
    Morton order: blocks do not straddle clusters except where the three extra points shift them, a workgroup needs its own
    cluster's four or five blocks (about n^2 / 8 pairs), and ANY exact box pruning stays below n^2 / 4."""
    p, q3 = _corner_clusters()
    n = p.shape[0]
    assert n == 8195
    dist3, scale, counted = _call(p, kr.morton_order(p), kr.REFERENCE, count=True)
    print("candidates %d = n^2 / %.2f, %.0f per query" % (counted, n * n / counted, counted / n))
    assert np.array_equal(_bits(dist3), _bits(np.sqrt(q3))) and np.array_equal(_bits(scale), _bits(kr.scale_of(q3, kr.REFERENCE)))
    assert counted <= n * n // 4, counted


# ---- Python
def _gaussians(points):
    from intro_to_gaussian_splatting_amd import Gaussians

    n = points.shape[0]
    return Gaussians(torch.from_numpy(np.array(points)), torch.zeros((n, 3)), device=DEV)


@pytest.mark.parametrize("kind,n", kr.FIXTURES)
def test_initialize_scale_against_the_reference_and_the_restatement(kind, n):
    ref = _golden(kind, n)
    c = kr.case(kind, n)
    g = _gaussians(c["points"])
    address, version = g.scales.data_ptr(), g.scales._version
    g.initialize_scale()
    assert g.scales.data_ptr() == address and g.scales._version > version          # in place: current_block_bounds() sees it
    got = g.scales.cpu().numpy()
    want = F(0.001) * c["scale_reference"]
    for axis in range(3):
        assert np.array_equal(_bits(got[:, axis]), _bits(want[:, 0])), (kind, n, axis)
    assert _close(got, ref["scales"], 16 * EPS)
    if n == 3:
        assert np.isinf(got).all() and np.isinf(ref["scales"]).all()
    # the published rule assigns; a second call gives the same scales again
    for _ in range(2):
        g.initialize_scale(rule="published")
        got = g.scales.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(np.repeat(c["scale_published"], 3, axis=1))), (kind, n)


def test_a_spatially_ordered_container_gives_the_same_values_in_permuted_rows():
    c = kr.case("clustered", 1500)
    plain, ordered = _gaussians(c["points"]), _gaussians(c["points"]).spatially_ordered()
    stale = ordered.current_block_bounds().clone()
    plain.initialize_scale()
    ordered.initialize_scale()
    perm = ordered.original_index.long()
    assert not torch.equal(perm, torch.arange(1500, device=DEV))
    assert torch.equal(ordered.scales, plain.scales[perm])
    fresh = ordered.current_block_bounds()
    assert not torch.equal(fresh[:, 3], stale[:, 3])                # the boxes' largest scale followed the in-place write


def test_nearest3_returns_both_arrays_and_refuses_what_it_cannot_take():
    from intro_to_gaussian_splatting_amd import nearest3

    c = kr.case("seams", 513)
    p = torch.from_numpy(np.array(c["points"])).to(DEV)
    stats = {}
    dist3, scale = nearest3(p, order=torch.from_numpy(kr.morton_order(c["points"])).to(DEV), rule="published", stats=stats)
    assert dist3.shape == (513, 3) and scale.shape == (513, 1) and 0 < stats["candidates"] <= 513 * 512
    assert np.array_equal(_bits(dist3.cpu().numpy()), _bits(c["dist3"]))
    assert np.array_equal(_bits(scale.cpu().numpy()), _bits(c["scale_published"]))
    empty = nearest3(torch.zeros((0, 3), device=DEV))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 1)
    bad = p.clone()
    bad[7, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN or an infinity"):
        nearest3(bad)
    bad[7, 1] = float("inf")
    with pytest.raises(ValueError, match="NaN or an infinity"):
        nearest3(bad)
    with pytest.raises(ValueError, match="contiguous float32"):
        nearest3(p.double())
    with pytest.raises(ValueError, match="contiguous float32"):
        nearest3(p.t().contiguous().t())
    with pytest.raises(ValueError, match="no CPU fallback"):
        nearest3(p.cpu())
    with pytest.raises(ValueError, match="order must be"):
        nearest3(p, order=torch.arange(513, device=DEV))            # int64
    with pytest.raises(ValueError, match="order must be"):
        nearest3(p, order=torch.arange(512, device=DEV, dtype=torch.int32))
