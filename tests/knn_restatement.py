"""The contract of gsx_knn3 (include/gsx.h), restated op for op: numpy, float32, brute force over all pairs.

For row i, over all rows j != i (by row: a duplicate counts, at distance 0): dx = xj - xi (likewise dy, dz),
q = (dx dx + dy dy) + dz dz, every operation rounded to float32 on its own; the three smallest q ascending, d_k = sqrt(q_k)
correctly rounded, +inf where there is no neighbour.  Only the values of the three smallest q enter, so neither ties nor
the order of the candidates matter.  numpy's float32 arithmetic rounds every operation and fuses nothing.

``nearest3_sq_torch`` is the same brute force in torch, for the sizes at which numpy's takes minutes.

Also the point clouds the knn tests share (``cloud``): the capture tool makes the reference's fixtures of them.
"""
import functools

import numpy as np

REFERENCE, PUBLISHED = 0, 1
F = np.float32
CLOUDS = ("uniform", "clustered", "lattice", "seams")
# the reference's fixtures (tools/capture_knn_golden.py): (cloud, n)
FIXTURES = (("uniform", 3), ("uniform", 4), ("uniform", 257), ("uniform", 1500), ("clustered", 1500), ("lattice", 900),
            ("seams", 1200))


def fixture_name(kind, n):
    return "knn_%s_n%d" % (kind, n)


def cloud(kind, n, seed=0):
    """(n, 3) float32, finite.
    uniform    the unit cube scaled to [-2, 3]
    clustered  clusters of very different sizes and axis ratios up to 100 : 1, an eighth of the rows exact duplicates of others
    lattice    an integer lattice at pitch 0.25 (every distance tied many times over), rows shuffled
    seams      within 1e-3 of the three mid-planes of the bounding box: the seams of a Morton curve, where the nearest
               neighbour lies far along the curve"""
    rs = np.random.RandomState(7919 * seed + 31 * n + CLOUDS.index(kind))
    if kind == "uniform":
        p = rs.uniform(-2.0, 3.0, size=(n, 3))
    elif kind == "clustered":
        k = max(1, min(12, n // 20))
        centre = rs.uniform(-10.0, 10.0, size=(k, 3))
        sigma = np.exp(rs.uniform(np.log(1e-3), np.log(1.0), size=(k, 1))) * np.exp(rs.uniform(np.log(0.01), 0.0, size=(k, 3)))
        which = rs.randint(0, k, size=n)
        p = centre[which] + sigma[which] * rs.normal(size=(n, 3))
        p = p.astype(F)
        dup = rs.choice(n, size=n // 8, replace=False)
        p[dup] = p[rs.randint(0, n, size=dup.size)]
    elif kind == "lattice":
        side = int(np.ceil(n ** (1.0 / 3.0)))
        g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
        p = g[rs.permutation(g.shape[0])[:n]] * 0.25 - 1.0
    elif kind == "seams":
        p = rs.uniform(-1.0, 1.0, size=(n, 3))
        axis = rs.randint(0, 3, size=n)
        p[np.arange(n), axis] = rs.uniform(-1e-3, 1e-3, size=n)
        p[:min(n, 8)] = np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], dtype=np.float64)[:min(n, 8)]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p, dtype=F)


def nearest3_sq(points, chunk=512):
    """(n, 3) float32: the three smallest q of every row, ascending; +inf where there is no neighbour."""
    p = np.ascontiguousarray(points, dtype=F)
    n = p.shape[0]
    out = np.full((n, 3), np.inf, dtype=F)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    for i0 in range(0, n, chunk):
        i1 = min(i0 + chunk, n)
        dx = x[None, :] - x[i0:i1, None]
        dy = y[None, :] - y[i0:i1, None]
        dz = z[None, :] - z[i0:i1, None]
        q = (dx * dx + dy * dy) + dz * dz
        assert q.dtype == F
        q[np.arange(i1 - i0), np.arange(i0, i1)] = np.inf          # exclusion by row
        k = min(3, n)
        part = np.partition(q, k - 1, axis=1)[:, :k] if n > k else q
        out[i0:i1, :k] = np.sort(part, axis=1)[:, :k]
    return out


def nearest3_sq_torch(points, device, chunk=1024):
    """nearest3_sq in torch float32 on `device`, for the sizes at which numpy's brute force takes minutes: the same n^2
    pairs in the same operation order, 1024 queries x n per step, every operation an eager elementwise op of its own (each
    rounds on its own; nothing is there to contract), the query's own row set to +inf, the three smallest by topk.  An oracle
    only where tests/test_hip_knn.py has first held it to nearest3_sq bit for bit."""
    import torch

    p = torch.from_numpy(np.array(points, dtype=F)).to(device)           # (a copy: the shared cases are read only)
    n = p.shape[0]
    out = torch.full((n, 3), float("inf"), dtype=torch.float32, device=device)
    x, y, z = p[:, 0].contiguous(), p[:, 1].contiguous(), p[:, 2].contiguous()
    k = min(3, n)
    for i0 in range(0, n, chunk):
        i1 = min(i0 + chunk, n)
        dx = x[None, :] - x[i0:i1, None]
        dy = y[None, :] - y[i0:i1, None]
        dz = z[None, :] - z[i0:i1, None]
        xx, yy, zz = dx * dx, dy * dy, dz * dz
        q = (xx + yy) + zz
        assert q.dtype == torch.float32 and q.shape == (i1 - i0, n)
        q[torch.arange(i1 - i0, device=device), torch.arange(i0, i1, device=device)] = float("inf")    # exclusion by row
        out[i0:i1, :k] = torch.topk(q, k, dim=1, largest=False, sorted=True).values
    return out.cpu().numpy()


def scale_of(q3, rule):
    """(n, 1) float32 from the three smallest q."""
    q3 = np.ascontiguousarray(q3, dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        if rule == PUBLISHED:
            s = np.sqrt(np.maximum(((q3[:, 0] + q3[:, 1]) + q3[:, 2]) / F(3.0), F(1e-7)))
        else:
            d = np.sqrt(q3)
            s = np.maximum(((d[:, 0] + d[:, 1]) + d[:, 2]) / F(3.0), F(1e-5))
    assert s.dtype == F
    return s.reshape(-1, 1)


def nearest3(points, rule=REFERENCE):
    """(dist3 (n, 3), scale (n, 1)), float32: what gsx_knn3 returns, bit for bit."""
    q3 = nearest3_sq(points)
    return np.sqrt(q3), scale_of(q3, rule)


@functools.lru_cache(maxsize=None)
def case(kind, n, seed=0):
    """The cloud and its restated results, computed once and shared (treat as read only):
    dict(points, q3, dist3, scale_reference, scale_published)."""
    p = cloud(kind, n, seed)
    q3 = nearest3_sq(p)
    out = dict(points=p, q3=q3, dist3=np.sqrt(q3), scale_reference=scale_of(q3, REFERENCE), scale_published=scale_of(q3, PUBLISHED))
    for a in out.values():
        a.setflags(write=False)
    return out


def morton_order(points, bits=21):
    """int32 (n,): rows along a Morton curve of the bounding box (numpy; the tests' own, so that the kernel's independence of
    `order` is not checked against the package's helper alone)."""
    p = np.asarray(points, dtype=np.float64)
    n = p.shape[0]
    if n == 0:
        return np.zeros(0, np.int32)
    lo, hi = p.min(axis=0), p.max(axis=0)
    cell = np.clip(((p - lo) / np.maximum(hi - lo, 1e-30) * (1 << bits)).astype(np.int64), 0, (1 << bits) - 1)
    code = np.zeros(n, np.int64)
    for b in range(bits):
        for axis in range(3):
            code |= ((cell[:, axis] >> b) & 1) << (3 * b + axis)
    return np.argsort(code, kind="stable").astype(np.int32)
