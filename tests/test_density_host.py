"""Density control without a GPU: the header and the binding, every refusal of the three calls by name (before any HIP call),
the Python surface's ValueErrors on CPU tensors, and the float32 restatement (tests/density_restatement.py) against an
independent float64 composition in torch on the CPU -- boolean masks, cat, and the rotation from the textbook formula
R = I + 2 w [v]x + 2 [v]x^2 of the unit quaternion.

Tolerance of a split child's position against the float64 value (eps = 2^-24, |R| <= 1, d_k = s_k e_k):
the unit quaternion's components carry <= 3 eps relative; an off-diagonal entry 2 (x y +- w z) then <= 16 eps absolute, a
diagonal entry 1 - 2 (y y + z z) <= 17 eps; a term R d_k <= (17 + 1 + 1) eps |d_k|; the two additions of the three terms
<= 2 eps sum|d_k|; the final addition <= eps |result|.  Bound: eps (|result| + 22 sum_k |d_k|) (21, and one for the second
order).  A split scale s / shrink is one correctly rounded divide: eps |result|.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import density_restatement as dr

RULES = dr.rules(grad_threshold=0.5, dense_scale=0.1, prune_logit=-2.0, prune_scale=1.0, split_shrink=1.6)
MIXES = ("keep", "prune", "split", "random", "edges")
EPS = 2.0 ** -24


def case(n, mix, seed=0):
    """A scene of n rows whose actions under RULES are `mix`: dict of float32 / uint32 arrays.  No statistic lies within
    1e-6 relative of a threshold (asserted by clear_of_thresholds)."""
    rs = np.random.RandomState(1000 * seed + n % 997)
    def pick(lo_hi):                    # uniform inside one of the intervals, which keep clear of the thresholds
        ends = np.array(lo_hi)[rs.randint(0, len(lo_hi), size=n)]
        return rs.uniform(ends[:, 0], ends[:, 1])

    seen = rs.randint(0, 6, size=n).astype(np.uint32)
    mean = pick([(0.05, 0.4), (0.6, 3.0)])
    smax = pick([(0.01, 0.08), (0.12, 0.9), (1.1, 2.0)])
    logit = pick([(-4.0, -2.1), (-1.9, 4.0), (-1.9, 4.0)])
    if mix == "keep":
        seen[:], smax, logit = 0, np.minimum(smax, 0.9), np.abs(logit)
    elif mix == "prune":
        logit = -np.abs(logit) - 2.1
    elif mix == "split":
        seen[:], mean, smax, logit = 3, mean + 0.6, rs.uniform(0.12, 0.9, size=n), np.abs(logit)
    elif mix == "edges":                # the first and last row of every block of 256: PRUNE | SPLIT, alternating
        for b, lo in enumerate(range(0, n, 256)):
            hi = min(lo + 256, n) - 1
            for row, split in ((lo, b % 2 == 1), (hi, b % 2 == 0)):
                if split:
                    seen[row], mean[row], smax[row], logit[row] = 2, 1.5, 0.5, 1.0
                else:
                    logit[row] = -3.0
    scales = (smax[:, None] * rs.uniform(0.2, 1.0, size=(n, 3))).astype(np.float32)
    scales[np.arange(n), rs.randint(0, 3, size=n)] = smax.astype(np.float32)
    q = rs.normal(size=(n, 4)) * np.exp(rs.uniform(-2, 2, size=(n, 1)))        # not normalised
    return dict(grad_sum=(mean * seen).astype(np.float32), seen=seen, scales=scales,
                opacity=logit.astype(np.float32).reshape(n, 1), quats=q.astype(np.float32),
                points=rs.normal(size=(n, 3)).astype(np.float32), noise=rs.normal(size=(n, 2, 3)).astype(np.float32))


def clear_of_thresholds(c, r=RULES, rel=1e-6):
    s = c["scales"].astype(np.float64).max(axis=1)
    seen = c["seen"].astype(np.float64)
    mean = c["grad_sum"].astype(np.float64)[seen > 0] / seen[seen > 0]
    far = lambda v, t: bool((np.abs(v - float(t)) > rel * abs(float(t))).all())  # noqa: E731
    return far(s, r["dense_scale"]) and far(s, r["prune_scale"]) and far(mean, r["grad_threshold"]) and \
        far(c["opacity"].astype(np.float64), r["prune_logit"])


# ---- C ABI
def test_header_declares_ffi_binds_and_layout():
    from intro_to_gaussian_splatting_amd import _ffi

    hdr = open(os.path.join(ROOT, "include", "gsx.h")).read()
    import test_cabi

    declared = test_cabi._declared_functions()
    for name, n_args in (("gsx_density_accumulate", 6), ("gsx_density_workspace_bytes", 1), ("gsx_density_plan", 10),
                         ("gsx_density_apply", 9)):
        assert re.search(r"GSX_API\s+\w+\s+%s\(" % name, hdr) and name in declared, name
        assert len(_ffi.SIGNATURES[name][1]) == n_args, name
        assert hasattr(_ffi.load(), name)
    assert re.search(r"#define\s+GSX_VERSION\s+305\b", hdr) and _ffi.load().gsx_version() == 305
    assert ctypes.sizeof(_ffi.GsxDensityGroup) == 24 and ctypes.sizeof(_ffi.GsxDensityRules) == 24
    assert _ffi.GsxDensityGroup.dst.offset == 8 and _ffi.GsxDensityGroup.width.offset == 16 and _ffi.GsxDensityGroup.role.offset == 20
    assert [f[0] for f in _ffi.GsxDensityRules._fields_] == ["grad_threshold", "dense_scale", "prune_logit", "prune_scale",
                                                             "split_shrink", "flags"]
    assert ctypes.sizeof(_ffi.GsxParams) == 160 and ctypes.sizeof(_ffi.GsxFrameStats) == 72
    for name in ("GSX_DENSITY_MAX_GROUPS", "GSX_DENSITY_COPY", "GSX_DENSITY_ZERO_NEW", "GSX_DENSITY_POINTS", "GSX_DENSITY_SCALES",
                 "GSX_DENSITY_QUATS"):
        m = re.search(r"\b%s\s*=?\s*(\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(_ffi, name), name
    assert (dr.COPY, dr.ZERO_NEW, dr.POINTS, dr.SCALES, dr.QUATS) == (0, 1, 2, 3, 4)
    assert "GSX_FLAG_DENSITY" not in hdr          # (tests/test_cabi.py: every GSX_FLAG_* of the header is a render flag)


def test_workspace_bytes_is_monotone_and_zero_on_bad_arguments():
    from intro_to_gaussian_splatting_amd import _ffi

    f = _ffi.load().gsx_density_workspace_bytes
    sizes = [f(n) for n in (0, 1, 255, 256, 257, 1024, 1025, 262144, 262145, 10 ** 6, 2 ** 30)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert sizes[-1] >= 5 * 2 ** 30            # an action byte and a prefix word per row
    assert f(-1) == 0 and f(2 ** 30 + 1) == 0 and f(-2 ** 40) == 0


WS, PTR = 1 << 20, 4096           # a 256-byte aligned "workspace" and "arrays": never dereferenced


def _rules(**kw):
    from intro_to_gaussian_splatting_amd import _ffi

    r = _ffi.GsxDensityRules(0.5, 0.1, -2.0, 1.0, 1.6, 0)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_accumulate_and_plan_refusals_name_the_argument_and_need_no_gpu():
    from intro_to_gaussian_splatting_amd import _ffi

    lib = _ffi.load()
    big = lib.gsx_density_workspace_bytes(100)

    def acc(grad=PTR, width=3, n=100, grad_sum=PTR, seen=PTR):
        return lib.gsx_density_accumulate(grad, width, n, grad_sum, seen, None)

    for kw, word in ((dict(grad=None), b"grad is"), (dict(grad_sum=None), b"grad_sum"), (dict(seen=None), b"seen"),
                     (dict(width=0), b"width"), (dict(width=2 ** 20 + 1), b"width"), (dict(n=-1), b"n = -1"),
                     (dict(n=2 ** 30 + 1), b"n = ")):
        assert acc(**kw) == _ffi.GSX_ERR_INVALID_ARGUMENT, kw
        assert word in lib.gsx_last_error(), (kw, lib.gsx_last_error())
    assert acc(n=0) == _ffi.GSX_OK and acc(n=0, grad=None, grad_sum=None, seen=None) == _ffi.GSX_OK

    counts = (ctypes.c_int64 * 4)(7, 7, 7, 7)

    def plan(grad_sum=PTR, seen=PTR, scales=PTR, opacity=PTR, n=100, rules=None, ws=WS, ws_bytes=big, out=counts):
        rules = ctypes.byref(_rules()) if rules is None else rules
        return lib.gsx_density_plan(grad_sum, seen, scales, opacity, n, rules, ws, ws_bytes, out, None)

    nan = float("nan")
    for kw, word in ((dict(grad_sum=None), b"grad_sum"), (dict(seen=None), b"seen"), (dict(scales=None), b"scales"),
                     (dict(opacity=None), b"opacity_logit"), (dict(n=-1), b"n = -1"), (dict(n=2 ** 30 + 1), b"n = "),
                     (dict(rules=ctypes.POINTER(_ffi.GsxDensityRules)()), b"rules"), (dict(ws=None), b"workspace"),
                     (dict(ws=WS + 128), b"256-byte aligned"), (dict(out=None), b"counts_host"),
                     (dict(rules=ctypes.byref(_rules(flags=1))), b"flags"),
                     (dict(rules=ctypes.byref(_rules(split_shrink=0.0))), b"split_shrink"),
                     (dict(rules=ctypes.byref(_rules(split_shrink=nan))), b"split_shrink")):
        assert plan(**kw) == _ffi.GSX_ERR_INVALID_ARGUMENT, kw
        assert word in lib.gsx_last_error(), (kw, lib.gsx_last_error())
    assert plan(ws_bytes=big - 1) == _ffi.GSX_ERR_WORKSPACE_TOO_SMALL and b"gsx_density_workspace_bytes" in lib.gsx_last_error()
    assert list(counts) == [7, 7, 7, 7]
    assert plan(n=0, ws_bytes=lib.gsx_density_workspace_bytes(0)) == _ffi.GSX_OK and list(counts) == [0, 0, 0, 0]


def _groups(spec, **last):
    """spec: [(width, role)]; `last`: fields of the last group overwritten."""
    from intro_to_gaussian_splatting_amd import _ffi

    arr = (_ffi.GsxDensityGroup * max(len(spec), 1))()
    for i, (width, role) in enumerate(spec):
        arr[i].src, arr[i].dst, arr[i].width, arr[i].role = PTR * (2 * i + 1), PTR * (2 * i + 2), width, role
    for k, v in last.items():
        setattr(arr[len(spec) - 1], k, v)
    return arr


def test_apply_refusals_name_the_argument_and_need_no_gpu():
    from intro_to_gaussian_splatting_amd import _ffi

    lib = _ffi.load()
    big = lib.gsx_density_workspace_bytes(100)
    P, S, Q, C, Z = (3, dr.POINTS), (3, dr.SCALES), (4, dr.QUATS), (48, dr.COPY), (1, dr.ZERO_NEW)
    full = [P, S, Q, C, Z]

    def apply(spec=full, n_groups=None, n=100, n_out=150, noise=PTR, ws=WS, ws_bytes=big, groups=False, **last):
        arr = _groups(spec, **last) if groups is False else groups
        return lib.gsx_density_apply(arr, len(spec) if n_groups is None else n_groups, n, n_out, noise, None, ws, ws_bytes, None)

    bad = [(dict(groups=None), b"groups is NULL"), (dict(n_groups=0), b"n_groups"), (dict(n_groups=25), b"n_groups"),
           (dict(spec=[C] * 25), b"n_groups"), (dict(n=-1), b"n = -1"), (dict(n=2 ** 30 + 1), b"n = "),
           (dict(n_out=-1), b"n_out"), (dict(n_out=201), b"n_out"), (dict(ws=None), b"workspace"),
           (dict(ws=WS + 64), b"256-byte aligned"),
           (dict(width=0), b"groups[4].width"), (dict(width=2 ** 20 + 1), b"groups[4].width"),
           (dict(role=5), b"groups[4].role"), (dict(role=-1), b"groups[4].role"),
           (dict(src=None), b"groups[4].src"), (dict(dst=None), b"groups[4].dst"), (dict(dst=PTR * 9), b"groups[4].dst equals src"),
           (dict(spec=full + [P]), b"second POINTS"), (dict(spec=full + [S]), b"second SCALES"), (dict(spec=full + [Q]), b"second QUATS"),
           (dict(spec=[S, Q, (4, dr.POINTS)]), b"groups[2].width = 4: a POINTS group has width 3"),
           (dict(spec=[P, Q, (4, dr.SCALES)]), b"a SCALES group has width 3"),
           (dict(spec=[P, S, (3, dr.QUATS)]), b"a QUATS group has width 4"),
           (dict(spec=[P, S, C]), b"POINTS group needs a SCALES and a QUATS"), (dict(spec=[P, Q]), b"POINTS group needs"),
           (dict(spec=[P]), b"POINTS group needs"), (dict(noise=None), b"noise")]
    for kw, word in bad:
        assert apply(**kw) == _ffi.GSX_ERR_INVALID_ARGUMENT, kw
        assert word in lib.gsx_last_error(), (kw, lib.gsx_last_error())
    assert apply(ws_bytes=big - 1) == _ffi.GSX_ERR_WORKSPACE_TOO_SMALL
    # nothing to do: no pointer is looked at, but the descriptors are still checked; noise may be NULL without a POINTS group
    assert apply(n=0, n_out=0, ws_bytes=256 * 3) == _ffi.GSX_OK and apply(n_out=0) == _ffi.GSX_OK
    assert apply(n_out=0, spec=[S, Q, C, Z], noise=None) == _ffi.GSX_OK and apply(n_out=0, spec=[C] * 24, noise=None) == _ffi.GSX_OK
    assert apply(n_out=0, role=7) == _ffi.GSX_ERR_INVALID_ARGUMENT


# ---- Python surface, as far as it goes without a GPU
def test_python_surface_refuses_cpu_tensors_foreign_optimisers_and_ordered_containers():
    from intro_to_gaussian_splatting_amd import DensityControl, Gaussians, GaussianScene

    g = Gaussians(torch.zeros((4, 3)), torch.zeros((4, 3)), device="cpu")
    with pytest.raises(ValueError, match="points is on cpu.*no CPU fallback"):
        DensityControl(g)

    class Opt:
        gaussians = Gaussians(torch.zeros((4, 3)), torch.zeros((4, 3)), device="cpu")

    with pytest.raises(ValueError, match="optimizer belongs to another container"):
        DensityControl(g, optimizer=Opt())
    with pytest.raises(ValueError, match="split_shrink"):
        DensityControl(g, split_shrink=0.0)
    ordered = Gaussians(torch.rand((8, 3)), torch.zeros((8, 3)), device="cpu").spatially_ordered()
    assert ordered.original_index is not None
    with pytest.raises(ValueError, match="spatially ordered.*call spatially_ordered\\(\\) again"):
        DensityControl(ordered)
    assert callable(GaussianScene.gaussians_changed)


# ---- the restatement against float64
def _textbook_rotation(q):
    """R = I + 2 w [v]x + 2 [v]x^2 of the unit quaternion (w, v), float64 torch; the identity for a zero quaternion."""
    q = q.double()
    nrm = q.norm(dim=1, keepdim=True)
    unit = torch.where(nrm > 0, q / torch.where(nrm > 0, nrm, torch.ones_like(nrm)), torch.tensor([1.0, 0, 0, 0], dtype=torch.float64))
    w, v = unit[:, 0], unit[:, 1:]
    K = torch.zeros((q.shape[0], 3, 3), dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -v[:, 2], v[:, 1], v[:, 2], -v[:, 0], -v[:, 1], v[:, 0]
    return torch.eye(3, dtype=torch.float64) + 2 * w[:, None, None] * K + 2 * K @ K


def _float64_composition(c, r):
    """The round as a user would compose it in torch: masks, indexing, cat; the new rows APPENDED (clones, then the split
    children).  Returns per kind the source rows and, for the split children, positions / scales / offsets' |d| sum."""
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in c.items() if k != "seen"}
    seen = torch.from_numpy(c["seen"].astype(np.int64))
    s = t["scales"].double()
    smax = s.max(dim=1).values
    mean = t["grad_sum"].double() / seen.clamp(min=1).double()
    prune = (t["opacity"].double().reshape(-1) < float(r["prune_logit"])) | (smax > float(r["prune_scale"]))
    hot = (seen > 0) & (mean >= float(r["grad_threshold"]))
    split = ~prune & hot & (smax > float(r["dense_scale"]))
    clone = ~prune & hot & ~(smax > float(r["dense_scale"]))
    keep = ~prune & ~split
    rows = torch.arange(s.shape[0])
    d = s[split][:, None, :] * t["noise"].double()[split]                      # (m, 2, 3)
    off = torch.einsum("mkj,mcj->mck", _textbook_rotation(t["quats"][split]), d)
    children = t["points"].double()[split][:, None, :] + off
    return dict(continued=rows[keep], cloned=rows[clone], split=rows[split], children=children,
                child_scales=s[split] / float(r["split_shrink"]), dsum=d.abs().sum(dim=2), pruned=rows[prune])


@pytest.mark.parametrize("mix", MIXES)
def test_restatement_against_an_independent_float64_composition(mix):
    left_out = 0
    for n in (1, 257, 1500):
        c = case(n, mix, seed=3)
        if not clear_of_thresholds(c):
            left_out += 1
            continue
        action, prefix, counts = dr.plan(c["grad_sum"], c["seen"], c["scales"], c["opacity"], RULES)
        ref = _float64_composition(c, RULES)
        # actions and counts, exactly
        assert sorted(np.flatnonzero(action == dr.PRUNE)) == ref["pruned"].tolist()
        assert sorted(np.flatnonzero(action == dr.CLONE)) == ref["cloned"].tolist()
        assert sorted(np.flatnonzero(action == dr.SPLIT)) == ref["split"].tolist()
        assert counts == (len(ref["continued"]) + len(ref["cloned"]) + 2 * len(ref["split"]), len(ref["pruned"]),
                          len(ref["cloned"]), len(ref["split"]))
        if mix == "keep":
            assert counts == (n, 0, 0, 0)
        if mix == "prune":
            assert counts == (0, n, 0, 0)
        if mix == "split":
            assert counts == (2 * n, 0, 0, n)
        if mix in ("random", "edges") and n > 256:
            assert min(counts) > 0
        # source_row, exactly: rows in source order, the children beside their parent
        groups = [(c["points"], dr.POINTS), (c["scales"], dr.SCALES), (c["quats"], dr.QUATS), (c["opacity"], dr.COPY),
                  (c["noise"].reshape(n, 6), dr.ZERO_NEW)]
        (pts, scl, qts, opa, mom), source_row = dr.apply(groups, action, prefix, counts[0], c["noise"], RULES["split_shrink"])
        want = []
        for i in range(n):
            want += {dr.KEEP: [i], dr.PRUNE: [], dr.CLONE: [i, -(i + 1)], dr.SPLIT: [-(i + 1), -(i + 1)]}[int(action[i])]
        assert source_row.tolist() == want and source_row.dtype == np.int32
        assert prefix.tolist() == [sum(int(dr.ROWS_OF[a]) for a in action[:i]) for i in range(n)] if n <= 300 else True
        # continued and cloned rows: the source's bits; new moments: +0
        src = np.where(source_row >= 0, source_row, -source_row - 1)
        is_split = action[src] == dr.SPLIT
        for got, orig in ((pts, c["points"]), (scl, c["scales"]), (qts, c["quats"]), (opa, c["opacity"])):
            assert np.array_equal(got[~is_split].view(np.uint32), orig[src[~is_split]].view(np.uint32))
        assert np.array_equal(qts.view(np.uint32), c["quats"][src].view(np.uint32))
        new = source_row < 0
        assert not mom[new].view(np.uint32).any()
        assert np.array_equal(mom[~new].view(np.uint32), c["noise"].reshape(n, 6)[src[~new]].view(np.uint32))
        # the split children against float64
        if is_split.any():
            m = len(ref["split"])
            got_p = pts[is_split].reshape(m, 2, 3).astype(np.float64)
            want_p = ref["children"].numpy()
            bound = EPS * (np.abs(want_p) + 22.0 * ref["dsum"].numpy()[:, :, None])
            assert (np.abs(got_p - want_p) <= bound).all(), float((np.abs(got_p - want_p) / bound).max())
            got_s = scl[is_split].reshape(m, 2, 3).astype(np.float64)
            want_s = ref["child_scales"].numpy()[:, None, :]
            assert (np.abs(got_s - want_s) <= EPS * np.abs(want_s)).all()
            assert (np.abs(got_p[:, 0] - got_p[:, 1]) > 0).any()            # the two children differ
    assert left_out == 0


def test_restatement_of_accumulate_and_its_edge_rows():
    rs = np.random.RandomState(5)
    g = rs.normal(size=(40, 3)).astype(np.float32)
    g[3] = 0.0
    g[4] = [0.0, -0.0, 0.0]
    g[5] = [0.0, np.nan, 0.0]
    g[6] = [1e-30, 0.0, 0.0]               # squares underflow: the norm is 0, the row still counts
    s0 = rs.uniform(size=40).astype(np.float32)
    n0 = rs.randint(0, 4, size=40).astype(np.uint32)
    s1, n1 = dr.accumulate(g, s0, n0)
    live = np.ones(40, bool)
    live[[3, 4]] = False
    assert np.array_equal(n1, n0 + live.astype(np.uint32))
    assert np.array_equal(s1[~live].view(np.uint32), s0[~live].view(np.uint32))
    assert np.isnan(s1[5]) and s1[6] == s0[6] and n1[6] == n0[6] + 1
    fin = live & (np.arange(40) != 5)
    want = s0.astype(np.float64) + np.sqrt((g.astype(np.float64) ** 2).sum(axis=1))
    assert (np.abs(s1[fin] - want[fin]) <= 4 * EPS * np.abs(want[fin])).all()


def test_restatement_nan_rows_are_kept_and_a_zero_quaternion_is_the_identity():
    c = case(64, "split", seed=1)
    c["grad_sum"][0] = np.nan
    c["scales"][1, 1] = np.nan
    c["opacity"][2] = np.nan
    c["quats"][3] = 0.0
    action, prefix, counts = dr.plan(c["grad_sum"], c["seen"], c["scales"], c["opacity"], RULES)
    assert action[0] == dr.KEEP and action[1] == dr.KEEP and action[2] == dr.SPLIT and (action[3:] == dr.SPLIT).all()
    assert counts == (2 * 64 - 2, 0, 0, 62)
    R = dr.rotation(c["quats"][:5])
    assert np.array_equal(R[3], np.eye(3, dtype=np.float32))
    assert np.abs(R[4] @ R[4].T - np.eye(3)).max() < 1e-6
    want = _textbook_rotation(torch.from_numpy(c["quats"][:5])).numpy()
    assert np.abs(R - want).max() <= 17 * EPS
