"""gsx_density_accumulate / gsx_density_plan / gsx_density_apply on the GPU (csrc/gsx_density.hip) and DensityControl on top.

Bits: the statistic, the four counts, every rewritten array and source_row equal the float32 restatement
(tests/density_restatement.py) bit for bit, with 16-byte stores and float by float alike.  The plan in the workspace is
checked through what it decides: the counts, and source_row, which names every row's action and place.  Every output lies
between two 64-element margins of a sentinel that must survive (no GPU sanitizer).

Printed on an MI355X:
    short fit, 400 Gaussians, 64 x 64, 30 steps, one round after step 15: loss first 0.0669991, before the round 0.0110978,
      after it 0.081865, last 0.024561; rows 400 -> 418 (12 pruned, 15 cloned, 15 split)
"""
import ctypes

import numpy as np
import pytest
import torch

import density_restatement as dr
from test_density_host import MIXES, RULES, case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 12345.678
GUARD = 64
BIG = 256 * 1024 + 1            # one row more than a single pass of the block-level scan covers (kDensityScanPass, gsx_internal.h)
SIZES = [1, 63, 64, 255, 256, 257, 513, BIG]
P, S, Q = (3, dr.POINTS), (3, dr.SCALES), (4, dr.QUATS)
FULL = [P, S, Q, (1, dr.COPY), (48, dr.COPY), (3, dr.ZERO_NEW), (4, dr.ZERO_NEW), (48, dr.ZERO_NEW), (1, dr.ZERO_NEW)]
SMALL = [(1, dr.COPY), P, (4, dr.ZERO_NEW), S, Q]


class Guarded:
    """`count` elements on the device, `lead` elements behind a 64-element margin and in front of another."""

    def __init__(self, count, lead=0, dtype=torch.float32):
        fill = SENTINEL if dtype == torch.float32 else 0x5A5A5A5
        self.fill, self.lo, self.hi = fill, GUARD + lead, GUARD + lead + count
        self.whole = torch.full((self.hi + GUARD,), fill, dtype=dtype, device=DEV)
        self.view = self.whole[self.lo:self.hi]

    def intact(self):
        return bool((self.whole[:self.lo] == self.fill).all()) and bool((self.whole[self.hi:] == self.fill).all()) and \
            self.whole[self.hi:].numel() == GUARD


def _lib():
    from intro_to_gaussian_splatting_amd import _ffi

    return _ffi, _ffi.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _rules_struct(r=RULES):
    _ffi, _ = _lib()
    return _ffi.GsxDensityRules(float(r["grad_threshold"]), float(r["dense_scale"]), float(r["prune_logit"]),
                                float(r["prune_scale"]), float(r["split_shrink"]), 0)


def _plan(c, n, r=RULES):
    """Runs gsx_density_plan on the case; returns (workspace tensor, counts tuple, the device inputs kept alive)."""
    _ffi, lib = _lib()
    need = lib.gsx_density_workspace_bytes(n)
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = ws[(-ws.data_ptr()) % 256:][:need]
    held = [_dev(c["grad_sum"]), _dev(c["seen"].view(np.int32)), _dev(c["scales"]), _dev(c["opacity"])]
    counts = (ctypes.c_int64 * 4)(-1, -1, -1, -1)
    rules = _rules_struct(r)
    rc = lib.gsx_density_plan(held[0].data_ptr(), held[1].data_ptr(), held[2].data_ptr(), held[3].data_ptr(), n,
                              ctypes.byref(rules), ws.data_ptr(), need, counts, _stream())
    assert rc == 0, lib.gsx_last_error()
    return ws, tuple(int(v) for v in counts)


def _sources(c, n, spec, seed=0):
    rs = np.random.RandomState(seed + 17)
    out = []
    for width, role in spec:
        if role == dr.POINTS:
            out.append(c["points"])
        elif role == dr.SCALES:
            out.append(c["scales"])
        elif role == dr.QUATS:
            out.append(c["quats"])
        else:
            a = rs.normal(size=(n, width)).astype(np.float32)
            a[rs.uniform(size=(n, width)) < 0.05] = -0.0            # a copied -0 stays -0; a new moment is +0
            out.append(a)
    return out


def _apply(ws, n, n_out, spec, sources, noise, lead, n_groups=None, with_rows=True):
    """Runs gsx_density_apply; returns (rc, [Guarded dst], Guarded source_row or None)."""
    _ffi, lib = _lib()
    arr = (_ffi.GsxDensityGroup * max(len(spec), 1))()
    held, dsts = [], []
    for i, ((width, role), src) in enumerate(zip(spec, sources)):
        s, d = _dev(src), Guarded(n_out * width, lead)
        held.append(s)
        dsts.append(d)
        arr[i].src, arr[i].dst, arr[i].width, arr[i].role = s.data_ptr(), d.view.data_ptr(), width, role
    rows = Guarded(n_out, 0, torch.int32) if with_rows else None
    nz = _dev(noise)
    rc = lib.gsx_density_apply(arr, len(spec) if n_groups is None else n_groups, n, n_out, nz.data_ptr(),
                               rows.view.data_ptr() if with_rows else None, ws.data_ptr(), ws.numel(), _stream())
    torch.cuda.synchronize()
    return rc, dsts, rows


def _check_round(n, mix, spec, lead, seed=0, c=None):
    """Plan and apply on one case against the restatement, bit for bit; returns the counts."""
    c = case(n, mix, seed) if c is None else c
    action, prefix, want_counts = dr.plan(c["grad_sum"], c["seen"], c["scales"], c["opacity"], RULES)
    ws, counts = _plan(c, n)
    assert counts == want_counts, (n, mix, counts, want_counts)
    n_out = counts[0]
    sources = _sources(c, n, spec, seed)
    want, want_rows = dr.apply(list(zip(sources, [role for _, role in spec])), action, prefix, n_out, c["noise"],
                               RULES["split_shrink"])
    rc, dsts, rows = _apply(ws, n, n_out, spec, sources, c["noise"], lead)
    assert rc == 0, _lib()[1].gsx_last_error()
    assert _same(rows.view.cpu().numpy(), want_rows) and rows.intact(), (n, mix, lead)
    for (width, role), d, w in zip(spec, dsts, want):
        assert _same(d.view.cpu().numpy().reshape(n_out, width), w), (n, mix, lead, width, role)
        assert d.intact(), (n, mix, lead, width, role)
    return counts


# ---- gsx_density_accumulate
@pytest.mark.parametrize("n", SIZES)
def test_accumulate_equals_the_restatement_bit_for_bit(n):
    _ffi, lib = _lib()
    for width in ((1, 3, 4, 48) if n < BIG else (3,)):
        rs = np.random.RandomState(n % 1000 + width)
        want_sum, want_seen = np.zeros(n, np.float32), np.zeros(n, np.uint32)
        got_sum, got_seen = Guarded(n), Guarded(n, 0, torch.int32)
        got_sum.view.zero_()
        got_seen.view.zero_()
        for call in range(2):
            g = (rs.normal(size=(n, width)) * np.exp(rs.uniform(-6, 2, size=(n, 1)))).astype(np.float32)
            zero = rs.uniform(size=n) < 0.3
            g[zero] = 0.0
            g[zero & (np.arange(n) % 2 == 1), 0] = -0.0                 # -0 is zero
            if n > 2 and call == 1:
                g[n // 2] = 0.0
                g[n // 2, width - 1] = np.nan                           # a NaN is not zero
            grad = Guarded(n * width, call)                             # (the second call: a base off 16-byte alignment)
            grad.view.copy_(_dev(g).reshape(-1))
            rc = lib.gsx_density_accumulate(grad.view.data_ptr(), width, n, got_sum.view.data_ptr(), got_seen.view.data_ptr(), _stream())
            torch.cuda.synchronize()
            assert rc == 0, lib.gsx_last_error()
            want_sum, want_seen = dr.accumulate(g, want_sum, want_seen)
            assert _same(got_sum.view.cpu().numpy(), want_sum), (n, width, call)
            assert np.array_equal(got_seen.view.cpu().numpy().view(np.uint32), want_seen), (n, width, call)
            assert got_sum.intact() and got_seen.intact() and grad.intact()
        assert want_seen.max() <= 2
        if n > 2:
            assert np.isnan(want_sum[n // 2])


# ---- gsx_density_plan and gsx_density_apply
@pytest.mark.parametrize("n", SIZES)
def test_plan_and_apply_equal_the_restatement_for_every_action_mix(n):
    spec = FULL if n < BIG else SMALL
    for mix in MIXES:
        for lead in (0, 1):             # 16-byte aligned dst bases, and bases one float off
            counts = _check_round(n, mix, spec, lead, seed=1)
            if mix == "keep":
                assert counts == (n, 0, 0, 0)
            if mix == "prune":
                assert counts == (0, n, 0, 0)
            if mix == "split":
                assert counts == (2 * n, 0, 0, n)
            if mix in ("random", "edges") and n >= 255:
                assert min(counts) > 0, counts


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_one_group_and_twenty_four_groups(lead):
    n = 513
    for single in ([(3, dr.COPY)], [(1, dr.ZERO_NEW)], [(48, dr.COPY)], [(3, dr.SCALES)], [(4, dr.QUATS)]):
        _check_round(n, "random", single, lead, seed=2)
    widths = [1, 3, 4, 48, 2, 5, 7, 12, 27, 1, 3, 4, 6, 9, 16, 48, 11, 13, 1, 3, 4]
    spec = [P, S, Q] + [(w, dr.ZERO_NEW if i % 2 else dr.COPY) for i, w in enumerate(widths)]
    assert len(spec) == 24
    _check_round(n, "edges", spec, lead, seed=3)


def test_a_twenty_fifth_group_is_refused_and_nothing_is_written():
    _ffi, lib = _lib()
    n = 64
    c = case(n, "random", 4)
    ws, counts = _plan(c, n)
    spec = [(2, dr.COPY)] * 25
    rc, dsts, rows = _apply(ws, n, counts[0], spec, _sources(c, n, spec), c["noise"], 0)
    assert rc == _ffi.GSX_ERR_INVALID_ARGUMENT and b"n_groups" in lib.gsx_last_error()
    assert all(bool((d.whole == SENTINEL).all()) for d in dsts) and bool((rows.whole == rows.fill).all())


def test_apply_refuses_counts_that_are_not_the_plans():
    _ffi, lib = _lib()
    n = 300
    c = case(n, "random", 5)
    ws, counts = _plan(c, n)
    spec = [(3, dr.COPY)]
    for n_call, n_out, word in ((n, counts[0] + 1, b"n_out"), (n, counts[0] - 1, b"n_out"), (n - 1, counts[0], b"n = ")):
        rc, dsts, rows = _apply(ws, n_call, n_out, spec, _sources(c, n, spec), c["noise"], 0)
        assert rc == _ffi.GSX_ERR_INVALID_ARGUMENT and word in lib.gsx_last_error(), (n_call, n_out, lib.gsx_last_error())
        assert bool((dsts[0].whole == SENTINEL).all()) and bool((rows.whole == rows.fill).all())
    rc, dsts, rows = _apply(ws, n, counts[0], spec, _sources(c, n, spec), c["noise"], 0, with_rows=False)      # source_row NULL
    assert rc == 0 and rows is None and dsts[0].intact()


def test_nan_rows_and_a_zero_quaternion():
    n = 300
    c = case(n, "split", 6)
    nan = np.float32(np.nan)
    c["grad_sum"][0] = nan              # a NaN statistic fails >=: KEEP
    c["scales"][1, 1] = nan             # a NaN scale makes smax NaN, which fails every comparison: KEEP
    c["opacity"][2] = nan               # a NaN opacity fails <: not pruned, and this row splits
    c["opacity"][3] = -5.0              # pruned, although its statistic is NaN as well
    c["grad_sum"][3] = nan
    c["quats"][4] = 0.0                 # the identity
    c["quats"][5] = [0.0, 0.0, -0.0, 0.0]
    c["quats"][6, 2] = nan              # a NaN quaternion: !(nrm > 0) holds, the identity again
    action, _, _ = dr.plan(c["grad_sum"], c["seen"], c["scales"], c["opacity"], RULES)
    assert action[:7].tolist() == [dr.KEEP, dr.KEEP, dr.SPLIT, dr.PRUNE, dr.SPLIT, dr.SPLIT, dr.SPLIT]
    for lead in (0, 1):
        counts = _check_round(n, "split", FULL, lead, c=c)
        assert counts == (2 * (n - 3) + 2, 1, 0, n - 3)
    # the identity: the children of row 4 are p + s e
    ws, counts = _plan(c, n)
    rc, dsts, rows = _apply(ws, n, counts[0], [P, S, Q], [c["points"], c["scales"], c["quats"]], c["noise"], 0)
    assert rc == 0
    got = dsts[0].view.cpu().numpy().reshape(-1, 3)
    placed = rows.view.cpu().numpy()
    assert placed[:10].tolist() == [0, 1, -3, -3, -5, -5, -6, -6, -7, -7]       # row 3 is pruned
    for parent in (4, 5, 6):
        at = np.flatnonzero(placed == -(parent + 1))
        for child in range(2):
            assert _same(got[at[child]], c["points"][parent] + c["scales"][parent] * c["noise"][parent, child]), parent
    assert np.isfinite(got).all() and np.isnan(dsts[2].view.cpu().numpy().reshape(-1, 4)[8:10, 2]).all()


def test_two_runs_give_the_same_bits():
    n = 1500
    c = case(n, "random", 7)
    outs = []
    for _ in range(2):
        ws, counts = _plan(c, n)
        rc, dsts, rows = _apply(ws, n, counts[0], FULL, _sources(c, n, FULL, 7), c["noise"], 1)
        assert rc == 0
        outs.append((counts, [d.view.cpu().numpy() for d in dsts], rows.view.cpu().numpy()))
    assert outs[0][0] == outs[1][0] and _same(outs[0][2], outs[1][2])
    for a, b in zip(outs[0][1], outs[1][1]):
        assert _same(a, b)


# ---- DensityControl
NAMES5 = ("points", "scales", "quaternions", "opacity", "colors")
LR5 = {"points": 1e-3, "scales": 5e-3, "quaternions": 1e-3, "opacity": 2e-2, "colors": 2e-2}
KNOBS = dict(grad_threshold=1.5, dense_scale=0.06, prune_logit=-1.0, prune_scale=0.2, split_shrink=1.6)


def _trained_container(n=700, steps=2):
    """A container with an optimiser two steps in (non-zero moments) and a statistic of two accumulated gradients."""
    from intro_to_gaussian_splatting_amd import DensityControl, GaussianAdam
    from test_hip_adam import _container, _set_grads

    g = _container(n)
    for name in NAMES5:
        getattr(g, name).requires_grad_(True)
    opt = GaussianAdam(g, lr=LR5)
    dc = DensityControl(g, optimizer=opt, **KNOBS)
    for t in range(steps):
        _set_grads(g, 300 + t)
        with torch.no_grad():
            g.points.grad[::7] = 0.0            # rows the statistic does not see
        dc.accumulate()
        opt.step()
    return g, opt, dc


def _expected_round(g, opt, dc, seed):
    """The round restated: ({name: array}, {(key, name): array}, counts) from the container as it is now."""
    n = len(g)
    r = dr.rules(**KNOBS)
    cpu = lambda t: t.detach().cpu().numpy()  # noqa: E731
    action, prefix, counts = dr.plan(cpu(dc.grad_sum), cpu(dc.seen).view(np.uint32), cpu(g.scales), cpu(g.opacity), r)
    noise = cpu(torch.randn((n, 2, 3), generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV))
    roles = {"points": dr.POINTS, "scales": dr.SCALES, "quaternions": dr.QUATS}
    groups = [(cpu(getattr(g, k)), roles.get(k, dr.COPY)) for k in NAMES5]
    moments = [(key, k) for k in opt.names for key in ("exp_avg", "exp_avg_sq")]
    groups += [(cpu(getattr(opt, key)[k]), dr.ZERO_NEW) for key, k in moments]
    outs, source_row = dr.apply(groups, action, prefix, counts[0], noise, r["split_shrink"])
    return dict(zip(NAMES5, outs[:5])), dict(zip(moments, outs[5:])), counts, source_row


def test_densify_and_prune_keeps_survivors_bits_and_zeroes_new_moments():
    from test_hip_adam import _set_grads

    g, opt, dc = _trained_container()
    n = len(g)
    assert int((dc.seen == 0).sum()) == 100 and int(dc.seen.max()) == 2
    want, want_m, want_counts, source_row = _expected_round(g, opt, dc, 11)
    before = {k: getattr(g, k).detach().clone() for k in NAMES5}
    before_m = {(key, k): getattr(opt, key)[k].clone() for k in opt.names for key in ("exp_avg", "exp_avg_sq")}
    counts = dc.densify_and_prune(generator=torch.Generator(device=DEV).manual_seed(11))
    assert tuple(counts[k] for k in ("n_out", "n_pruned", "n_cloned", "n_split")) == want_counts and min(want_counts) > 0
    n_out = counts["n_out"]
    assert len(g) == n_out != n and opt.step_count == 2
    for k in NAMES5:
        t = getattr(g, k)
        assert t.is_leaf and t.requires_grad and t.grad is None and t.shape[0] == n_out, k
        assert _same(t.detach().cpu().numpy().reshape(n_out, -1), want[k]), k
    kept, new = source_row >= 0, source_row < 0
    src = torch.from_numpy(np.where(kept, source_row, 0)).to(DEV).long()
    keptd = torch.from_numpy(kept).to(DEV)
    for k in NAMES5:        # a survivor's parameters: the bits they had
        assert torch.equal(getattr(g, k).detach()[keptd].view(torch.int32), before[k][src[keptd]].view(torch.int32)), k
    for (key, k), w in want_m.items():
        m = getattr(opt, key)[k]
        assert _same(m.cpu().numpy().reshape(n_out, -1), w), (key, k)
        assert torch.equal(m[keptd].view(torch.int32), before_m[(key, k)][src[keptd]].view(torch.int32)), (key, k)
        assert not m[torch.from_numpy(new).to(DEV)].view(torch.int32).any() and bool(before_m[(key, k)].any()), (key, k)
    assert dc.grad_sum.shape == (n_out,) and dc.seen.shape == (n_out,) and not dc.grad_sum.any() and not dc.seen.any()
    # the next step runs on the new sizes
    _set_grads(g, 400)
    dc.accumulate()
    opt.step()
    assert opt.step_count == 3 and int(dc.seen.sum()) == n_out
    assert all(bool(torch.isfinite(getattr(g, k)).all()) and opt.exp_avg[k].shape == getattr(g, k).shape for k in NAMES5)


def test_the_same_seed_gives_the_same_container_and_max_gaussians_prunes_only():
    rounds = []
    for seed in (21, 21, 22):
        g, opt, dc = _trained_container()
        dc.densify_and_prune(generator=torch.Generator(device=DEV).manual_seed(seed))
        rounds.append({k: getattr(g, k).detach().clone() for k in NAMES5})
    for k in NAMES5:
        assert torch.equal(rounds[0][k].view(torch.int32), rounds[1][k].view(torch.int32)), k
    assert not torch.equal(rounds[0]["points"], rounds[2]["points"])
    assert torch.equal(rounds[0]["scales"].view(torch.int32), rounds[2]["scales"].view(torch.int32))

    g, opt, dc = _trained_container()
    n = len(g)
    _, _, full, _ = _expected_round(g, opt, dc, 0)
    dc.max_gaussians = full[0] - 1
    counts = dc.densify_and_prune()
    assert counts == dict(n_out=n - full[1], n_pruned=full[1], n_cloned=0, n_split=0) and len(g) == n - full[1]
    g, opt, dc = _trained_container()
    dc.max_gaussians = full[0]
    assert dc.densify_and_prune()["n_out"] == full[0]


def test_accumulate_allocates_nothing_and_needs_a_grad():
    from intro_to_gaussian_splatting_amd import DensityControl
    from test_hip_adam import _container, _set_grads

    g = _container(300)
    g.points.requires_grad_(True)
    dc = DensityControl(g, **KNOBS)
    with pytest.raises(ValueError, match="points has no .grad"):
        dc.accumulate()
    _set_grads(g, 1, ("points",))
    dc.accumulate()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    dc.accumulate()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(DEV) == before
    want = 2 * g.points.grad.norm(dim=1)
    assert torch.allclose(dc.grad_sum, want, rtol=1e-6) and bool((dc.seen == 2).all())


def test_reset_opacity_clamps_and_zeroes_only_the_opacity_moments():
    g, opt, dc = _trained_container()
    keep = {(key, k): getattr(opt, key)[k].clone() for k in opt.names for key in ("exp_avg", "exp_avg_sq")}
    before = g.opacity.detach().clone()
    assert bool((before > -0.5).any()) and bool((before < -0.5).any())
    dc.reset_opacity(-0.5)
    assert g.opacity.is_leaf and g.opacity.requires_grad
    assert torch.equal(g.opacity.detach(), before.clamp(max=-0.5))
    for (key, k), m in keep.items():
        now = getattr(opt, key)[k]
        assert (not now.any()) if k == "opacity" else torch.equal(now, m), (key, k)
    assert opt.step_count == 2


def test_a_spatially_ordered_container_and_a_foreign_optimiser_are_refused():
    from intro_to_gaussian_splatting_amd import DensityControl, GaussianAdam
    from test_hip_adam import _container

    g = _container(300)
    with pytest.raises(ValueError, match="spatially ordered.*spatially_ordered\\(\\) again"):
        DensityControl(g.spatially_ordered())
    other = _container(300)
    other.points.requires_grad_(True)
    with pytest.raises(ValueError, match="optimizer belongs to another container"):
        DensityControl(g, optimizer=GaussianAdam(other, lr={"points": 1e-3}))


# ---- with a scene: the caches, and a short fit
TRAINED = ("points", "scales", "quaternions", "opacity", "colors")
LR = {"colors": 0.02, "opacity": 0.02, "quaternions": 1e-3, "points": 1e-3, "scales": 5e-3}


def _scene(tmp_path, n=400, size=64, seed=2):
    from intro_to_gaussian_splatting_amd import GaussianScene, Gaussians
    from intro_to_gaussian_splatting_amd.synthetic import make_scene, write_colmap_text

    sc = make_scene(n, size, size, seed=seed, sigma_scale=2.0)
    write_colmap_text(str(tmp_path), sc)
    g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"], device=DEV)
    return GaussianScene(str(tmp_path), g)


def _perturbed_target(scene, seed):
    g = scene.gaussians
    rs = np.random.RandomState(seed)
    noise = lambda t, sigma: torch.from_numpy(rs.normal(0, sigma, size=tuple(t.shape)).astype(np.float32)).to(DEV)  # noqa: E731
    with torch.no_grad():
        keep = {k: getattr(g, k).clone() for k in TRAINED}
        g.colors.add_(noise(g.colors, 0.15)).clamp_(0.0, 1.0)
        g.opacity.add_(noise(g.opacity, 0.5))
        g.points.add_(noise(g.points, 0.02))
        g.scales.mul_(torch.exp(noise(g.scales, 0.1)))
        target = scene.render_image_hip(1).clone()
        for k, v in keep.items():
            getattr(g, k).copy_(v)
    return target


def _quantile_knobs(dc, g):
    """Thresholds from the scene itself: the hottest ~8 % densify (split above their median size), the faintest ~3 % go."""
    mean = dc.grad_sum / dc.seen.clamp(min=1).float()
    dc.grad_threshold = float(torch.quantile(mean[dc.seen > 0], 0.92))
    hot = (dc.seen > 0) & (mean >= dc.grad_threshold)
    dc.dense_scale = float(g.scales.detach().amax(dim=1)[hot].median())
    dc.prune_logit = float(torch.quantile(g.opacity.detach().reshape(-1), 0.03))
    dc.prune_scale = float("inf")


def test_frames_after_a_round_are_those_of_a_fresh_scene(tmp_path):
    from intro_to_gaussian_splatting_amd import DensityControl, GaussianAdam, GaussianScene, Gaussians

    scene = _scene(tmp_path)
    g = scene.gaussians
    target = _perturbed_target(scene, 3)
    for k in TRAINED:
        getattr(g, k).requires_grad_(True)
    opt = GaussianAdam(g, lr=LR)
    dc = DensityControl(g, optimizer=opt, scene=scene)
    for _ in range(3):                  # three frames of the old rows fill the view's caches and hints
        opt.zero_grad()
        scene.photometric_loss(1, scene.render_image_hip(1, geometry_gradients=True), target).backward()
        dc.accumulate()
        opt.step()
    assert scene._cap_hints and scene._kept_hints and len(scene._hints) and scene._instances_hint > 0
    _quantile_knobs(dc, g)
    n = len(g)
    counts = dc.densify_and_prune(generator=torch.Generator(device=DEV).manual_seed(1))
    assert counts["n_out"] != n and min(counts.values()) > 0, counts
    assert not scene._cap_hints and not scene._kept_hints and not scene._n_redo_seen and not len(scene._hints)
    assert scene._instances_hint == 0 and scene._last_instances == 0
    opt.zero_grad()
    frame = scene.render_image_hip(1, geometry_gradients=True)
    scene.photometric_loss(1, frame, target).backward()
    for k in TRAINED:
        t = getattr(g, k)
        assert t.grad is not None and t.grad.shape == t.shape and t.shape[0] == counts["n_out"], k
        assert bool(torch.isfinite(t.grad).all()) and bool(t.grad.any()), k
    fresh_g = Gaussians.from_arrays(g.points.detach().cpu(), g.colors.detach().cpu() * 256, g.scales.detach().cpu(),
                                    g.quaternions.detach().cpu(), g.opacity.detach().cpu(), device=DEV)
    assert torch.equal(fresh_g.colors, g.colors.detach())
    fresh = GaussianScene(str(tmp_path), fresh_g)
    with torch.no_grad():
        assert torch.equal(fresh.render_image_hip(1).view(torch.int32), frame.detach().view(torch.int32))
        assert torch.equal(scene.render_image_hip(1).view(torch.int32), frame.detach().view(torch.int32))      # and the frame after it


def test_a_short_fit_with_one_round_in_the_middle(tmp_path):
    from intro_to_gaussian_splatting_amd import DensityControl, GaussianAdam

    scene = _scene(tmp_path)
    g = scene.gaussians
    target = _perturbed_target(scene, 4)
    for k in TRAINED:
        getattr(g, k).requires_grad_(True)
    opt = GaussianAdam(g, lr=LR, skip_zero_rows=True)
    dc = DensityControl(g, optimizer=opt, scene=scene)
    losses, rows = [], [len(g)]
    for step in range(30):
        opt.zero_grad()
        loss = scene.photometric_loss(1, scene.render_image_hip(1, geometry_gradients=True), target)
        loss.backward()
        dc.accumulate()
        opt.step()
        losses.append(loss.detach())
        if step == 14:
            _quantile_knobs(dc, g)
            counts = dc.densify_and_prune(generator=torch.Generator(device=DEV).manual_seed(2))
            rows.append(len(g))
    losses = [float(v) for v in losses]
    print("short fit: loss first %.6g, before the round %.6g, after it %.6g, last %.6g; rows %d -> %d %s"
          % (losses[0], losses[14], losses[15], losses[-1], rows[0], rows[1], counts))
    assert all(np.isfinite(losses)) and rows[1] != rows[0] and len(g) == rows[1] == counts["n_out"]
    assert losses[-1] < losses[0]
    assert opt.step_count == 30 and bool((g.scales > 0).all())
