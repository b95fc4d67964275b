"""gsx_adam_step on the GPU (csrc/gsx_adam.hip) and GaussianAdam on top of it.

Bits: a LINEAR group's parameter and every group's two moments equal the float32 restatement (tests/adam_restatement.py)
bit for bit, on the 16-byte and the float-by-float path alike.  A LOG group's parameter goes through the device library's
expf and is held to BOUND_KERNEL["log"] = 12 E_REF (tests/test_adam_host.py) against the float64 restatement, in the host
test's error scale lr |p| + t 2^-24 |p|; its distance to the float32 restatement is printed.  A real step against
torch.optim.Adam is held to 12 E_REF of the LINEAR scale lr + t 2^-24 |p|.

Printed on an MI355X:
    LOG parameters, 5 chained steps, all shapes: worst error / scale 3.65e-05 (bound 0.221); worst distance to the float32
      restatement 2 ulp
    a scale of 1e-3, 200 steps of 1e-2: LINEAR ends at -1.999, LOG at 2.407e-4
    one real step against torch.optim.Adam, worst error / scale (bound 0.0959): points 3.73e-05, scales 1.49e-04,
      quaternions 2.38e-04, opacity 2.38e-05, sh 1.19e-05
    training, 30 steps, scales in log space, zero rows skipped: photometric loss 0.060862 -> 0.0126407; 208 of 3000
      Gaussians never had a gradient and carry their starting bits
"""
import ctypes

import numpy as np
import pytest
import torch

import adam_restatement as ar
from test_adam_host import BETAS, BOUND_KERNEL, EPS, error_scale, gradients, start

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 12345.678
GUARD = 64
NAN_BITS = 0x7FC12345


class Group:
    """One group's four arrays on the device, each `lead` floats behind a 64-float guard and in front of another (lead 1:
    every base is off 16-byte alignment by one float), and the restatement's float32 state next to them."""

    def __init__(self, n, width, transform, lr, lead, seed):
        self.n, self.width, self.transform, self.lr, self.lead = n, width, transform, lr, lead
        self.p = start(transform, seed, (n, width))
        self.m = np.zeros((n, width), np.float32)
        self.v = np.zeros((n, width), np.float32)
        self.whole, self.view = {}, {}
        for key in "pgmv":
            w = torch.full((GUARD + lead + n * width + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
            self.whole[key] = w
            self.view[key] = w[GUARD + lead:GUARD + lead + n * width].view(n, width)
        self.upload()

    def upload(self):
        for key, a in (("p", self.p), ("m", self.m), ("v", self.v)):
            self.view[key].copy_(torch.from_numpy(a))

    def set_grad(self, g):
        self.g = np.ascontiguousarray(g, np.float32)
        self.view["g"].copy_(torch.from_numpy(self.g))

    def device(self, key):
        return self.view[key].cpu().numpy()

    def guards_intact(self):
        for w in self.whole.values():
            head, tail = w[:GUARD + self.lead], w[GUARD + self.lead + self.n * self.width:]
            if not (bool((head == SENTINEL).all()) and bool((tail == SENTINEL).all()) and tail.numel() == GUARD):
                return False
        return True


def _call(groups, n, step, flags=0, n_groups=None, betas=BETAS, eps=EPS):
    from intro_to_gaussian_splatting_amd import _ffi

    arr = (_ffi.GsxAdamGroup * max(len(groups), 1))()
    for a, g in zip(arr, groups):
        a.param, a.grad = g.view["p"].data_ptr(), g.view["g"].data_ptr()
        a.exp_avg, a.exp_avg_sq = g.view["m"].data_ptr(), g.view["v"].data_ptr()
        a.width, a.transform, a.lr, a.reserved = g.width, g.transform, g.lr, 0.0
    rc = _ffi.load().gsx_adam_step(arr, len(groups) if n_groups is None else n_groups, n, step, betas[0], betas[1], eps, flags,
                                   ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return rc


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _ulps(a, b):
    """Distance in float32 ulps between two positive float32 arrays."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


WIDTH_SETS = {
    "six": [(1, ar.LINEAR), (3, ar.LOG), (4, ar.LINEAR), (12, ar.LINEAR), (27, ar.LOG), (48, ar.LINEAR)],
    "three": [(3, ar.LINEAR)],
    "eight": [(w, (ar.LOG if w in (2, 5) else ar.LINEAR)) for w in (1, 2, 3, 4, 5, 6, 7, 8)],
}
LR_BITS = 1e-2


def _chain(n, spec, lead, steps=5):
    """`steps` chained calls; asserts the bits and the LOG bound after every one.  Returns the final device arrays per group
    and the worst LOG error / scale and ulp distance met."""
    groups = [Group(n, w, tr, LR_BITS, lead, 10 + i) for i, (w, tr) in enumerate(spec)]
    grads = [gradients(20 + i, steps, (n, w), zeroed=(2, 4)) for i, (w, _) in enumerate(spec)]
    p64 = [g.p.astype(np.float64) for g in groups]
    m64 = [np.zeros_like(p) for p in p64]
    v64 = [np.zeros_like(p) for p in p64]
    worst_e, worst_ulp = 0.0, 0
    for t in range(1, steps + 1):
        for g, gr in zip(groups, grads):
            g.set_grad(gr[t - 1])
        assert _call(groups, n, t) == 0
        for i, g in enumerate(groups):
            # a LOG group's restatement starts every step from the parameter the DEVICE holds: its moments see g p
            p2, m2, v2 = ar.step32(g.p, g.g, g.m, g.v, g.lr, t, BETAS[0], BETAS[1], EPS, g.transform)
            p64[i], m64[i], v64[i] = ar.step64(p64[i], g.g, m64[i], v64[i], g.lr, t, BETAS[0], BETAS[1], EPS, g.transform)
            got_p, got_m, got_v = g.device("p"), g.device("m"), g.device("v")
            assert _same_bits(got_m, m2) and _same_bits(got_v, v2), (n, lead, g.width, t)
            if g.transform == ar.LINEAR:
                assert _same_bits(got_p, p2), (n, lead, g.width, t)
            else:
                assert np.isfinite(got_p).all() and (got_p > 0).all()
                e = float((np.abs(got_p - p64[i]) / error_scale(p64[i], g.lr, t, ar.LOG)).max())
                worst_e, worst_ulp = max(worst_e, e), max(worst_ulp, int(_ulps(got_p, p2).max()))
                assert e <= BOUND_KERNEL["log"], (n, lead, g.width, t, e)
            g.p, g.m, g.v = got_p, m2, v2
            assert g.guards_intact(), (n, lead, g.width, t)
    return [(g.device("p"), g.device("m"), g.device("v")) for g in groups], worst_e, worst_ulp


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_five_chained_steps_equal_the_restatement_bit_for_bit_on_both_paths(n):
    for name, spec in WIDTH_SETS.items():
        aligned, e0, u0 = _chain(n, spec, 0)
        shifted, e1, u1 = _chain(n, spec, 1)
        print("n %d, %s: LOG parameters: worst error / scale %.3g (bound %.3g), worst distance to the float32 restatement %d ulp"
              % (n, name, max(e0, e1), BOUND_KERNEL["log"], max(u0, u1)))
        for a, b in zip(aligned, shifted):
            for x, y in zip(a, b):
                assert _same_bits(x, y), (n, name)


def test_a_ninth_group_is_refused():
    from intro_to_gaussian_splatting_amd import _ffi

    groups = [Group(4, 1, ar.LINEAR, 1e-3, 0, i) for i in range(9)]
    for g in groups:
        g.set_grad(np.ones((4, 1), np.float32))
    assert _call(groups, 4, 1) == _ffi.GSX_ERR_INVALID_ARGUMENT and b"n_groups" in _ffi.load().gsx_last_error()
    for g in groups:
        assert _same_bits(g.device("p"), g.p) and not g.device("m").any()


@pytest.mark.parametrize("step", [1, 10 ** 6])
def test_first_step_and_a_late_step_from_given_moments(step):
    rs = np.random.RandomState(step % 1000)
    groups = [Group(257, w, ar.LINEAR, 3e-3, lead, 40 + w) for w, lead in ((3, 0), (4, 0), (5, 1))]
    for g in groups:
        if step > 1:
            g.m = rs.normal(size=g.p.shape).astype(np.float32)
            g.v = (rs.normal(size=g.p.shape) ** 2).astype(np.float32)
            g.upload()
        g.set_grad(gradients(step % 1000, 1, g.p.shape, zeroed=())[0])
    assert _call(groups, 257, step) == 0
    k = ar.host_scalars(3e-3, BETAS[0], BETAS[1], step)
    if step > 1:
        assert k["s2"] == 1.0 and k["a"] == np.float32(3e-3)        # the bias corrections have run out
    for g in groups:
        p2, m2, v2 = ar.step32(g.p, g.g, g.m, g.v, g.lr, step, BETAS[0], BETAS[1], EPS)
        assert _same_bits(g.device("p"), p2) and _same_bits(g.device("m"), m2) and _same_bits(g.device("v"), v2), g.width
        assert not _same_bits(p2, g.p) and g.guards_intact()


def test_log_space_keeps_a_scale_positive_where_a_linear_step_does_not():
    """The reason for the transform: a scale of 1e-3 under 200 steps of lr 1e-2 along gradients of constant sign."""
    lin, log = Group(300, 3, ar.LINEAR, 1e-2, 0, 1), Group(300, 3, ar.LOG, 1e-2, 0, 1)
    g = np.exp(np.random.RandomState(3).uniform(-3, 3, size=(300, 3))).astype(np.float32)       # all positive: shrink
    for grp in (lin, log):
        grp.p = np.full((300, 3), 1e-3, np.float32)
        grp.upload()
        grp.set_grad(g)
    for t in range(1, 201):
        assert _call([lin, log], 300, t) == 0
    a, b = lin.device("p"), log.device("p")
    print("after 200 steps: linear scales in [%.4g, %.4g], log-space scales in [%.4g, %.4g]" % (a.min(), a.max(), b.min(), b.max()))
    assert np.isfinite(a).all() and (a < 0).all()
    assert np.isfinite(b).all() and (b > 0).all() and (b < 1e-3).all()


# ---- GSX_ADAM_SKIP_ZERO_ROWS
SKIP_SPEC = [(3, ar.LINEAR), (3, ar.LOG), (4, ar.LINEAR), (1, ar.LINEAR), (12, ar.LINEAR)]


@pytest.mark.parametrize("lead", [0, 1])
def test_skip_zero_rows(lead):
    n = 600
    rs = np.random.RandomState(9)
    zero = rs.uniform(size=n) < 0.3
    zero[250:512] = True                # a run over the block boundary 255 | 256 | 257, and the whole of block 1
    zero[[10, 20, 513]] = False
    one_group_only, nan_row = 10, 20
    nan_pattern = np.full(1, NAN_BITS, np.uint32).view(np.float32)[0]

    def make():
        groups = [Group(n, w, tr, 1e-2, lead, 60 + i) for i, (w, tr) in enumerate(SKIP_SPEC)]
        for i, g in enumerate(groups):
            r = np.random.RandomState(70 + i)
            gr = gradients(80 + i, 1, (n, g.width), zeroed=())[0]
            gr[zero] = 0.0
            gr[zero & (np.arange(n) % 2 == 1)] = -0.0           # -0.0 counts as zero
            if i != 4:
                gr[one_group_only] = 0.0                        # zero in four groups, non-zero in the fifth
            gr[nan_row] = 0.0
            if i == 2:
                gr[nan_row, 1] = np.nan                         # a NaN is not zero
            g.m = r.normal(size=g.p.shape).astype(np.float32)
            g.v = (r.normal(size=g.p.shape) ** 2).astype(np.float32)
            g.m[zero], g.v[zero] = nan_pattern, nan_pattern     # an untouched row is provable
            g.upload()
            g.set_grad(gr)
        return groups

    dense, sparse = make(), make()
    assert np.signbit(sparse[0].g[zero]).any() and not np.signbit(sparse[0].g[zero]).all()
    live = ar.live_rows([g.g for g in sparse])
    assert np.array_equal(live, ~zero) and live[one_group_only] and live[nan_row] and not live[250:512].any()
    assert _call(dense, n, 7) == 0
    assert _call(sparse, n, 7, flags=1) == 0
    for d, s in zip(dense, sparse):
        for key, before in (("p", s.p), ("m", s.m), ("v", s.v)):
            got, want = s.device(key), d.device(key)
            assert _same_bits(got[zero], before[zero]), (s.width, key)          # skipped: the bits they had
            assert _same_bits(got[live], want[live]), (s.width, key)            # the others: the dense call's bits
        assert (s.device("m")[zero].view(np.uint32) == NAN_BITS).all()
        assert not _same_bits(s.device("m")[one_group_only], s.m[one_group_only]), s.width   # updated in ALL groups
        assert s.guards_intact() and d.guards_intact()
        # and the dense call is the restatement's (moments everywhere, the parameter of the LINEAR groups)
        p2, m2, v2 = ar.step32(d.p, d.g, d.m, d.v, d.lr, 7, BETAS[0], BETAS[1], EPS, d.transform)
        finite = live & ~(np.arange(n) == nan_row)
        assert _same_bits(d.device("m")[finite], m2[finite]) and _same_bits(d.device("v")[finite], v2[finite])
        if d.transform == ar.LINEAR:
            assert _same_bits(d.device("p")[finite], p2[finite])
    assert np.isnan(sparse[2].device("p")[nan_row, 1]) and np.isfinite(sparse[0].device("p")[nan_row]).all()


# ---- GaussianAdam
def _container(n=700, seed=4):
    from intro_to_gaussian_splatting_amd import Gaussians

    rs = np.random.RandomState(seed)
    q = rs.normal(size=(n, 4))
    return Gaussians.from_arrays(rs.normal(size=(n, 3)).astype(np.float32), rs.uniform(0, 255, size=(n, 3)),
                                 np.exp(rs.normal(-3, 0.5, size=(n, 3))).astype(np.float32),
                                 (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32),
                                 rs.normal(size=(n, 1)).astype(np.float32), device=DEV)


NAMES5 = ("points", "scales", "quaternions", "opacity", "colors")
LR5 = {"points": 1e-3, "scales": 5e-3, "quaternions": 1e-3, "opacity": 2e-2, "colors": 2e-2}


def _set_grads(g, seed, names=NAMES5):
    rs = np.random.RandomState(seed)
    for name in names:
        t = getattr(g, name)
        t.grad = torch.from_numpy(rs.normal(size=tuple(t.shape)).astype(np.float32)).to(DEV)


def _snapshot(g, names=NAMES5):
    return {name: getattr(g, name).detach().clone() for name in names}


def test_step_is_deterministic_allocates_nothing_and_bumps_versions():
    from intro_to_gaussian_splatting_amd import GaussianAdam

    results = []
    for _ in range(2):
        g = _container()
        for name in NAMES5:
            getattr(g, name).requires_grad_(True)
        opt = GaussianAdam(g, lr=LR5)
        assert opt.names == NAMES5 and opt.log_groups == ("scales",)
        for t in range(3):
            _set_grads(g, 100 + t)
            versions = {name: getattr(g, name)._version for name in NAMES5}
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated(DEV)
            assert opt.step() is None
            torch.cuda.synchronize()
            assert torch.cuda.memory_allocated(DEV) == before
            for name in NAMES5:
                assert getattr(g, name)._version > versions[name], name
        assert bool((g.scales > 0).all())
        results.append((_snapshot(g), {k: v.clone() for k, v in opt.exp_avg.items()}, {k: v.clone() for k, v in opt.exp_avg_sq.items()}))
        opt.zero_grad()
        assert all(getattr(g, name).grad is None for name in NAMES5)
    for a, b in zip(results[0], results[1]):
        for name in NAMES5:
            assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name


def test_step_refuses_a_missing_or_unfit_grad_by_name():
    from intro_to_gaussian_splatting_amd import GaussianAdam

    g = _container(50)
    g.points.requires_grad_(True)
    g.opacity.requires_grad_(True)
    opt = GaussianAdam(g, lr={"points": 1e-3, "opacity": 1e-2})
    _set_grads(g, 1, ("points",))
    with pytest.raises(ValueError, match="opacity has no .grad"):
        opt.step()
    g.opacity.grad = torch.zeros((50, 2), device=DEV)[:, :1]
    assert not g.opacity.grad.is_contiguous()
    with pytest.raises(ValueError, match="opacity.grad must be contiguous"):
        opt.step()
    assert opt.step_count == 0


def test_boxes_of_a_spatially_ordered_container_follow_a_step():
    from intro_to_gaussian_splatting_amd import GaussianAdam

    g = _container().spatially_ordered()
    g.points.requires_grad_(True)
    g.scales.requires_grad_(True)
    before = g.current_block_bounds().clone()
    opt = GaussianAdam(g, lr={"points": 1e-2, "scales": 1e-2})
    _set_grads(g, 5, ("points", "scales"))
    opt.step()
    after = g.current_block_bounds().clone()
    g.refresh_block_bounds()
    assert torch.equal(after, g.block_bounds) and not torch.equal(after, before)


def test_state_dict_round_trip_continues_with_the_same_bits_and_a_callable_rate_is_honoured():
    from intro_to_gaussian_splatting_amd import GaussianAdam

    g = _container()
    for name in NAMES5:
        getattr(g, name).requires_grad_(True)
    rate = lambda step: 1e-2 if step != 4 else 0.0      # noqa: E731
    lr = dict(LR5, points=rate)
    opt = GaussianAdam(g, lr=lr, skip_zero_rows=True)
    for t in range(3):
        _set_grads(g, 200 + t)
        opt.step()
    state, kept = opt.state_dict(), _snapshot(g)
    assert state["step"] == 3 and state["log_groups"] == ("scales",) and "points" not in state["lr"]

    def two_more(o):
        out = []
        for t in range(3, 5):
            _set_grads(g, 200 + t)
            o.step()
            out.append(_snapshot(g))
        return out, {k: v.clone() for k, v in o.exp_avg_sq.items()}

    first, sq_first = two_more(opt)
    assert torch.equal(first[0]["points"], kept["points"])                  # step 4: the callable said 0
    assert not torch.equal(first[0]["scales"], kept["scales"]) and not torch.equal(first[1]["points"], kept["points"])
    with torch.no_grad():
        for name in NAMES5:
            getattr(g, name).copy_(kept[name])
    again = GaussianAdam(g, lr=lr, betas=(0.5, 0.5), eps=1e-3, log_groups=())
    again.load_state_dict(state)
    assert again.step_count == 3 and again.log_groups == ("scales",) and again.betas == opt.betas and again.skip_zero_rows
    second, sq_second = two_more(again)
    for a, b in zip(first, second):
        for name in NAMES5:
            assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name
    for name in NAMES5:
        assert torch.equal(sq_first[name].view(torch.int32), sq_second[name].view(torch.int32)), name


# ---- one real step, and training (the scene and rates of test_hip_geometry_backward_edges' training test)
TRAINED = ("points", "scales", "quaternions", "opacity", "sh")
LR = {"sh": 0.02, "opacity": 0.02, "quaternions": 1e-3, "points": 1e-4, "scales": 1e-4}


def _perturbed_target(scene, seed):
    """The frame of the scene with noise on the coefficients (0.2), the quaternions (0.1), the points (0.01) and, by a factor
    exp(N(0, 0.1)), the scales."""
    g = scene.gaussians
    rs = np.random.RandomState(seed)
    noise = lambda t, sigma: torch.from_numpy(rs.normal(0, sigma, size=tuple(t.shape)).astype(np.float32)).to(DEV)  # noqa: E731
    with torch.no_grad():
        keep = {k: getattr(g, k).clone() for k in ("sh", "quaternions", "points", "scales")}
        g.sh.add_(noise(g.sh, 0.2))
        g.quaternions.add_(noise(g.quaternions, 0.1))
        g.points.add_(noise(g.points, 0.01))
        g.scales.mul_(torch.exp(noise(g.scales, 0.1)))
        target = scene.render_image_hip(1).clone()
        for k, v in keep.items():
            getattr(g, k).copy_(v)
    return target


def _training_scene(tmp_path):
    from test_hip_sh_backward import _sh_scene

    scene, _ = _sh_scene(tmp_path, 2)
    target = _perturbed_target(scene, 5)
    for k in TRAINED:
        getattr(scene.gaussians, k).requires_grad_(True)
    return scene, target


def test_one_real_step_agrees_with_torch_adam(tmp_path):
    from intro_to_gaussian_splatting_amd import GaussianAdam

    scene, target = _training_scene(tmp_path)
    g = scene.gaussians
    scene.photometric_loss(1, scene.render_image_hip(1, geometry_gradients=True), target).backward()
    clones = {k: getattr(g, k).detach().clone().requires_grad_(True) for k in TRAINED}
    for k in TRAINED:
        clones[k].grad = getattr(g, k).grad.clone()
        assert getattr(g, k).grad.abs().max() > 0, k
    torch.optim.Adam([dict(params=[clones[k]], lr=LR[k]) for k in TRAINED]).step()
    before = _snapshot(g, TRAINED)
    GaussianAdam(g, lr=LR, log_groups=()).step()
    for k in TRAINED:
        got, want = getattr(g, k).detach().double().cpu().numpy(), clones[k].detach().double().cpu().numpy()
        assert not torch.equal(getattr(g, k).detach(), before[k]), k
        e = float((np.abs(got - want) / error_scale(want, LR[k], 1, ar.LINEAR)).max())
        print("one real step, %s: worst error / scale against torch.optim.Adam %.3g (bound %.3g)" % (k, e, BOUND_KERNEL["linear"]))
        assert e <= BOUND_KERNEL["linear"], (k, e)
    for k in TRAINED:
        getattr(g, k).requires_grad_(False)


def test_training_in_log_space_with_zero_rows_skipped(tmp_path):
    from intro_to_gaussian_splatting_amd import GaussianAdam

    scene, target = _training_scene(tmp_path)
    g = scene.gaussians
    begin = _snapshot(g, TRAINED)
    opt = GaussianAdam(g, lr=LR, log_groups=("scales",), skip_zero_rows=True)
    ever = torch.zeros(len(g), dtype=torch.bool, device=DEV)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = scene.photometric_loss(1, scene.render_image_hip(1, geometry_gradients=True), target)
        loss.backward()
        for k in TRAINED:
            ever |= (getattr(g, k).grad.reshape(len(g), -1) != 0).any(dim=1)        # (NaN != 0 and -0.0 == 0, as the kernel has it)
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in losses]
    never = ~ever
    print("photometric loss, scales in log space, zero rows skipped: first %.6g, last %.6g; %d of %d Gaussians never had a gradient"
          % (losses[0], losses[-1], int(never.sum()), len(g)))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert bool((g.scales > 0).all()) and bool(torch.isfinite(g.scales).all())
    assert int(never.sum()) > 0 and int(ever.sum()) > 0
    for k in TRAINED:
        now = getattr(g, k).detach()
        assert torch.equal(now[never].view(torch.int32), begin[k][never].view(torch.int32)), k
        assert not torch.equal(now[ever], begin[k][ever]), k
        assert not opt.exp_avg[k][never].any() and not opt.exp_avg_sq[k][never].any(), k
        getattr(g, k).requires_grad_(False)
