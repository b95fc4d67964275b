"""Fixed-budget densification without a GPU: the relocation formula against ``decimal`` at 50 digits, the plan's restatement
against its definition, every refusal of the C ABI by name (before any HIP call), the Python surface's ValueErrors, the
event mapping of ``Trainer(strategy="mcmc")``, the workspace carve under the sanitizers (tests/host/plan_mcmc_sanitize.cpp),
and the float32 reference errors E_REF_REGULARIZE / E_REF_PERTURB the GPU test's bounds are built from.

E_REF_*: the float32 mirrors of tests/mcmc_restatement.py (the kernels' operation order, numpy's float32 exp) against its
float64 restatement, worst over ``step_inputs(n)`` for n in STEP_SIZES under STEP_RULES (lambda 0.01 both, rate 80, gate 100
/ 0.995) -- the inputs tests/test_hip_mcmc.py runs.  The normalisation is fixed here, before any GPU run:
    regularize  |grad' - float64| in units of the regulariser's own coefficient, lambda / n (opacity) or lambda / (3 n)
                (scales), the larger of the two sides;
    perturb     |delta - float64 delta| in units of rate * max_c s_c^2 * |eps|_2 of the row (rows whose delta is not finite
                keep their bits and are compared as bits).  The kernel's POINT is then held to
                12 E_REF_PERTURB * that unit + one float32 ulp of the point, the ulp for the final addition.
Measured on the CPU:
    E_REF_REGULARIZE  1.906e-07   (step_inputs(1000): the rounding of the sum g + c f with |g| of a few c, and of c itself)
    E_REF_PERTURB     6.259e-07   (step_inputs(1000): the gate multiplies the rounding of 1 - sigma by gate_k = 100)
The kernels are held to 12 x these (tests/test_hip_mcmc.py), the project's multiple for a float32 kernel with the device's
exp over its numpy mirror.  numpy's float32 exp may differ between CPUs: the test accepts a factor of 1.5 either way, as
tests/test_photometric_loss_host.py does, and the bounds are built from the RECORDED figures.
"""
import ctypes
import decimal
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import mcmc_restatement as mr

E_REF_REGULARIZE = 1.906e-07
E_REF_PERTURB = 6.259e-07
MIN_OPACITY = 0.005


# ---- the relocation formula
def _decimal_relocation(a, N):
    """(x, D) at 50 digits from the float64 a: x = 1 - (1 - a)^(1/N), D the double sum of the issue."""
    decimal.getcontext().prec = 50
    a = decimal.Decimal(a)
    one = decimal.Decimal(1)
    x = one - ((one - a).ln() / N).exp()
    D = decimal.Decimal(0)
    for i in range(1, N + 1):
        for k in range(i):
            D += math.comb(i - 1, k) * (-1) ** k * x ** (k + 1) / decimal.Decimal(k + 1).sqrt()
    return x, D


@pytest.mark.parametrize("N", [1, 2, 3, 12, 24, 51])
@pytest.mark.parametrize("a", [MIN_OPACITY, 0.5, 0.99, 1.0 - 2.0 ** -24])
def test_relocation_in_float64_against_decimal(a, N):
    x, D, coeff = mr.relocation(a, N)
    xd, Dd = _decimal_relocation(a, N)
    rel_x = abs(float((decimal.Decimal(x) - xd) / xd))
    rel_D = abs(float((decimal.Decimal(D) - Dd) / Dd))
    print("a = %.9g, N = %d: x rel %.3g, D rel %.3g, coeff %.17g" % (a, N, rel_x, rel_D, coeff))
    assert rel_D < 1e-8 and rel_x < 1e-12
    assert abs(coeff - float(decimal.Decimal(a) / Dd)) <= 1e-8 * coeff
    if N == 1:
        assert abs(coeff - 1.0) <= 4 * 2.0 ** -52 and abs(x - a) <= 4 * 2.0 ** -52 * a


def test_relocation_clamps_a_saturated_sigmoid_and_keeps_the_composite():
    """a = 1 exactly (a float32 sigmoid that saturated) is evaluated at 1 - 2^-24; N copies of opacity x composite to a."""
    assert mr.relocation(1.0, 51) == mr.relocation(mr.TOP, 51)
    for a in (0.01, 0.5, 0.99):
        for N in (2, 7, 51):
            x, D, coeff = mr.relocation(a, N)
            assert abs((1.0 - (1.0 - x) ** N) - a) < 1e-12 and 0.0 < coeff <= 1.0 and D > 0.0
    lo, _ = mr.relocated(np.float32(-5.0), 51, MIN_OPACITY)        # x far below min_opacity: clamped up to it
    assert lo == np.float32(math.log(float(np.float32(MIN_OPACITY)) / (1.0 - float(np.float32(MIN_OPACITY)))))


# ---- the plan's restatement against its definition
def plan_case(n, n_out, seed=0):
    """(opacity float32 (n), dead_logit float32, uniforms float64 (n_out)): logits around the threshold, with rows exactly
    at dead_logit, one ulp either side, +-inf, NaN and logits of 20 (sigma saturates in float32) where n allows."""
    rs = np.random.RandomState(9000 + 31 * seed + n + n_out)
    dead_logit = np.float32(math.log(MIN_OPACITY / (1.0 - MIN_OPACITY)))
    o = rs.normal(-3.0, 3.0, size=n).astype(np.float32)
    special = [dead_logit, np.nextafter(dead_logit, np.float32(0)), np.nextafter(dead_logit, np.float32(-100)), np.float32(np.inf),
               np.float32(-np.inf), np.float32(np.nan), np.float32(20.0), np.float32(20.0)]
    if n >= 16:
        at = rs.permutation(n)[:len(special)]
        o[at] = special
        o[n - 1] = np.float32(1.5)              # the last row is alive: the search's last block has weight
    elif n == 2:
        o[:] = (dead_logit, 20.0)
    else:
        o[:] = 0.25
    return o, dead_logit, rs.random_sample(n_out)


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 3000])
def test_plan_restatement_meets_its_definition(n):
    for n_out in sorted({n, n + 1, int(math.floor(1.05 * n))}):
        o, dead_logit, u = plan_case(n, n_out)
        w = mr.weights_of(o, dead_logit)
        source, count, (n_dead, n_live, n_new), draws = mr.plan(w, o, dead_logit, n_out, u)
        P = np.concatenate([[0], np.cumsum(w.astype(np.uint64))]).astype(np.uint64)
        total = int(P[-1])
        dead = mr.dead_rows(o, dead_logit)
        assert (w[dead] == 0).all() and (w[~np.isfinite(o)] == 0).all() and (w[np.isfinite(o) & ~dead] >= 1).all()
        assert w.max() <= 2 ** 22 and total > 0
        drawn = [j for j in range(n_out) if j >= n or dead[j]]
        assert [d[0] for d in draws] == drawn and int(count.sum()) == len(drawn)
        for j, t, s in draws:
            assert 0 <= t < total and int(P[s]) <= t < int(P[s]) + int(w[s]) and w[s] > 0 and source[j] == s
        kept = np.setdiff1d(np.arange(n_out), drawn)
        assert (source[kept] == kept).all()
        assert np.array_equal(count, np.bincount(source[drawn], minlength=n).astype(np.uint32))
        assert (n_dead, n_live, n_new) == (int(dead.sum()), int((w > 0).sum()), n_out - n)


def test_plan_restatement_of_nothing_alive_and_of_the_ends_of_the_range():
    o = np.full(7, -9.0, np.float32)
    source, count, counts, draws = mr.plan(mr.weights_of(o, -5.0), o, -5.0, 9, np.full(9, 0.5))
    assert list(source) == [0, 1, 2, 3, 4, 5, 6, 6, 6] and not count.any() and counts == (7, 0, 2) and not draws
    o = np.array([-9.0, 0.0, -9.0, 0.0], np.float32)       # u = 0 draws the first live row, the largest u below 1 the last
    w = mr.weights_of(o, -5.0)
    source, count, _, _ = mr.plan(w, o, -5.0, 4, np.array([0.0, 0.3, np.nextafter(1.0, 0.0), 0.3]))
    assert list(source) == [1, 1, 3, 3] and list(count) == [0, 1, 0, 1]


# ---- C ABI
WS, PTR = 1 << 20, 4096           # a 256-byte aligned "workspace" and "arrays": never dereferenced


def test_header_declares_and_ffi_binds():
    import re

    import test_cabi
    from intro_to_gaussian_splatting_amd import _ffi

    hdr = open(os.path.join(ROOT, "include", "gsx.h")).read()
    declared = test_cabi._declared_functions()
    for name, n_args in (("gsx_mcmc_regularize", 8), ("gsx_mcmc_perturb", 10), ("gsx_mcmc_workspace_bytes", 1),
                         ("gsx_mcmc_plan", 12), ("gsx_mcmc_apply", 8)):
        assert re.search(r"GSX_API\s+\w+\s+%s\(" % name, hdr) and name in declared, name
        assert len(_ffi.SIGNATURES[name][1]) == n_args, name
        assert hasattr(_ffi.load(), name)
    for name in ("GSX_MCMC_N_MAX", "GSX_MCMC_COPY", "GSX_MCMC_ZERO_MOVED", "GSX_MCMC_OPACITY", "GSX_MCMC_SCALES"):
        m = re.search(r"\b%s\s*=?\s*(\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(_ffi, name), name
    assert (mr.COPY, mr.ZERO_MOVED, mr.OPACITY, mr.SCALES, mr.N_MAX) == (0, 1, 2, 3, 51)
    assert _ffi.load().gsx_version() == 305                     # untouched
    mk = open(os.path.join(ROOT, "intro_to_gaussian_splatting_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bgsx_mcmc\b", mk, flags=re.M)


def test_workspace_bytes_is_monotone_and_zero_on_bad_arguments():
    from intro_to_gaussian_splatting_amd import _ffi

    f = _ffi.load().gsx_mcmc_workspace_bytes
    sizes = [f(n) for n in (0, 1, 1023, 1024, 1025, 262144, 262145, 10 ** 6, 2 ** 30)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert sizes[-1] >= 4 * 2 ** 30            # a prefix word per row
    assert f(-1) == 0 and f(2 ** 30 + 1) == 0 and f(-2 ** 40) == 0


def test_regularize_and_perturb_refusals_name_the_argument_and_need_no_gpu():
    from intro_to_gaussian_splatting_amd import _ffi

    lib = _ffi.load()
    nan, inf = float("nan"), float("inf")

    def reg(opacity=PTR, scales=PTR, n=100, lo=0.01, ls=0.01, go=PTR, gs=PTR):
        return lib.gsx_mcmc_regularize(opacity, scales, n, lo, ls, go, gs, None)

    for kw, word in ((dict(opacity=None), b"opacity is NULL"), (dict(go=None), b"grad_opacity"), (dict(scales=None), b"scales is NULL"),
                     (dict(gs=None), b"grad_scales"), (dict(n=-1), b"n = -1"), (dict(n=2 ** 30 + 1), b"n = "),
                     (dict(lo=-1.0), b"lambda_opacity"), (dict(lo=nan), b"lambda_opacity"), (dict(ls=inf), b"lambda_scale"),
                     (dict(ls=-0.5), b"lambda_scale")):
        assert reg(**kw) == _ffi.GSX_ERR_INVALID_ARGUMENT, kw
        assert word in lib.gsx_last_error(), (kw, lib.gsx_last_error())
    assert reg(n=0) == _ffi.GSX_OK and reg(n=0, opacity=None, scales=None, go=None, gs=None) == _ffi.GSX_OK
    # a lambda of 0: its side's pointers are not looked at; with both 0 nothing is launched
    assert reg(lo=0.0, ls=0.0, opacity=None, scales=None, go=None, gs=None) == _ffi.GSX_OK

    def per(points=PTR, scales=PTR, quats=PTR, opacity=PTR, noise=PTR, n=100, rate=80.0, k=100.0, x0=0.995):
        return lib.gsx_mcmc_perturb(points, scales, quats, opacity, noise, n, rate, k, x0, None)

    for kw, word in ((dict(points=None), b"points"), (dict(scales=None), b"scales"), (dict(quats=None), b"quaternions"),
                     (dict(opacity=None), b"opacity"), (dict(noise=None), b"noise"), (dict(n=-1), b"n = -1"),
                     (dict(n=2 ** 30 + 1), b"n = "), (dict(rate=-1.0), b"rate"), (dict(rate=nan), b"rate"), (dict(rate=inf), b"rate"),
                     (dict(k=-1.0), b"gate_k"), (dict(k=nan), b"gate_k"), (dict(x0=nan), b"gate_x0"), (dict(x0=inf), b"gate_x0")):
        assert per(**kw) == _ffi.GSX_ERR_INVALID_ARGUMENT, kw
        assert word in lib.gsx_last_error(), (kw, lib.gsx_last_error())
    assert per(n=0) == _ffi.GSX_OK and per(n=0, points=None, noise=None) == _ffi.GSX_OK


def test_plan_refusals_name_the_argument_and_need_no_gpu():
    from intro_to_gaussian_splatting_amd import _ffi

    lib = _ffi.load()
    big = lib.gsx_mcmc_workspace_bytes(100)
    counts = (ctypes.c_int64 * 3)(7, 7, 7)

    def plan(opacity=PTR, n=100, dead=-5.3, n_out=105, u=PTR, w=PTR, source=PTR, count=PTR, ws=WS, ws_bytes=big, out=counts):
        return lib.gsx_mcmc_plan(opacity, n, dead, n_out, u, w, source, count, ws, ws_bytes, out, None)

    for kw, word in ((dict(opacity=None), b"opacity"), (dict(u=None), b"uniforms"), (dict(w=None), b"weights"),
                     (dict(source=None), b"source"), (dict(count=None), b"count is"), (dict(n=-1), b"n = -1"),
                     (dict(n=2 ** 30 + 1), b"n = "), (dict(n_out=99), b"n_out"), (dict(n_out=2 ** 30 + 1), b"n_out"),
                     (dict(dead=float("nan")), b"dead_logit"), (dict(ws=None), b"workspace"), (dict(ws=WS + 128), b"256-byte aligned"),
                     (dict(out=None), b"counts_host"), (dict(n=0, n_out=1), b"n_out")):
        assert plan(**kw) == _ffi.GSX_ERR_INVALID_ARGUMENT, kw
        assert word in lib.gsx_last_error(), (kw, lib.gsx_last_error())
    assert plan(ws_bytes=big - 1) == _ffi.GSX_ERR_WORKSPACE_TOO_SMALL and b"gsx_mcmc_workspace_bytes" in lib.gsx_last_error()
    assert list(counts) == [7, 7, 7]
    assert plan(n=0, n_out=0, ws_bytes=lib.gsx_mcmc_workspace_bytes(0)) == _ffi.GSX_OK and list(counts) == [0, 0, 0]


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
    O, S, C, Z = (1, mr.OPACITY), (3, mr.SCALES), (48, mr.COPY), (4, mr.ZERO_MOVED)
    full = [O, S, C, Z]

    def apply(spec=full, n_groups=None, n=100, n_out=105, source=PTR, count=PTR, min_opacity=0.005, groups=False, **last):
        arr = _groups(spec, **last) if groups is False else groups
        return lib.gsx_mcmc_apply(arr, len(spec) if n_groups is None else n_groups, n, n_out, source, count, min_opacity, None)

    bad = [(dict(groups=None), b"groups is NULL"), (dict(n_groups=0), b"n_groups"), (dict(n_groups=25), b"n_groups"),
           (dict(n=-1), b"n = -1"), (dict(n=2 ** 30 + 1), b"n = "), (dict(n_out=99), b"n_out"), (dict(n_out=2 ** 30 + 1), b"n_out"),
           (dict(min_opacity=0.0), b"min_opacity"), (dict(min_opacity=1.0), b"min_opacity"), (dict(min_opacity=float("nan")), b"min_opacity"),
           (dict(width=0), b"groups[3].width"), (dict(width=2 ** 20 + 1), b"groups[3].width"),
           (dict(role=4), b"groups[3].role"), (dict(role=-1), b"groups[3].role"),
           (dict(src=None), b"groups[3].src"), (dict(dst=None), b"groups[3].dst"), (dict(dst=PTR * 7), b"groups[3].dst equals src"),
           (dict(spec=full + [O]), b"second OPACITY"), (dict(spec=full + [S]), b"second SCALES"),
           (dict(spec=[C, (3, mr.OPACITY)]), b"groups[1].width = 3: a OPACITY group has width 1"),
           (dict(spec=[O, (4, mr.SCALES)]), b"a SCALES group has width 3"),
           (dict(spec=[S, C]), b"SCALES group needs an OPACITY"),
           (dict(source=None), b"source is NULL"), (dict(count=None), b"count is NULL")]
    for kw, word in bad:
        assert apply(**kw) == _ffi.GSX_ERR_INVALID_ARGUMENT, kw
        assert word in lib.gsx_last_error(), (kw, lib.gsx_last_error())
    # nothing to do: no pointer is looked at, but the descriptors are still checked
    assert apply(n=0, n_out=0, source=None, count=None) == _ffi.GSX_OK and apply(n=0, n_out=0, spec=[C] * 24) == _ffi.GSX_OK
    assert apply(n=0, n_out=0, role=7) == _ffi.GSX_ERR_INVALID_ARGUMENT


# ---- the workspace carve under the sanitizers
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_plan_mcmc_carve_under_sanitizers(tmp_path):
    exe = str(tmp_path / "plan_mcmc_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "intro_to_gaussian_splatting_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "plan_mcmc_sanitize.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.startswith("ok:")
    # the library's own answer is the carve's
    from intro_to_gaussian_splatting_amd import _ffi

    for line in run.stdout.splitlines()[1:]:
        n, total = (int(v) for v in line.split())
        assert _ffi.load().gsx_mcmc_workspace_bytes(n) == total, line


# ---- Python surface, as far as it goes without a GPU
def test_python_surface_refusals_by_name():
    from intro_to_gaussian_splatting_amd import Gaussians, GaussianScene, MCMCControl

    g = Gaussians(torch.zeros((4, 3)), torch.zeros((4, 3)), device="cpu")
    with pytest.raises(ValueError, match="cap_max is required"):
        MCMCControl(g)
    with pytest.raises(ValueError, match="cap_max = 3 is below the 4 Gaussians"):
        MCMCControl(g, cap_max=3)
    with pytest.raises(ValueError, match="cap_max = 4.5 is not an integer"):
        MCMCControl(g, cap_max=4.5)
    with pytest.raises(ValueError, match="points is on cpu.*no CPU fallback"):
        MCMCControl(g, cap_max=8)

    class Opt:
        gaussians = Gaussians(torch.zeros((4, 3)), torch.zeros((4, 3)), device="cpu")

    class Scene:
        gaussians = Opt.gaussians

    with pytest.raises(ValueError, match="optimizer belongs to another container"):
        MCMCControl(g, optimizer=Opt(), cap_max=8)
    with pytest.raises(ValueError, match="scene renders another container"):
        MCMCControl(g, scene=Scene(), cap_max=8)
    for kw, match in ((dict(min_opacity=0.0), "min_opacity"), (dict(min_opacity=1.0), "min_opacity"), (dict(growth=0.9), "growth"),
                      (dict(growth=float("inf")), "growth"), (dict(noise_lr=-1.0), "noise_lr"), (dict(lambda_opacity=-1e-3), "lambda_opacity"),
                      (dict(lambda_scale=float("nan")), "lambda_scale"), (dict(gate_k=-1.0), "gate_k"), (dict(gate_x0=float("nan")), "gate_x0")):
        with pytest.raises(ValueError, match=match):
            MCMCControl(g, cap_max=8, **kw)
    ordered = Gaussians(torch.rand((8, 3)), torch.zeros((8, 3)), device="cpu").spatially_ordered()
    with pytest.raises(ValueError, match="spatially ordered.*call spatially_ordered\\(\\) again"):
        MCMCControl(ordered, cap_max=8)
    assert callable(GaussianScene.gaussians_changed)
    doc = MCMCControl.__doc__
    assert "draws twice" in doc and "skip_zero_rows" in doc and "photometric" in doc


def test_n_out_is_host_arithmetic():
    from intro_to_gaussian_splatting_amd import MCMCControl

    mc = MCMCControl.__new__(MCMCControl)
    mc.cap_max, mc.growth, mc.min_opacity = 2600, 1.05, MIN_OPACITY
    assert [mc.n_out_for(n) for n in (1, 19, 20, 2000, 2476, 2477, 2600)] == [1, 19, 21, 2100, 2599, 2600, 2600]
    assert abs(mc.dead_logit - math.log(0.005 / 0.995)) < 1e-15


def test_trainer_strategy_arguments_and_event_mapping(tmp_path):
    import inspect

    from intro_to_gaussian_splatting_amd import Gaussians, GaussianScene, Trainer, events_at
    from intro_to_gaussian_splatting_amd import fit
    from intro_to_gaussian_splatting_amd.synthetic import make_scene, write_colmap_text

    p = inspect.signature(Trainer.__init__).parameters
    assert p["strategy"].default == "adaptive" and p["mcmc"].default is None and p["opacity_reset_every"].default == 3000
    sc = make_scene(8, 32, 32, seed=0)
    write_colmap_text(str(tmp_path), sc)
    g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"], device="cpu")
    scene = GaussianScene(str(tmp_path), g)
    targets = {1: torch.zeros((32, 32, 3))}
    ok = dict(strategy="mcmc", mcmc=dict(cap_max=16))
    for kw, match in ((dict(strategy="greedy"), "strategy = 'greedy'"),
                      (dict(ok, density=dict(grad_threshold=1e-4)), "density= goes to DensityControl"),
                      (dict(ok, statistic="screen"), "statistic= is the adaptive"),
                      (dict(ok, opacity_reset_every=3000), "opacity_reset_every cannot be combined"),
                      (dict(ok, opacity_reset_every=None), "opacity_reset_every cannot be combined"),
                      (dict(strategy="mcmc"), "needs mcmc=dict\\(cap_max"),
                      (dict(strategy="mcmc", mcmc=dict(growth=1.1)), "needs mcmc=dict\\(cap_max"),
                      (dict(mcmc=dict(cap_max=16)), "mcmc= goes to MCMCControl")):
        with pytest.raises(ValueError, match=match):
            Trainer(scene, targets, **kw)
    assert not g.points.requires_grad          # refused before anything was touched
    with pytest.raises(ValueError, match="points is on cpu.*no CPU fallback"):      # good ones get as far as the optimiser
        Trainer(scene, targets, **ok)

    # the event mapping: events_at unchanged, "densify" where it was, "opacity_reset" never
    t = Trainer.__new__(Trainer)
    periods = dict(sh_degree_every=4, densify_from=3, densify_every=5, densify_until=30)
    t._schedule = dict(periods, opacity_reset_every=None)
    for step in range(1, 41):
        assert t.events_at(step) == events_at(step, opacity_reset_every=None, **periods)
        assert t.events_at(step) == tuple(e for e in events_at(step, opacity_reset_every=6, **periods) if e != "opacity_reset")
    assert fit.STRATEGIES == ("adaptive", "mcmc")


# ---- the float32 reference errors
def _measure():
    worst = {"regularize": (0.0, None), "perturb": (0.0, None)}
    R = mr.STEP_RULES
    for n in mr.STEP_SIZES:
        c = mr.step_inputs(n)
        go, gs = mr.regularize_f32(c["opacity"], c["scales"], c["grad_opacity"], c["grad_scales"], R["lambda_opacity"], R["lambda_scale"])
        e = mr.regularize_error(go, gs, c, R["lambda_opacity"], R["lambda_scale"])
        if e > worst["regularize"][0]:
            worst["regularize"] = (e, n)
        args = (c["points"], c["scales"], c["quats"], c["opacity"], c["noise"], R["rate"], R["gate_k"], R["gate_x0"])
        _, d32, kept32 = mr.perturb_f32(*args)
        _, d64, kept64 = mr.perturb_f64(*args)
        assert np.array_equal(kept32, kept64) and kept64.sum() == (2 if n >= 5 else 0)
        unit = mr.perturb_norm(c["scales"], c["noise"], R["rate"])
        live = ~kept64
        e = float((np.abs(d32.astype(np.float64) - d64)[live].max(axis=1) / unit[live]).max())
        if e > worst["perturb"][0]:
            worst["perturb"] = (e, n)
    return worst


def test_reference_errors_are_the_recorded_ones():
    worst = _measure()
    print("E_REF_REGULARIZE measured %.4g at n = %s (recorded %.4g); E_REF_PERTURB measured %.4g at n = %s (recorded %.4g)"
          % (worst["regularize"] + (E_REF_REGULARIZE,) + worst["perturb"] + (E_REF_PERTURB,)))
    assert E_REF_REGULARIZE / 1.5 <= worst["regularize"][0] <= E_REF_REGULARIZE * 1.5
    assert E_REF_PERTURB / 1.5 <= worst["perturb"][0] <= E_REF_PERTURB * 1.5


def test_mirrors_leave_what_the_contract_leaves():
    """A lambda of 0 returns its array's bits; a zero quaternion and a NaN noise row keep the point's bits; an opaque row
    barely moves and a nearly dead one moves by about rate * Sigma eps."""
    c = mr.step_inputs(257)
    R = mr.STEP_RULES
    go, gs = mr.regularize_f32(c["opacity"], c["scales"], c["grad_opacity"], c["grad_scales"], 0.0, R["lambda_scale"])
    assert np.array_equal(go.view(np.int32), c["grad_opacity"].view(np.int32)) and not np.array_equal(gs, c["grad_scales"])
    assert gs[0, 0] == c["grad_scales"][0, 0] and gs[0, 1] < c["grad_scales"][0, 1]       # sign(0) = 0, sign(-0.02) = -1
    go, gs = mr.regularize_f32(c["opacity"], c["scales"], c["grad_opacity"], c["grad_scales"], R["lambda_opacity"], 0.0)
    assert np.array_equal(gs.view(np.int32), c["grad_scales"].view(np.int32)) and (go > c["grad_opacity"]).all()
    out, d, kept = mr.perturb_f32(c["points"], c["scales"], c["quats"], c["opacity"], c["noise"], R["rate"], R["gate_k"], R["gate_x0"])
    assert list(np.nonzero(kept)[0]) == [1, 2]
    assert np.array_equal(out[1:3].view(np.int32), c["points"][1:3].view(np.int32))
    unit = mr.perturb_norm(c["scales"], c["noise"], R["rate"])
    # the gate is at most 1 / (1 + exp(-gate_k (1 - gate_x0))) = 0.6225 with the published values
    assert np.abs(d[3]).max() < 1e-30 * unit[3] and 0.0 < np.abs(d[4]).max() <= unit[4] * 0.63
