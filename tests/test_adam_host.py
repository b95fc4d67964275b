"""gsx_adam_step, host side: the C ABI's refusals and layout, the Python surface as far as it goes without a GPU, expon_lr,
and the float32 restatement (tests/adam_restatement.py) against torch's Adam on the CPU.

The restatement against torch: 20 steps from zero moments over 1500 elements, fresh gradients per step (random sign,
magnitude exp(U(-3, 3)), a fifth of the entries zeroed on steps 5 and 12), at lr 1e-4 and 2e-2, betas (0.9, 0.999), eps 1e-8;
LINEAR on parameters N(0, 1), LOG on parameters exp(N(-3, 1)) against torch.optim.Adam on a leaf theta = log p with
theta.grad = g exp(theta).  Truth is torch's Adam (foreach=False) in float64.  Error of an element after step t, in units of
    lr + t 2^-24 |p|        (LINEAR: a step is of the order of lr; the parameter is rounded once per step)
    lr |p| + t 2^-24 |p|    (LOG: a step moves log p by the order of lr)
E_REF: the worst such error of torch's own float32 Adam (foreach=False) against the truth, over both rates, all steps and
elements.  Measured on the CPU:
    linear  7.993e-03   (lr 1e-4; 3.456e-05 at lr 2e-2)
    log     1.838e-02   (lr 1e-4; 9.096e-05 at lr 2e-2)
and the float32 restatement's own worst error, held to 2 E_REF: linear 7.993e-03 (1.00 E_REF), log 6.386e-03 (0.35 E_REF).
(The scale is generous to both -- what is left of float32's rounding of p is well below t 2^-24 |p| -- and the ratio is what
counts: the restatement is torch's float32 Adam to the last digit printed on a LINEAR group.)
(LOG: torch rounds theta, of magnitude 3, once per step and exponentiates it; the restatement rounds p itself.)
The GPU tests (tests/test_hip_adam.py) hold the kernel's LOG parameters, and a real step against torch, to 12 E_REF, the
multiple the SH, geometry and loss tests use.  torch's float32 kernels may fuse or order operations differently from one CPU
to another: the test accepts the measured figure within a factor 1.5 of the recorded one; the bounds are built from the
RECORDED figures.
"""
import ctypes
import math
import re
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

import adam_restatement as ar

E_REF = {"linear": 7.993e-03, "log": 1.838e-02}
E_REF_WINDOW = 1.5
BOUND_RESTATEMENT = {k: 2 * v for k, v in E_REF.items()}
BOUND_KERNEL = {k: 12 * v for k, v in E_REF.items()}

STEPS, ELEMENTS, RATES = 20, 1500, (1e-4, 2e-2)
BETAS, EPS = (0.9, 0.999), 1e-8
ULP = 2.0 ** -24


def gradients(seed, steps=STEPS, shape=(ELEMENTS,), zeroed=(5, 12)):
    """Fresh float32 gradients per step: random sign, magnitude exp(U(-3, 3)); on the steps `zeroed` (1-based) a fifth of
    the entries are zero."""
    rs = np.random.RandomState(seed)
    out = []
    for t in range(1, steps + 1):
        g = (rs.choice([-1.0, 1.0], size=shape) * np.exp(rs.uniform(-3, 3, size=shape))).astype(np.float32)
        if t in zeroed:
            g[rs.uniform(size=shape) < 0.2] = 0.0
        out.append(g)
    return out


def start(transform, seed=1, shape=(ELEMENTS,)):
    rs = np.random.RandomState(seed)
    z = rs.normal(size=shape)
    return (np.exp(z - 3.0) if transform == ar.LOG else z).astype(np.float32)


def error_scale(p_true, lr, t, transform):
    p = np.abs(p_true)
    return (lr * p if transform == ar.LOG else lr) + t * ULP * p


def torch_adam(p0, grads, lr, transform, dtype):
    """torch.optim.Adam (foreach=False) in `dtype`; LOG: on a leaf theta = log p0 (rounded to `dtype`), theta.grad = g exp(theta).
    Returns the parameter p after every step, float64."""
    x = torch.from_numpy(p0.astype(np.float64))
    leaf = (torch.log(x) if transform == ar.LOG else x).to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([leaf], lr=lr, betas=BETAS, eps=EPS, foreach=False)
    out = []
    for g in grads:
        gt = torch.from_numpy(g).to(dtype)
        leaf.grad = gt * torch.exp(leaf.detach()) if transform == ar.LOG else gt
        opt.step()
        p = torch.exp(leaf.detach()) if transform == ar.LOG else leaf.detach()
        out.append(p.double().numpy().copy())
    return out


def restatement(p0, grads, lr, transform):
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    out = []
    for t, g in enumerate(grads, 1):
        p, m, v = ar.step32(p, g, m, v, lr, t, BETAS[0], BETAS[1], EPS, transform)
        out.append(p.astype(np.float64))
    return out


def worst(run, truth, lr, transform):
    return max(float((np.abs(a - b) / error_scale(b, lr, t, transform)).max()) for t, (a, b) in enumerate(zip(run, truth), 1))


@pytest.mark.parametrize("name,transform", [("linear", ar.LINEAR), ("log", ar.LOG)])
def test_restatement_is_as_close_to_float64_adam_as_torchs_float32_adam(name, transform):
    e_ref, e_mine = 0.0, 0.0
    for lr in RATES:
        p0, grads = start(transform), gradients(2)
        truth = torch_adam(p0, grads, lr, transform, torch.float64)
        ref = worst(torch_adam(p0, grads, lr, transform, torch.float32), truth, lr, transform)
        mine = worst(restatement(p0, grads, lr, transform), truth, lr, transform)
        print("%s lr %g: torch float32 %.4g, restatement %.4g of the error scale" % (name, lr, ref, mine))
        e_ref, e_mine = max(e_ref, ref), max(e_mine, mine)
    print("E_REF %s = %.4g (recorded %.4g); restatement %.4g = %.2f E_REF" % (name, e_ref, E_REF[name], e_mine, e_mine / E_REF[name]))
    assert E_REF[name] / E_REF_WINDOW <= e_ref <= E_REF[name] * E_REF_WINDOW, (name, e_ref)
    assert e_mine <= BOUND_RESTATEMENT[name], (name, e_mine)


def test_float64_restatement_is_float64_adam():
    """step64 differs from torch's float64 Adam by the hyper-parameters alone (the float32 values the C ABI receives):
    beta2 = float32(0.999) is 1.3e-8 off, which over 20 steps stays below 1e-6 of the error scale's lr."""
    for transform in (ar.LINEAR, ar.LOG):
        p0, grads = start(transform), gradients(2)
        truth = torch_adam(p0, grads, 2e-2, transform, torch.float64)
        p, m, v = p0.astype(np.float64), np.zeros(p0.shape), np.zeros(p0.shape)
        for t, g in enumerate(grads, 1):
            p, m, v = ar.step64(p, g, m, v, 2e-2, t, BETAS[0], BETAS[1], EPS, transform)
            e = float((np.abs(p - truth[t - 1]) / error_scale(truth[t - 1], 2e-2, t, transform)).max())
            assert e <= 1e-6, (transform, t, e)


def test_live_rows_nan_counts_and_negative_zero_does_not():
    a = np.zeros((5, 3), np.float32)
    b = np.zeros((5, 1), np.float32)
    a[1, 2] = -0.0
    a[2, 0] = np.nan
    b[3, 0] = 1e-45
    assert ar.live_rows([a, b]).tolist() == [False, False, True, True, False]
    p = np.arange(15, dtype=np.float32).reshape(5, 3) + 1
    m = np.full((5, 3), np.nan, np.float32)
    p2, m2, v2 = ar.step32(p, a, m, m, 1e-2, 3, rows=ar.live_rows([a, b]))
    for r in (0, 1, 4):
        assert p2[r].tobytes() == p[r].tobytes() and m2[r].tobytes() == m[r].tobytes() and v2[r].tobytes() == m[r].tobytes()


# ---- C ABI
def test_header_declares_ffi_binds_and_layout():
    from intro_to_gaussian_splatting_amd import _ffi

    hdr = open(os.path.join(ROOT, "include", "gsx.h")).read()
    assert re.search(r"GSX_API\s+int\s+gsx_adam_step\(", hdr)
    assert re.search(r"#define\s+GSX_VERSION\s+305\b", hdr) and _ffi.load().gsx_version() == 305
    assert len(_ffi.SIGNATURES["gsx_adam_step"][1]) == 9
    assert ctypes.sizeof(_ffi.GsxAdamGroup) == 48
    assert _ffi.GsxAdamGroup.width.offset == 32 and _ffi.GsxAdamGroup.lr.offset == 40 and _ffi.GsxAdamGroup.reserved.offset == 44
    for name in ("GSX_ADAM_MAX_GROUPS", "GSX_ADAM_LINEAR", "GSX_ADAM_LOG", "GSX_ADAM_SKIP_ZERO_ROWS"):
        m = re.search(r"\b%s\s*=?\s*(\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(_ffi, name), name
    import test_cabi

    assert "gsx_adam_step" in test_cabi._declared_functions()


def _groups(k=2, **kw):
    from intro_to_gaussian_splatting_amd import _ffi

    arr = (_ffi.GsxAdamGroup * max(k, 1))()
    for i in range(k):
        g = arr[i]
        g.param, g.grad, g.exp_avg, g.exp_avg_sq = 4096, 8192, 12288, 16384      # never dereferenced
        g.width, g.transform, g.lr, g.reserved = 3, i % 2, 1e-3, 0.0
    for key, val in kw.items():
        setattr(arr[k - 1], key, val)
    return arr


def test_refusals_name_the_argument_and_need_no_gpu():
    from intro_to_gaussian_splatting_amd import _ffi

    lib = _ffi.load()
    ok = dict(groups=_groups(), n_groups=2, n=100, step=1, beta1=0.9, beta2=0.999, eps=1e-8, flags=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gsx_adam_step(a["groups"], a["n_groups"], a["n"], a["step"], a["beta1"], a["beta2"], a["eps"], a["flags"], None)

    nan, inf = float("nan"), float("inf")
    bad = [(dict(groups=None), b"groups"), (dict(n_groups=0), b"n_groups"), (dict(n_groups=9), b"n_groups"),
           (dict(n_groups=-1), b"n_groups"), (dict(n=-1), b"n = -1"), (dict(step=0), b"step"), (dict(step=-5), b"step"),
           (dict(groups=_groups(param=None)), b"groups[1].param"), (dict(groups=_groups(grad=None)), b"groups[1].grad"),
           (dict(groups=_groups(exp_avg=None)), b"groups[1].exp_avg "), (dict(groups=_groups(exp_avg_sq=None)), b"groups[1].exp_avg_sq"),
           (dict(groups=_groups(width=0)), b"groups[1].width"), (dict(groups=_groups(width=-3)), b"groups[1].width"),
           (dict(groups=_groups(transform=2)), b"groups[1].transform"), (dict(groups=_groups(transform=-1)), b"groups[1].transform"),
           (dict(groups=_groups(reserved=1.0)), b"groups[1].reserved"), (dict(groups=_groups(reserved=nan)), b"groups[1].reserved"),
           (dict(groups=_groups(lr=-1e-3)), b"groups[1].lr"), (dict(groups=_groups(lr=nan)), b"groups[1].lr"),
           (dict(groups=_groups(lr=inf)), b"groups[1].lr"),
           (dict(beta1=-0.1), b"beta1"), (dict(beta1=1.0), b"beta1"), (dict(beta1=nan), b"beta1"), (dict(beta1=inf), b"beta1"),
           (dict(beta2=-0.1), b"beta2"), (dict(beta2=1.0), b"beta2"), (dict(beta2=nan), b"beta2"),
           (dict(eps=-1e-8), b"eps"), (dict(eps=nan), b"eps"), (dict(eps=inf), b"eps"),
           (dict(flags=2), b"flags"), (dict(flags=0x80000001), b"flags")]
    for kw, word in bad:
        assert call(**kw) == _ffi.GSX_ERR_INVALID_ARGUMENT, kw
        assert word in lib.gsx_last_error(), (kw, lib.gsx_last_error())
    # n == 0: nothing to do, and no pointer is looked at -- but the descriptors are still checked
    null = _groups(param=None, grad=None, exp_avg=None, exp_avg_sq=None)
    assert call(n=0) == _ffi.GSX_OK and call(n=0, groups=null) == _ffi.GSX_OK and call(n=0, flags=1) == _ffi.GSX_OK
    assert call(n=0, groups=_groups(width=0)) == _ffi.GSX_ERR_INVALID_ARGUMENT
    assert call(n=0, step=0) == _ffi.GSX_ERR_INVALID_ARGUMENT
    with pytest.raises(_ffi.GsxError):
        _ffi.check(call(step=0))


# ---- Python surface, as far as it goes without a GPU
def _cpu_container(n=4):
    from intro_to_gaussian_splatting_amd import Gaussians

    return Gaussians(torch.zeros((n, 3)), torch.zeros((n, 3)), device="cpu")


def test_python_surface_refuses_cpu_tensors_empty_group_sets_and_unknown_names():
    from intro_to_gaussian_splatting_amd import GaussianAdam

    g = _cpu_container()
    with pytest.raises(ValueError, match="nothing to optimise"):
        GaussianAdam(g, lr={"points": 1e-3})                    # nothing requires grad
    g.points.requires_grad_(True)
    with pytest.raises(ValueError, match="nothing to optimise"):
        GaussianAdam(g, lr={"scales": 1e-3})                    # named, but not trained
    with pytest.raises(ValueError, match="nothing to optimise"):
        GaussianAdam(g, lr={"sh": 1e-3})                        # named, but absent
    with pytest.raises(ValueError, match="points is on cpu.*no CPU fallback"):
        GaussianAdam(g, lr={"points": 1e-3})
    with pytest.raises(ValueError, match="log_groups names 'scale'"):
        GaussianAdam(g, lr={"points": 1e-3}, log_groups=("scale",))
    with pytest.raises(ValueError, match="lr names 'means'"):
        GaussianAdam(g, lr={"means": 1e-3})
    with pytest.raises(ValueError, match="betas"):
        GaussianAdam(g, lr={"points": 1e-3}, betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="eps"):
        GaussianAdam(g, lr={"points": 1e-3}, eps=-1.0)


def test_expon_lr_at_its_ends_between_and_beyond():
    from intro_to_gaussian_splatting_amd import expon_lr

    f = expon_lr(1.6e-4, 1.6e-6, 30000)
    assert f(0) == 1.6e-4 and f(30000) == 1.6e-6 and f(10 ** 6) == 1.6e-6 and f(-3) == 1.6e-4
    assert abs(f(15000) / 1.6e-5 - 1) <= 1e-12                  # the geometric mean half way
    assert all(f(t) > f(t + 1) for t in range(0, 30000, 997))
    for t in (1, 100, 29999):
        assert abs(math.log(f(t)) - ((1 - t / 30000) * math.log(1.6e-4) + t / 30000 * math.log(1.6e-6))) <= 1e-12
    with pytest.raises(ValueError):
        expon_lr(0.0, 1e-3, 10)
    with pytest.raises(ValueError):
        expon_lr(1e-3, 1e-4, 0)
