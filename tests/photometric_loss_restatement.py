"""The photometric loss of include/gsx.h (gsx_photometric_loss) restated in float64 numpy: the value, and the closed-form
gradient exactly as the header writes it.  Helper module of tests/test_photometric_loss_host.py (which pins the closed form
to torch's float64 autograd and to central differences, and measures the float32 reference error E_REF) and of
tests/test_hip_photometric_loss.py (which holds the kernels to 12 E_REF of it).  No tests in here.

The float32 inputs are converted exactly to float64, so x - y -- and with it the L1 sign -- is the same on both sides: no
element is ever left out of a comparison.
"""
import functools

import numpy as np

TILE = 32                   # csrc/gsx_plan.h kLossTile: the edge of a workgroup's tile
LAMBDAS = (0.0, 0.2, 1.0)
C1, C2 = 0.01 ** 2, 0.03 ** 2


def lam64(lam):
    """lambda as the library receives it: a float32, taken to float64 exactly."""
    return float(np.float32(lam))


def window():
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    return g / g.sum()


@functools.lru_cache(maxsize=None)
def _band(n):
    """(n, n): row i holds the window centred on i, cut at the border -- the zero-padded 11-tap filter as a matrix."""
    g = window()
    k = np.zeros((n, n))
    for i in range(n):
        for t in range(11):
            j = i + t - 5
            if 0 <= j < n:
                k[i, j] = g[t]
    return k


def blur(z):
    """G* of the issue: the separable 11 x 11 filter per channel of z (a, b, 3), zero padding 5.  Symmetric: its own adjoint."""
    rows = np.tensordot(_band(z.shape[0]), z, axes=(1, 0))                      # (i, b, c)
    return np.tensordot(rows, _band(z.shape[1]), axes=(1, 1)).transpose(0, 2, 1)  # (i, c, j) -> (i, j, c)


def _parts(x, y):
    mu1, mu2, p, q, r = blur(x), blur(y), blur(x * x), blur(x * y), blur(y * y)
    s1, s2, s12 = p - mu1 * mu1, r - mu2 * mu2, q - mu1 * mu2
    A1, A2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2
    B1, B2 = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    return mu1, mu2, A1, A2, B1, B2


def forward(x, y, lam):
    """(loss, l1, ssim) of two (a, b, 3) images, in float64."""
    x, y, lam = np.asarray(x, np.float64), np.asarray(y, np.float64), lam64(lam)
    _, _, A1, A2, B1, B2 = _parts(x, y)
    ssim = float((A1 * A2 / (B1 * B2)).mean())
    l1 = float(np.abs(x - y).mean())
    return (1 - lam) * l1 + lam * (1 - ssim), l1, ssim


def gradient(x, y, lam):
    """dloss/dx (a, b, 3) in float64: the closed form of include/gsx.h, term by term."""
    x, y, lam = np.asarray(x, np.float64), np.asarray(y, np.float64), lam64(lam)
    n = x.size
    mu1, mu2, A1, A2, B1, B2 = _parts(x, y)
    w = -lam / n
    d_mu = 2 * mu2 * (A2 - A1) / (B1 * B2) - 2 * mu1 * A1 * A2 * (B2 - B1) / (B1 * B2) ** 2
    d_p = -A1 * A2 / (B1 * B2 ** 2)
    d_q = 2 * A1 / (B1 * B2)
    return (1 - lam) * np.sign(x - y) / n + blur(w * d_mu) + 2 * x * blur(w * d_p) + y * blur(w * d_q)


def torch_loss(x, y, lam):
    """The forward formula in torch, in the dtype of x (an (a, b, 3) tensor): F.conv2d(padding=5, groups=3) with the 11 x 11
    window.  Its float64 autograd pins the closed form; its float32 evaluation is the reference whose error is E_REF, and,
    on the GPU, the composition a user would otherwise write.  Returns (loss, l1, ssim)."""
    import torch
    import torch.nn.functional as F

    g = torch.from_numpy(window()).to(dtype=x.dtype, device=x.device)
    k = (g[:, None] * g[None, :]).expand(3, 1, 11, 11).contiguous()
    conv = lambda z: F.conv2d(z.permute(2, 0, 1)[None], k, padding=5, groups=3)  # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    ssim, l1 = m.mean(), (x - y).abs().mean()
    lam = lam64(lam)
    return (1 - lam) * l1 + lam * (1 - ssim), l1, ssim


# ---- the cases of the kernel test: (name, tensor shape (A, B), region (a, b), floats the base pointer is moved by)
T = TILE
CASES = [
    ("one_pixel", (1, 1), (1, 1), 0),
    ("window_larger_than_image", (5, 7), (5, 7), 0),
    ("window_equals_image", (11, 11), (11, 11), 0),
    ("tile_minus_1_by_tile_plus_1", (T - 1, T + 1), (T - 1, T + 1), 0),
    ("tile_by_two_tiles", (T, 2 * T), (T, 2 * T), 0),                       # stride 192: the 16-byte path
    ("two_tiles_plus_5_by_3", (2 * T + 5, 3), (2 * T + 5, 3), 0),
    ("halo_across_a_neighbour", (T + 6, T + 6), (T + 6, T + 6), 0),         # stride 114: the scalar path
    ("cropped_32x48_of_48x64", (48, 64), (32, 48), 0),                      # stride != 3 cols, 16-byte path
    ("cropped_45x50_of_48x64", (48, 64), (45, 50), 0),                      # ... and a row that ends inside a 16-byte access
    ("unaligned_base", (40, 44), (40, 44), 1),                              # stride 132 is a multiple of 4, the base is not
]
CASE_IDS = [c[0] for c in CASES]

# ---- the smallest shapes at which the one-workgroup reduce over the tile partials (loss_reduce_kernel, sum_records:
# `for (i = threadIdx.x; i < tiles; i += 256)`) takes its second step, and at which a tile has neighbours on all eight sides.
# Same format as CASES.  They do not feed E_REF (tests/test_photometric_loss_host.py holds the float32 reference to
# E_REF x E_REF_WINDOW at each of them instead).
LARGE_CASES = [
    ("tiles_3x3_vector", (3 * T, 3 * T), (3 * T, 3 * T), 0),                # stride 288: the 16-byte path; one interior tile
    ("tiles_4x4_scalar", (97, 103), (97, 103), 0),                          # stride 309: the scalar path; partial far tiles
    ("tiles_256", (512, 512), (512, 512), 0),                               # 16 x 16 tiles: one record per reduce thread
    ("tiles_289_scalar", (513, 513), (513, 513), 0),                        # 17 x 17: threads 0..32 take a second; stride 1539
    ("tiles_289_vector_cropped", (520, 516), (513, 514), 0),                # stride 1548: 16-byte path, a row ends inside an access
]
LARGE_CASE_IDS = [c[0] for c in LARGE_CASES]
_ALL_CASES = CASES + LARGE_CASES
_ALL_IDS = CASE_IDS + LARGE_CASE_IDS


def case_of(name):
    """The (name, tensor shape, region, base shift) entry of a case of CASES or LARGE_CASES."""
    return _ALL_CASES[_ALL_IDS.index(name)]


def tiles_of(region):
    return -(-region[0] // TILE) * -(-region[1] // TILE)


def case_inputs(name):
    """(frame, target) float32 (A, B, 3) in [0, 1] of the named case: a smooth-ish random frame and a noisy copy of it."""
    idx = _ALL_IDS.index(name)
    shape = _ALL_CASES[idx][1]
    rs = np.random.RandomState(100 + idx)
    x = rs.uniform(size=shape + (3,)).astype(np.float32)
    y = np.clip(x + rs.normal(0, 0.15, size=x.shape), 0.0, 1.0).astype(np.float32)
    return x, y


def errors(loss, grad, ref_loss, ref_grad):
    """The units of E_REF: |dloss| / loss for the value, max|dgrad| / max|grad| for the gradient."""
    return abs(float(loss) - ref_loss) / abs(ref_loss), float(np.abs(np.asarray(grad, np.float64) - ref_grad).max() / np.abs(ref_grad).max())
