"""gsx_photometric_loss_weighted of include/gsx.h restated in float64 numpy: the weighted value, and the closed-form
gradients dL/dx and dL/dE exactly as the header writes them, built on photometric_loss_restatement (blur, _parts).  Helper
module of tests/test_photometric_loss_weighted_host.py (which pins the closed form to torch's float64 autograd and to central
differences, and measures the float32 reference error E_REF_W) and of tests/test_hip_photometric_loss_weighted.py (which
holds the kernels to 12 E_REF_W of it).  No tests in here.

x' is formed in numpy FLOAT32 in the header's order -- each product and each sum rounded on its own -- and only then taken
to float64: x' - y, and with it the L1 sign, is then the kernel's on every element, and no element is ever left out of a
comparison.  The gradients treat x' as exactly affine in x and E.
"""
import numpy as np

import photometric_loss_restatement as plr

LAMBDAS = plr.LAMBDAS
T = plr.TILE


def apply_exposure(x, E):
    """x' (float32) of an (a, b, 3) float32 image: ((E_i0 x_0 + E_i1 x_1) + E_i2 x_2) + E_i3, every step rounded to float32."""
    x, E = np.asarray(x, np.float32), np.asarray(E, np.float32)
    out = np.empty_like(x)
    for i in range(3):
        out[..., i] = ((E[i, 0] * x[..., 0] + E[i, 1] * x[..., 1]) + E[i, 2] * x[..., 2]) + E[i, 3]
    return out


def _prepare(x, y, m, E):
    x32 = np.asarray(x, np.float32)
    xp = (x32 if E is None else apply_exposure(x32, E)).astype(np.float64)
    y = np.asarray(y, np.float64)
    m = np.ones(x32.shape[:2]) if m is None else np.asarray(m, np.float64)
    return x32.astype(np.float64), xp, y, m


def forward(x, y, lam, m=None, E=None):
    """(loss, l1, ssim, W) of two (a, b, 3) images, an (a, b) weight (None: ones) and a (3, 4) exposure (None: x' = x)."""
    _, xp, y, m = _prepare(x, y, m, E)
    lam = plr.lam64(lam)
    W = float(m.sum())
    if W == 0.0:
        return 0.0, 0.0, 0.0, 0.0
    _, _, A1, A2, B1, B2 = plr._parts(xp, y)
    ssim = float((m[..., None] * (A1 * A2 / (B1 * B2))).sum() / (3 * W))
    l1 = float((m[..., None] * np.abs(xp - y)).sum() / (3 * W))
    return (1 - lam) * l1 + lam * (1 - ssim), l1, ssim, W


def gradient(x, y, lam, m=None, E=None):
    """(dloss/dx (a, b, 3), dloss/dE (3, 4) or None) in float64: the closed form of include/gsx.h, term by term."""
    x, xp, y, m = _prepare(x, y, m, E)
    lam = plr.lam64(lam)
    W = float(m.sum())
    if W == 0.0:
        return np.zeros_like(x), (None if E is None else np.zeros((3, 4)))
    n = 3 * W
    mm = m[..., None]
    mu1, mu2, A1, A2, B1, B2 = plr._parts(xp, y)
    w = -lam / n
    d_mu = 2 * mu2 * (A2 - A1) / (B1 * B2) - 2 * mu1 * A1 * A2 * (B2 - B1) / (B1 * B2) ** 2
    d_p = -A1 * A2 / (B1 * B2 ** 2)
    d_q = 2 * A1 / (B1 * B2)
    gp = ((1 - lam) * mm * np.sign(xp - y) / n + plr.blur(w * mm * d_mu) + 2 * xp * plr.blur(w * mm * d_p)
          + y * plr.blur(w * mm * d_q))
    if E is None:
        return gp, None
    E64 = np.asarray(E, np.float32).astype(np.float64)
    dx = gp @ E64[:, :3]                                  # dx_j = sum_i E_ij g'_i
    dE = np.empty((3, 4))
    dE[:, :3] = np.einsum("abi,abj->ij", gp, x)
    dE[:, 3] = gp.sum(axis=(0, 1))
    return dx, dE


def torch_loss(x, y, lam, m=None, E=None, delta=None):
    """plr.torch_loss extended: the forward formula in torch, in the dtype of x ((a, b, 3)), with an (a, b) weight and a
    (3, 4) exposure applied elementwise in the header's order (in float32 that is x' bit for bit).  ``delta``: a constant
    added to x' -- the float64 autograd check passes (float32 x' - float64 affine x') there, so that its forward sees the
    restatement's x' while its gradient is that of the affine map.  Returns (loss, l1, ssim)."""
    import torch
    import torch.nn.functional as F

    if E is not None:
        x = torch.stack([((E[i, 0] * x[..., 0] + E[i, 1] * x[..., 1]) + E[i, 2] * x[..., 2]) + E[i, 3] for i in range(3)], dim=-1)
    if delta is not None:
        x = x + delta
    g = torch.from_numpy(plr.window()).to(dtype=x.dtype, device=x.device)
    k = (g[:, None] * g[None, :]).expand(3, 1, 11, 11).contiguous()
    conv = lambda z: F.conv2d(z.permute(2, 0, 1)[None], k, padding=5, groups=3)  # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    smap = ((2 * mu1 * mu2 + plr.C1) * (2 * s12 + plr.C2)) / ((mu1 * mu1 + mu2 * mu2 + plr.C1) * (s1 + s2 + plr.C2))
    if m is None:
        ssim, l1 = smap.mean(), (x - y).abs().mean()
    else:
        n = 3 * m.sum()
        ssim, l1 = (m[None, None] * smap).sum() / n, (m[..., None] * (x - y).abs()).sum() / n
    lam = plr.lam64(lam)
    return (1 - lam) * l1 + lam * (1 - ssim), l1, ssim


# ---- the cases: (name, the shape case of photometric_loss_restatement it reuses, mask kind, exposure kind)
# masks     none: a NULL weight;  ones;  binary: 1 except the rows and the columns [32, 35), zero there -- one edge on a tile
#           seam, the other inside the next tile's halo;  single: one pixel with weight 1;  random: uniform in [0, 1];  zero
# exposures none: a NULL exposure;  identity;  general: diagonal 0.6 .. 1.4, off-diagonal and offset within +-0.1;
#           offset: [I | 0.2] -- on a cropped case: wrong if the padding outside the region becomes E_i3
CASES = [
    ("one_pixel_ones_general", "one_pixel", "ones", "general"),
    ("one_pixel_random_none", "one_pixel", "random", "none"),
    ("window_larger_than_image_random_general", "window_larger_than_image", "random", "general"),
    ("tile_minus_1_by_tile_plus_1_binary_identity", "tile_minus_1_by_tile_plus_1", "binary", "identity"),
    ("halo_across_a_neighbour_binary_general", "halo_across_a_neighbour", "binary", "general"),
    ("halo_across_a_neighbour_single_none", "halo_across_a_neighbour", "single", "none"),
    ("halo_across_a_neighbour_random_general", "halo_across_a_neighbour", "random", "general"),
    ("halo_across_a_neighbour_zero_general", "halo_across_a_neighbour", "zero", "general"),
    ("cropped_45x50_of_48x64_random_offset", "cropped_45x50_of_48x64", "random", "offset"),
    ("cropped_45x50_of_48x64_binary_general", "cropped_45x50_of_48x64", "binary", "general"),
    ("cropped_45x50_of_48x64_ones_none", "cropped_45x50_of_48x64", "ones", "none"),
    ("cropped_45x50_of_48x64_zero_none", "cropped_45x50_of_48x64", "zero", "none"),
    ("unaligned_base_random_general", "unaligned_base", "random", "general"),
    ("unaligned_base_none_general", "unaligned_base", "none", "general"),
]
CASE_IDS = [c[0] for c in CASES]
NONZERO_CASE_IDS = [c[0] for c in CASES if c[2] != "zero"]
ZERO_CASE_IDS = [c[0] for c in CASES if c[2] == "zero"]

# ---- plr.LARGE_CASES (tiles with eight neighbours; 256 and 289 tile partials, where wloss_reduce_kernel and
# wloss_exposure_reduce_kernel -- sum_records<3> and <12>, records rec[i * K + k] -- take their loop's second step) x the
# weights that differ per pixel x the exposure that makes dL/dE an output; and the 289 tiles once with both options NULL
# and once with W = 0.  Same format as CASES; they do not feed E_REF_W.
LARGE_CASES = [("%s_%s_general" % (base, mask), base, mask, "general") for base in plr.LARGE_CASE_IDS
               for mask in ("random", "binary")]
LARGE_CASES += [("tiles_289_scalar_none_none", "tiles_289_scalar", "none", "none"),
                ("tiles_289_scalar_zero_general", "tiles_289_scalar", "zero", "general")]
LARGE_CASE_IDS = [c[0] for c in LARGE_CASES]
LARGE_NONZERO_CASE_IDS = [c[0] for c in LARGE_CASES if c[2] != "zero"]
LARGE_ZERO_CASE_IDS = [c[0] for c in LARGE_CASES if c[2] == "zero"]
_ALL_CASES = CASES + LARGE_CASES
_ALL_IDS = CASE_IDS + LARGE_CASE_IDS


def case_geometry(name):
    """(tensor shape (A, B), region (a, b), floats the base pointers are moved by) of the named case."""
    base = _ALL_CASES[_ALL_IDS.index(name)][1]
    _, shape, region, skip = plr.case_of(base)
    return shape, region, skip


def case_inputs(name):
    """(frame, target float32 (A, B, 3); weight float32 (A, B) or None; exposure float32 (3, 4) or None) of the named case.
    Outside the region the weight holds values a correct call never reads (random, or ones for the all-zero mask)."""
    idx = _ALL_IDS.index(name)
    _, base, mask, expo = _ALL_CASES[idx]
    shape, (a, b), _ = case_geometry(name)
    x, y = plr.case_inputs(base)
    rs = np.random.RandomState(500 + idx)
    if mask == "none":
        m = None
    else:
        m = rs.uniform(size=shape).astype(np.float32)
        if mask == "zero":
            m[:] = 1.0
            m[:a, :b] = 0.0
        elif mask == "ones":
            m[:a, :b] = 1.0
        elif mask == "binary":
            m[:a, :b] = 1.0
            m[32:35, :b] = 0.0
            m[:a, 32:35] = 0.0
        elif mask == "single":
            m[:a, :b] = 0.0
            m[min(a - 1, 33), min(b - 1, 31)] = 1.0
    if expo == "none":
        E = None
    else:
        E = np.eye(3, 4, dtype=np.float32)
        if expo == "general":
            E = rs.uniform(-0.1, 0.1, size=(3, 4)).astype(np.float32)
            E[np.arange(3), np.arange(3)] = rs.uniform(0.6, 1.4, size=3).astype(np.float32)
        elif expo == "offset":
            E[:, 3] = 0.2
    return x, y, m, E


def cropped_inputs(name):
    """The inputs of the named case cropped to its region, contiguous: what the restatement takes."""
    x, y, m, E = case_inputs(name)
    _, (a, b), _ = case_geometry(name)
    crop = lambda t: None if t is None else np.ascontiguousarray(t[:a, :b])  # noqa: E731
    return crop(x), crop(y), crop(m), E


def rel_max(got, ref):
    """max|got - ref| in units of the largest entry of ref."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def errors(loss, grad, grad_e, ref_loss, ref_grad, ref_grad_e):
    """The units of E_REF_W: |dloss| / loss for the value, max|d| / max|ref| for dL/dx and for dL/dE (None without E)."""
    out = {"value": abs(float(loss) - ref_loss) / abs(ref_loss), "grad": rel_max(grad, ref_grad)}
    if ref_grad_e is not None:
        out["grad_exposure"] = rel_max(grad_e, ref_grad_e)
    return out
