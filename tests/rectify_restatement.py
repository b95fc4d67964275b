"""gsx_rectify_photo (include/gsx.h) restated in numpy: the formula in float64 with every per-sample decision, and a float32
mirror in the kernel's written operation order with the decisions FROZEN to the float64 ones.

The kernel is held to the float64 restatement within 12 x E_REF, E_REF being the mirror's own largest error over CASES
(tests/test_capture_host.py records it and asserts it is still the mirror's).  A float32 coordinate within DELTA of a validity
edge may decide either way: output pixels with such a sample are left out of the comparison (``ambiguous``), their weight
may differ by (ambiguous samples) / S^2, and at most 2 % of a case's pixels may be left out.
"""
import numpy as np

f32 = np.float32
MODELS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4}

# name -> photo size (W, H), COLMAP model and params, target (W', H', fx, fy, cx, cy), samples, seed of the random photo.
# Focal lengths and principal points are not round: no sample sits on a validity edge by construction.
CASES = {
    # every coefficient of the full model, 97 x 61 -> 48 x 32: the target's field is the photo's, so the rim is partly valid
    "opencv_s2": dict(size=(97, 61), model="OPENCV", params=(83.7, 84.9, 47.3, 31.6, -0.11, 0.03, 0.004, -0.006),
                      target=(48, 32, 41.3, 41.9, 23.37, 15.61), samples=2, seed=1),
    "radial_s3": dict(size=(64, 48), model="RADIAL", params=(57.3, 31.2, 24.7, 0.08, -0.01),
                      target=(48, 32, 44.1, 43.7, 23.9, 15.3), samples=3, seed=2),
    # an identity lens at the photo's own size, one sample per pixel
    "pinhole_s1": dict(size=(97, 61), model="PINHOLE", params=(91.3, 90.7, 48.1, 30.9),
                       target=(97, 61, 93.1, 92.3, 47.83, 30.21), samples=1, seed=3),
    # partial blocks on both axes
    "simple_radial_33x7": dict(size=(64, 48), model="SIMPLE_RADIAL", params=(51.9, 32.4, 23.6, -0.07),
                               target=(33, 7, 26.3, 25.1, 16.2, 3.1), samples=2, seed=4),
    "simple_pinhole_s8": dict(size=(64, 48), model="SIMPLE_PINHOLE", params=(49.3, 31.7, 24.4),
                              target=(5, 3, 4.3, 4.7, 2.1, 1.05), samples=8, seed=5),
    # an off-centre principal point under a target wider than the photo: a border of pixels with no valid sample on all sides
    "offcentre_border": dict(size=(97, 61), model="OPENCV", params=(83.7, 84.9, 60.2, 25.3, -0.05, 0.01, -0.002, 0.003),
                             target=(48, 32, 30.2, 29.6, 23.37, 15.61), samples=2, seed=6),
    # a barrel lens strong enough to fold inside the target's field: samples that land in the photo with det <= 0
    "barrel_fold": dict(size=(64, 48), model="SIMPLE_RADIAL", params=(40.3, 31.6, 23.8, -0.6),
                        target=(48, 32, 18.3, 18.9, 23.6, 15.4), samples=2, seed=7),
}


def photo_of(case):
    w, h = case["size"]
    return np.random.default_rng(case["seed"]).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def lens_coefficients(model, params):
    """(fx_s, fy_s, cx_s, cy_s, k1, k2, p1, p2) of COLMAP's params: a coefficient the model lacks is 0."""
    p = [float(v) for v in params]
    if model == "SIMPLE_PINHOLE":
        return p[0], p[0], p[1], p[2], 0.0, 0.0, 0.0, 0.0
    if model == "PINHOLE":
        return p[0], p[1], p[2], p[3], 0.0, 0.0, 0.0, 0.0
    if model == "SIMPLE_RADIAL":
        return p[0], p[0], p[1], p[2], p[3], 0.0, 0.0, 0.0
    if model == "RADIAL":
        return p[0], p[0], p[1], p[2], p[3], p[4], 0.0, 0.0
    if model == "OPENCV":
        return tuple(p)
    raise ValueError(model)


def _inputs(case, dtype):
    """The numbers the kernel sees -- everything goes through float32 first, as the C structs hold it."""
    co = [dtype(f32(v)) for v in lens_coefficients(case["model"], case["params"])]
    tw, th = case["target"][:2]
    tg = [dtype(f32(v)) for v in case["target"][2:]]
    return co, int(tw), int(th), tg


def _coordinates(case, dtype):
    """(x, y, u, v, det), arrays (W', H', S, S) indexed [i, j, b, a], in ``dtype``, in the header's operation order."""
    (fxs, fys, cxs, cys, k1, k2, p1, p2), tw, th, (fx, fy, cx, cy) = _inputs(case, dtype)
    S = int(case["samples"])
    half, one, two, six = dtype(0.5), dtype(1.0), dtype(2.0), dtype(6.0)
    off = (np.arange(S).astype(dtype) + half) / dtype(S) - half
    i = np.arange(tw).astype(dtype)[:, None, None, None]
    j = np.arange(th).astype(dtype)[None, :, None, None]
    x = ((i + off[None, None, None, :]) - cx) / fx
    y = ((j + off[None, None, :, None]) - cy) / fy
    x, y = np.broadcast_arrays(x, y)
    xx, yy, xy = x * x, y * y, x * y
    r2 = xx + yy
    rho = (k1 + k2 * r2) * r2
    xd = ((x + x * rho) + (two * p1) * xy) + p2 * (r2 + two * xx)
    yd = ((y + y * rho) + p1 * (r2 + two * yy)) + (two * p2) * xy
    g = one + rho
    gp = k1 + (two * k2) * r2
    jxx = ((g + (two * xx) * gp) + (two * p1) * y) + (six * p2) * x
    jyy = ((g + (two * yy) * gp) + (six * p1) * y) + (two * p2) * x
    jxy = ((two * xy) * gp + (two * p1) * x) + (two * p2) * y
    det = jxx * jyy - jxy * jxy
    u = fxs * xd + (cxs - half)
    v = fys * yd + (cys - half)
    return x, y, u, v, det


def _bilinear(photo, u, v, dtype):
    """(..., 3): top = p00 + tx (p01 - p00); bot likewise; top + ty (bot - top).  Indices clamped into the photo (a frozen
    decision may gather a sample whose float32 coordinate is a hair outside)."""
    h, w = photo.shape[:2]
    u, v = np.clip(u, dtype(0), dtype(w - 1)), np.clip(v, dtype(0), dtype(h - 1))
    fu, fv = np.floor(u), np.floor(v)
    x0, y0 = fu.astype(np.int64), fv.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    tx, ty = (u - fu)[..., None], (v - fv)[..., None]
    p = photo.astype(dtype)
    top = p[y0, x0] + tx * (p[y0, x1] - p[y0, x0])
    bot = p[y1, x0] + tx * (p[y1, x1] - p[y1, x0])
    return top + ty * (bot - top)


def restate64(case, photo=None):
    """The float64 restatement: dict of image (W', H', 3), weight (W', H'), count, and per sample u, v, det and the
    decisions (valid, and why not: left / right / top / bottom / folded)."""
    photo = photo_of(case) if photo is None else photo
    h, w = photo.shape[:2]
    S = int(case["samples"])
    _, _, u, v, det = _coordinates(case, np.float64)
    left, right, top, bottom = u < 0, u > w - 1, v < 0, v > h - 1
    inside = ~(left | right | top | bottom)
    folded = inside & ~(det > 0)
    valid = inside & (det > 0)
    val = np.where(valid[..., None], _bilinear(photo, np.where(valid, u, 0.0), np.where(valid, v, 0.0), np.float64), 0.0)
    count = valid.sum(axis=(2, 3))
    total = val.sum(axis=(2, 3))
    image = np.where(count[..., None] > 0, total / (255.0 * np.maximum(count, 1)[..., None]), 0.0)
    return dict(image=image, weight=count / float(S * S), count=count, u=u, v=v, det=det, valid=valid, left=left, right=right,
                top=top, bottom=bottom, folded=folded)


def mirror32(case, valid, photo=None):
    """The float32 mirror in the kernel's operation order with the decisions ``valid`` (restate64's): image, weight, u, v, det."""
    photo = photo_of(case) if photo is None else photo
    S = int(case["samples"])
    _, _, u, v, det = _coordinates(case, f32)
    assert u.dtype == f32 and det.dtype == f32
    val = _bilinear(photo, np.where(valid, u, f32(0)), np.where(valid, v, f32(0)), f32)
    assert val.dtype == f32
    tw, th = u.shape[:2]
    total = np.zeros((tw, th, 3), f32)
    count = np.zeros((tw, th), np.int64)
    for b in range(S):              # the kernel's order: b outer, a inner, skipped samples add nothing
        for a in range(S):
            ok = valid[:, :, b, a]
            total = np.where(ok[..., None], total + val[:, :, b, a], total)
            count += ok
    den = f32(255.0) * np.maximum(count, 1).astype(f32)
    image = np.where(count[..., None] > 0, total / den[..., None], f32(0)).astype(f32)
    weight = (count.astype(f32) / f32(S * S)).astype(f32)
    return dict(image=image, weight=weight, u=u, v=v, det=det)


def ambiguous_samples(ref, size, delta):
    """Per output pixel, the samples whose float64 u or v lies within ``delta`` of a validity edge, or whose Jacobian
    determinant lies within ``delta`` of 0 while the sample is inside the photo: float32 may decide them either way."""
    w, h = size
    u, v, det = ref["u"], ref["v"], ref["det"]
    near = (np.abs(u) <= delta) | (np.abs(u - (w - 1)) <= delta) | (np.abs(v) <= delta) | (np.abs(v - (h - 1)) <= delta)
    near |= (np.abs(det) <= delta) & (u >= -delta) & (u <= w - 1 + delta) & (v >= -delta) & (v <= h - 1 + delta)
    return near.sum(axis=(2, 3))


def mirror_errors(case):
    """(E image, E weight, delta) of one case: the mirror against the float64 restatement."""
    photo = photo_of(case)
    ref = restate64(case, photo)
    mir = mirror32(case, ref["valid"], photo)
    e_img = float(np.abs(mir["image"].astype(np.float64) - ref["image"]).max())
    e_w = float(np.abs(mir["weight"].astype(np.float64) - ref["weight"]).max())
    # coordinate error where a decision can depend on it: samples that are inside the photo or within a pixel of it
    w, h = case["size"]
    close = (ref["u"] > -1) & (ref["u"] < w) & (ref["v"] > -1) & (ref["v"] < h)
    delta = max(float(np.abs(mir[k].astype(np.float64) - ref[k])[close].max()) for k in ("u", "v", "det"))
    return e_img, e_w, delta


def compare(case, image, weight, bound_image, bound_weight, delta, ref=None):
    """Asserts a kernel's outputs against the float64 restatement; returns (largest image error, largest weight error,
    pixels left out)."""
    ref = restate64(case) if ref is None else ref
    S = int(case["samples"])
    amb = ambiguous_samples(ref, case["size"], delta)
    keep = amb == 0
    assert (~keep).mean() <= 0.02, "more than 2 %% of the pixels are ambiguous: %d" % int((~keep).sum())
    e_img = np.abs(np.asarray(image, np.float64) - ref["image"])
    e_w = np.abs(np.asarray(weight, np.float64) - ref["weight"])
    worst_i, worst_w = float(e_img[keep].max()), float(e_w[keep].max())
    print("image error %.3g (bound %.3g), weight error %.3g (bound %.3g), %d pixels left out" % (
        worst_i, bound_image, worst_w, bound_weight, int((~keep).sum())))
    assert worst_i <= bound_image, (worst_i, bound_image)
    assert worst_w <= bound_weight, (worst_w, bound_weight)
    assert np.all(e_w[~keep] <= amb[~keep] / float(S * S) + bound_weight)
    return worst_i, worst_w, int((~keep).sum())
