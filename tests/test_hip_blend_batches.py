"""The tile-16 compositing instance a frame runs (gsx_blend.hip: blend_tile16<REF>) stages TWO 64-record sub-batches per
synchronisation where both are regular; the plain instance (GSX_FLAG_PLAIN_FOOTPRINTS) keeps batches of 64 and shares
every arithmetic path with it on scenes without flagged records -- an in-tree bit reference for the 64-record
semantics.  One 16x16 tile (tile (1, 1) of a 48x48 frame, or a 16x16 frame) with a hand-made list: list lengths around
every boundary of 64 and 128, the skip budget running out on either side of a seam, saturation in either half, a
flagged / D1 < 0 / monomial record in either half, and the cost word a tile leaves for the next frame's schedule.
Needs an MI355X: ``pytest -m gpu``.

Bars: REF against plain, and wh3 against hw3: bit-equal.  Against the C restatement: 1e-4 per pixel, the bar of
tests/test_hip_parity.py (PIXEL_TOL), which is also what its stage-2 tests of ill-conditioned conics use."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PIXEL_TOL = 1e-4
TILE = 16
X0 = Y0 = 16              # origin of the tile under test in the 48x48 frame
FRAME = 48
BUDGET = 1 << 23          # gsx_blend.hip: kSkipBudget, in units of 2^-40
BATCH_COST = 5            # gsx_blend.hip: kBatchCost
LENGTHS = [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU (run with -m gpu on an MI355X box)")


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def _pre(means, inv, op_arg, colors):
    """Stage-1 arrays of a list for tile (1, 1) of the 48x48 frame alone: the caller-given boxes (17 .. 30) touch no other
    tile under the reference's listing rule (x0 >= min - T and x0 <= max).  Rows are in compositing order."""
    from oracle import cpu_ref

    n = means.shape[0]
    f = np.float32
    box = lambda v: np.full(n, v, f)  # noqa: E731
    return cpu_ref.Preprocessed(
        points=means.astype(f), colors=colors.astype(f), covariance_2d=np.zeros((n, 2, 2), f),
        depths=np.arange(n, dtype=f) + 1.0, inverse_covariance_2d=inv.astype(f), radius=np.full(n, 7.0, f),
        points_xy=means.astype(f), min_x=box(X0 + 1), min_y=box(Y0 + 1), max_x=box(X0 + 14), max_y=box(Y0 + 14),
        sigmoid_opacity=np.asarray(op_arg, f).reshape(n, 1), order=np.arange(n))


def _round(rs, n, sigma=(0.8, 1.6), op_arg=(-2.0, 2.0)):
    """n round, unflagged footprints with their means spread over the tile: at these sizes a block drops the records of
    the far side of the tile (alpha < 2^-26 from ~7 sigma), so the four 8x8 blocks keep different subsets."""
    means = np.stack([rs.uniform(X0 - 1.0, X0 + 16.0, n), rs.uniform(Y0 - 1.0, Y0 + 16.0, n)], axis=1)
    s = rs.uniform(sigma[0], sigma[1], n)
    inv = np.zeros((n, 2, 2))
    inv[:, 0, 0] = inv[:, 1, 1] = 1.0 / (s * s)
    return means, inv, rs.uniform(op_arg[0], op_arg[1], n), rs.uniform(0.05, 1.0, (n, 3))


def _render(pre, flags=0, layout="wh3", frame=FRAME):
    from intro_to_gaussian_splatting_amd import render_preprocessed

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    st = {}
    img = render_preprocessed(frame, frame, TILE, t(pre.points), t(pre.colors), t(pre.inverse_covariance_2d), t(pre.min_x),
                              t(pre.max_x), t(pre.min_y), t(pre.max_y), t(pre.sigmoid_opacity), layout=layout, stats=st, flags=flags)
    torch.cuda.synchronize()
    return img, st


def _both_instances(pre, tag):
    """REF and plain frames of `pre` bit-equal, nothing left undone; returns the REF frame as numpy (W, H, 3)."""
    from intro_to_gaussian_splatting_amd import _ffi

    ref_img, st = _render(pre)
    plain_img, st_plain = _render(pre, flags=_ffi.GSX_FLAG_PLAIN_FOOTPRINTS)
    assert st["n_redo"] == 0 and st_plain["n_redo"] == 0, (tag, st, st_plain)
    assert st["n_instances"] == st_plain["n_instances"] == pre.points.shape[0], (tag, st)
    assert torch.equal(ref_img, plain_img), (tag, float((ref_img - plain_img).abs().max()))
    return ref_img.cpu().numpy()


def _nothing_saturates(means, inv, op_arg):
    """The instance a frame runs pairs sub-batches only until the tile's first pixel saturates: a case that is about a pair
    must not saturate anywhere in the list (host restatement; a factor of ten clear of the 1e-6 stop)."""
    t = _transmittance(means, inv, op_arg)
    print("smallest T in front of any record / behind the last: %.3g" % float(t.min()))
    return bool(t.min() > 1e-5)


def _against_c(pre, img, tag, frame=FRAME):
    from oracle import c_oracle

    ref, _, inst = c_oracle.render(pre, frame, frame, TILE)
    d = float(np.abs(img - ref).max())
    print("%s: max |dpixel| against the C restatement %.3g, image max %.3g" % (tag, d, float(ref.max())))
    assert inst == pre.points.shape[0]
    assert float(ref.max()) > 1e-3, tag          # (something is in the picture)
    assert d <= PIXEL_TOL, (tag, d)
    return ref


# ---- host restatement of what stage_records decides (float64; the tests keep every bound away from the class limits)

def _block_bounds(means, inv, op_arg, x0=X0, y0=Y0):
    """(n, 4): log2 of the largest alpha of every record over each 8x8 block of the tile at (x0, y0) -- stage_records' `over`."""
    c = 0.5 * np.log2(np.e)
    m00, m01, m11 = c * inv[:, 0, 0], c * 0.5 * (inv[:, 0, 1] + inv[:, 1, 0]), c * inv[:, 1, 1]
    r11 = np.sqrt(m11)
    h = m01 / r11
    d1 = m00 - h * h
    lop = np.log2(_sigmoid(op_arg))               # (the reference applies the sigmoid to PreprocessedScene.sigmoid_opacity again)
    x, y = means[:, 0] - x0, means[:, 1] - y0
    out = np.zeros((means.shape[0], 4))
    for g in range(4):
        xl, yl = 8.0 * (g & 1), 8.0 * (g >> 1)
        ex0, ex1, ey0, ey1 = x - xl, x - (xl + 7.0), y - yl, y - (yl + 7.0)
        ex_min2 = np.where(ex0 * ex1 <= 0.0, 0.0, np.minimum(ex0 * ex0, ex1 * ex1))
        w = np.stack([r11 * ey0 + h * ex0, r11 * ey1 + h * ex0, r11 * ey0 + h * ex1, r11 * ey1 + h * ex1])
        wlo, whi = w.min(axis=0), w.max(axis=0)
        w_min2 = np.where((wlo <= 0.0) & (whi >= 0.0), 0.0, np.minimum(np.abs(wlo), np.abs(whi)) ** 2)
        out[:, g] = lop - d1 * ex_min2 - w_min2
    return out


def _clear_of_limits(bounds, margin=0.005):
    """No bound so close to a class limit that float32 (the record's D1, h, r11 are rounded once from float64) could decide otherwise."""
    return bool(np.all(np.abs(bounds[..., None] - np.array([-26.0, -33.0, -40.0])) > margin))


def _stage(bounds):
    """stage_records + skip_threshold over a list walked 64 entries at a time: per sub-batch the entries every block
    keeps (4,) and the threshold every block applied (4,)."""
    skipped = [0, 0, 0, 0]
    counts, thrs = [], []
    for k in range(0, bounds.shape[0], 64):
        cnt, thr = [], []
        for g in range(4):
            b = bounds[k:k + 64, g]
            n3 = int((b < -40.0).sum())
            n2 = int((b < -33.0).sum()) - n3
            n1 = int((b < -26.0).sum()) - n2 - n3
            c3, c23 = n3, n3 + (n2 << 7)
            c123 = c23 + (n1 << 14)
            if skipped[g] + c123 <= BUDGET:
                skipped[g] += c123
                t = -26.0
            elif skipped[g] + c23 <= BUDGET:
                skipped[g] += c23
                t = -33.0
            elif skipped[g] + c3 <= BUDGET:
                skipped[g] += c3
                t = -40.0
            else:
                t = -np.inf
            thr.append(t)
            cnt.append(int((~(b < t)).sum()))
        counts.append(cnt)
        thrs.append(thr)
    return np.array(counts), np.array(thrs)


def _transmittance(means, inv, op_arg, x0=X0, y0=Y0):
    """(n + 1, 16, 16) float64: T of every pixel [x, y] of the tile in front of record k under the reference's rule (a
    pixel whose T (1 - alpha) would drop below 1e-6 stops: T = 0 from there)."""
    xs, ys = np.meshgrid(np.arange(16.0) + x0, np.arange(16.0) + y0, indexing="ij")
    T = np.ones((means.shape[0] + 1, 16, 16))
    op = _sigmoid(op_arg)
    for k in range(means.shape[0]):
        dx, dy = means[k, 0] - xs, means[k, 1] - ys
        q = inv[k]
        alpha = op[k] * np.exp(-0.5 * (dx * dx * q[0, 0] + dx * dy * (q[0, 1] + q[1, 0]) + dy * dy * q[1, 1]))
        t = T[k] * (1.0 - alpha)
        T[k + 1] = np.where((T[k] == 0.0) | (t < 1e-6), 0.0, t)
    return T


# ---- list lengths around every boundary

@pytest.mark.parametrize("length", LENGTHS)
def test_list_lengths_around_the_batch_boundaries(length):
    """L round footprints on one tile, L around every multiple of 64 and 128: a last sub-batch of one record, a pair whose
    second half is empty, full or one short.  The four blocks keep different subsets (checked on the host)."""
    _need_gpu()
    rs = np.random.RandomState(1000 + length)
    means, inv, op_arg, colors = _round(rs, length)
    pre = _pre(means, inv, op_arg, colors)
    counts, _ = _stage(_block_bounds(means, inv, op_arg))
    if length >= 63:
        assert len({int(c) for c in counts.sum(axis=0)}) > 1, counts.sum(axis=0)      # the blocks' lists differ
        assert counts.sum() < 4 * length                                               # some block drops some record
    T = _transmittance(means, inv, op_arg)
    assert T[-1].min() > 1e-5                      # (no pixel saturates: these cases are about the list alone)
    img = _both_instances(pre, "L=%d" % length)
    hw, st = _render(pre, layout="hw3")
    assert st["n_redo"] == 0
    assert np.array_equal(hw.cpu().numpy().transpose(1, 0, 2), img)
    _against_c(pre, img, "L=%d" % length)


# ---- the skip budget across the seam

def _far_records(rs, n, e_lo=26.5, e_hi=32.5):
    """Thin upright footprints to the right of the tile whose largest alpha on the tile's RIGHT blocks is 2^-e, e in
    [e_lo, e_hi): skip class 1 there (charged 2^14 units each); on the left blocks, 8 px farther, they are 2^-60 and less."""
    sx, sy = 2.0, 20.0
    op_arg = np.full(n, 10.0)
    e = rs.uniform(e_lo, e_hi, n)
    dx = sx * np.sqrt(2.0 * (e * np.log(2.0) + np.log(_sigmoid(10.0))))
    means = np.stack([X0 + 15.0 + dx, rs.uniform(Y0 + 6.0, Y0 + 9.0, n)], axis=1)
    inv = np.zeros((n, 2, 2))
    inv[:, 0, 0], inv[:, 1, 1] = 1.0 / sx ** 2, 1.0 / sy ** 2
    return means, inv, op_arg, np.ones((n, 3))


@pytest.mark.parametrize("lead", [0, 64])
def test_the_skip_budget_runs_out_on_either_side_of_a_seam(lead):
    """A block's budget (kSkipBudget = 2^23 units) takes 512 class-1 records at 2^14 units each, so it cannot run out inside
    the first 128 entries of a list; here every sub-batch of 64 holds 55 such records for the tile's right blocks (and 9
    near ones, so that every sub-batch stages something): nine sub-batches fit (495), the tenth does not.  With lead = 0
    that is the sub-batch of entries 576 .. 639, the SECOND half of the pair 512 .. 639; with lead = 64 (64 near records in
    front) the FIRST half of the pair 640 .. 767.  From there on the right blocks keep what they skipped before -- decided per
    sub-batch, in list order, against the running total --, which the host restatement confirms before the GPU is asked."""
    _need_gpu()
    rs = np.random.RandomState(77 + lead)
    parts = [_round(rs, lead, sigma=(1.0, 2.0))] if lead else []
    for k in range(12):
        far, near = _far_records(rs, 55), _round(rs, 9, sigma=(1.0, 2.0))
        order = rs.permutation(64)
        parts.append(tuple(np.concatenate([a, b])[order] for a, b in zip(far, near)))
    means, inv, op_arg, colors = (np.concatenate([p[i] for p in parts]) for i in range(4))
    bounds = _block_bounds(means, inv, op_arg)
    assert _clear_of_limits(bounds)
    counts, thrs = _stage(bounds)
    first = lead // 64
    out = first + 9                                # the sub-batch in which the right blocks (1, 3) run out
    assert (out % 2 == 1) == (lead == 0)           # lead = 0: the second half of a pair; lead = 64: the first
    for g in (1, 3):
        assert np.all(thrs[first:out, g] == -26.0) and np.all(thrs[out:, g] == -33.0), (g, thrs[:, g])
        assert np.all(counts[first:out, g] <= 9) and np.all(counts[out:, g] >= 55), (g, counts[:, g])
    for g in (0, 2):
        assert np.all(thrs[:, g] == -26.0), (g, thrs[:, g])
    assert _nothing_saturates(means, inv, op_arg)          # (the sub-batches around the seam are still paired)
    pre = _pre(means, inv, op_arg, colors)
    img = _both_instances(pre, "skip budget, lead %d" % lead)
    _against_c(pre, img, "skip budget, lead %d" % lead)


# ---- saturation in each half

def _flat(rs, n, alpha):
    """n broad footprints (sigma 40 px, centred on the tile's corner pixel (0, 0)) of peak alpha `alpha`: T falls by that factor per record."""
    means = np.tile(np.array([[X0 + 0.0, Y0 + 0.0]]), (n, 1)) + rs.uniform(-0.01, 0.01, (n, 2))
    inv = np.zeros((n, 2, 2))
    inv[:, 0, 0] = inv[:, 1, 1] = 1.0 / 40.0 ** 2
    a = np.full(n, alpha)
    return means, inv, np.log(a / (1.0 - a)), rs.uniform(0.05, 1.0, (n, 3))


@pytest.mark.parametrize("entry", [30, 90, 140])
def test_the_first_pixel_saturates_in_either_half(entry):
    """200 broad records of equal peak alpha a, 1 - a = 10^(-6 / entry): the first pixel of the tile stops at list entry
    ~entry -- in the first half of the first pair, in its second half, in the next pair -- and the others follow record
    by record (host restatement: the entry at which the first and the last pixel stop)."""
    _need_gpu()
    rs = np.random.RandomState(entry)
    means, inv, op_arg, colors = _flat(rs, 200, 1.0 - 10.0 ** (-6.0 / entry))
    T = _transmittance(means, inv, op_arg)
    dead = (T.reshape(T.shape[0], -1) == 0.0)
    first, last = int(np.argmax(dead.any(axis=1))), int(np.argmax(dead.all(axis=1)))
    print("saturation: first pixel stops in front of entry %d, the last in front of entry %d" % (first, last))
    assert abs(first - entry) <= 3 and first < last <= 199
    pre = _pre(means, inv, op_arg, colors)
    img = _both_instances(pre, "saturation at %d" % entry)
    _against_c(pre, img, "saturation at %d" % entry)


def test_one_block_dies_in_the_first_half_while_the_others_live_on():
    """50 opaque records of sigma 3.5 px on the middle of block 0 and then 150 round ones all over the tile: every pixel of
    block 0 has stopped before entry 64, every other block still has live pixels after the last entry (host restatement).
    The pair of entries 0 .. 127 notices the dead block at its end only; what block 0 walks of its second half adds 0."""
    _need_gpu()
    rs = np.random.RandomState(11)
    n0 = 50
    m0 = np.tile(np.array([[X0 + 3.5, Y0 + 3.5]]), (n0, 1)) + rs.uniform(-0.05, 0.05, (n0, 2))
    i0 = np.zeros((n0, 2, 2))
    i0[:, 0, 0] = i0[:, 1, 1] = 1.0 / 3.5 ** 2
    m1, i1, o1, c1 = _round(rs, 150)
    means, inv = np.concatenate([m0, m1]), np.concatenate([i0, i1])
    op_arg, colors = np.concatenate([np.full(n0, 30.0), o1]), np.concatenate([rs.uniform(0.05, 1.0, (n0, 3)), c1])
    T = _transmittance(means, inv, op_arg)
    assert np.all(T[60, 0:8, 0:8] == 0.0)                                  # block 0 is done inside the first sub-batch
    for blk in (T[-1, 8:16, 0:8], T[-1, 0:8, 8:16], T[-1, 8:16, 8:16]):
        assert blk.max() > 1e-3                                            # the others live on to the end
    pre = _pre(means, inv, op_arg, colors)
    img = _both_instances(pre, "block 0 dies")
    _against_c(pre, img, "block 0 dies")


# ---- a flagged record in each half (REF instance only)

# the conic of tests/test_hip_parity.py::test_conic_whose_float32_determinant_cancelled_takes_the_reference_order: a 290:1
# needle whose ridge runs through its mean, which lies in the tile
NEEDLE_CONIC = np.array([[16.614168167114258, -24.628461837768555], [-24.628463745117188, 36.50867462158203]])
NEEDLE_OP = 0.011413033120334148
WILD_CONIC = np.array([[0.010, 0.012], [0.012, 0.010]])       # Q00 Q11 < Q01^2: D1 < 0, alpha may exceed the opacity factor


def _with_special(rs, n, at, conic, op, mean):
    means, inv, op_arg, colors = _round(rs, n)        # (small footprints: most pixels are still live at the end of the list)
    for k, q, o, m in zip(at, conic, op, mean):
        means[k], inv[k], op_arg[k] = m, q, o
    return means, inv, op_arg, colors


def _needle_stays_flagged(mean, conic, op_arg):
    """stage_records' test on the tile's rectangle: the reference's rounding can move alpha by 2e-5 or more."""
    c = 0.5 * np.log2(np.e)
    m00, m01, m11 = c * conic[0, 0], c * 0.5 * (conic[0, 1] + conic[1, 0]), c * conic[1, 1]
    r11 = np.sqrt(m11)
    h = m01 / r11
    d1 = m00 - h * h
    bx, by = mean[0] - X0, mean[1] - Y0
    ex, ey = max(abs(bx), abs(bx - 15.0)), max(abs(by), abs(by - 15.0))
    S = np.log(2.0) * ((d1 + h * h) * ex * ex + 2.0 * abs(h) * r11 * ex * ey + r11 * r11 * ey * ey)
    delta = 2.4e-7 * S
    amax = _sigmoid(op_arg)                        # (the mean, hence the ridge, lies inside the tile: the exponent reaches 0)
    return delta >= 0.2 or delta * amax >= 4e-5     # (twice the kernel's limits: clear of them)


@pytest.mark.parametrize("at", [10, 70, 127, 128])
def test_a_flagged_record_in_either_half(at):
    """150 round records with the needle as list entry `at`: in the first half of the first pair, in its second half, as its
    last entry, as the first entry of the next pair.  The needle stays flagged on this tile (host restatement of
    stage_records' test), so n_redo = 1: the one tile that holds a still-flagged record."""
    _need_gpu()
    rs = np.random.RandomState(300 + at)
    mean = np.array([X0 + 7.3, Y0 + 8.4])
    assert _needle_stays_flagged(mean, NEEDLE_CONIC, NEEDLE_OP)
    means, inv, op_arg, colors = _with_special(rs, 150, [at], [NEEDLE_CONIC], [NEEDLE_OP], [mean])
    assert _nothing_saturates(means, inv, op_arg)
    pre = _pre(means, inv, op_arg, colors)
    img, st = _render(pre)
    assert st["n_redo"] == 1, st
    ref = _against_c(pre, img.cpu().numpy(), "needle at %d" % at)
    # (the needle is in the picture: without it the frame is another one)
    keep = np.arange(150) != at
    without = _pre(means[keep], inv[keep], op_arg[keep], colors[keep])
    from oracle import c_oracle
    assert float(np.abs(c_oracle.render(without, FRAME, FRAME, TILE)[0] - ref).max()) > 10 * PIXEL_TOL


@pytest.mark.parametrize("needle_at,wild_at", [(20, 100), (100, 20), (127, 128), (128, 127)])
def test_a_flagged_record_in_one_half_and_a_wild_one_in_the_other(needle_at, wild_at):
    """The same with a D1 < 0 record (a conic of negative determinant: the reference's exponent can be positive) in the
    other half, and across the seam between two pairs."""
    _need_gpu()
    rs = np.random.RandomState(500 + needle_at)
    mean = np.array([X0 + 7.3, Y0 + 8.4])
    means, inv, op_arg, colors = _with_special(rs, 150, [needle_at, wild_at], [NEEDLE_CONIC, WILD_CONIC], [NEEDLE_OP, -1.0],
                                               [mean, np.array([X0 + 9.0, Y0 + 5.0])])
    assert _nothing_saturates(means, inv, op_arg)
    pre = _pre(means, inv, op_arg, colors)
    img, st = _render(pre)
    assert st["n_redo"] == 1, st
    _against_c(pre, img.cpu().numpy(), "needle at %d, wild at %d" % (needle_at, wild_at))


# ---- the monomial fallback in the second half

def test_a_monomial_record_in_the_second_half_restarts_the_tile():
    """A caller-given conic with Q11 = 0 (no completed square: the monomial fallback) as entry 100 of 150 -- the second half
    of the first pair: the tile starts over on the scalar form.  Held against the C restatement, and against the same
    list with that record moved to entry 10: the record is a steep vertical bar at x' = 2 (Q00 = 20) whose alpha is exactly 0
    from x' = 6 on (its exponent is below -150: exp2 gives 0), so from there the two orders composite the same records in
    the same order and the columns are bit-equal."""
    _need_gpu()
    rs = np.random.RandomState(9)
    bar = np.array([[20.0, 0.0], [0.0, 0.0]])
    mean = np.array([X0 + 2.0, Y0 + 8.0])
    means, inv, op_arg, colors = _with_special(rs, 150, [100], [bar], [1.0], [mean])
    assert _nothing_saturates(means, inv, op_arg)
    pre = _pre(means, inv, op_arg, colors)
    img, st = _render(pre)
    assert st["n_redo"] == 0
    _against_c(pre, img.cpu().numpy(), "monomial at 100")
    assert 0.5 * 20.0 * 4.0 ** 2 * np.log2(np.e) > 160.0           # 4 px from the bar the exponent is below float32's range
    perm = np.concatenate([np.arange(10), [100], np.arange(10, 100), np.arange(101, 150)])
    assert _nothing_saturates(means[perm], inv[perm], op_arg[perm])
    moved = _pre(means[perm], inv[perm], op_arg[perm], colors[perm])
    img2, st2 = _render(moved)
    assert st2["n_redo"] == 0
    _against_c(moved, img2.cpu().numpy(), "monomial at 10")
    assert torch.equal(img[X0 + 6:], img2[X0 + 6:])


# ---- cost words

@pytest.mark.parametrize("length", LENGTHS)
def test_cost_words_are_the_sum_over_sub_batches_of_64(tmp_path, monkeypatch, length):
    """hints.lens[t], what the next frame's schedule and its choice of long tiles are made from, stays
    sum over 64-record sub-batches (longest of the sub-batch's four block counts + kBatchCost) whether or not two
    sub-batches were staged together.  Whole path (only there does a frame keep a hints buffer, and only from 16 385
    Gaussians): the 48x48 frame under the identity pose, `length` round Gaussians at rising depths with their means inside
    tile (1, 1) -- its list is exactly these -- and the rest behind the camera.  The block membership comes from the C restatement's stage-1 arrays of the same scene (which
    the library's are bit-equal to), every bound clear of the class limits; both instances leave the same word."""
    _need_gpu()
    from intro_to_gaussian_splatting_amd import gaussian_scene as wrapper
    from intro_to_gaussian_splatting_amd.synthetic import make_scene
    from intro_to_gaussian_splatting_amd import GaussianScene, Gaussians
    from intro_to_gaussian_splatting_amd.synthetic import write_colmap_text
    from oracle import c_oracle, cpu_ref

    n = 16_385 + 300
    sc = make_scene(n, FRAME, FRAME, seed=length, qvec=(1.0, 0.0, 0.0, 0.0), tvec=(0.0, 0.0, 0.0))
    rs = np.random.RandomState(2000 + length)
    fx = float(sc["fx"])
    tan = FRAME / (2.0 * fx)
    pts, scales = sc["points"].copy(), sc["scales"].copy()
    pts[:] = np.array([0.0, 0.0, -5.0], np.float32)                # behind the camera
    z = 2.0 + 0.01 * np.arange(length)
    scales[:length] = (rs.uniform(0.6, 1.2, length) * z / fx)[:, None]
    sc["scales"], sc["opacity"] = scales.astype(np.float32), np.full((n, 1), -1.0, np.float32)

    def build(where, points):
        write_colmap_text(str(where), dict(sc, points=points))
        return GaussianScene(str(where), Gaussians.from_arrays(points, sc["colors_0_255"], sc["scales"], sc["quaternions"],
                                                               sc["opacity"], device="cuda:0"))

    scene = build(tmp_path / "camera", pts.astype(np.float32))     # (nothing in view yet: the camera and the colours)
    im, c = scene.images[1], scene.images[1].gsx_camera()
    cam = cpu_ref.Camera(im.world2view.cpu().numpy(), im.full_proj_transform.cpu().numpy(), np.float32(c.tan_fovx),
                         np.float32(c.tan_fovy), np.float32(c.fx), np.float32(c.fy), c.width, c.height)
    colors = scene.gaussians.colors.cpu().numpy()
    # means inside tile (1, 1) (pixels 17.3 .. 30.7); a Gaussian one of whose four bounds comes within 0.005 of a class limit
    # -- float32 could decide it either way -- is drawn again
    redraw = np.ones(length, bool)
    for _ in range(50):
        k = int(redraw.sum())
        u, v = rs.uniform(-0.28, 0.28, k), rs.uniform(-0.28, 0.28, k)
        pts[:length][redraw] = np.stack([u * tan * z[redraw], v * tan * z[redraw], z[redraw]], axis=1)
        pre = c_oracle.preprocess(pts.astype(np.float32), colors, sc["scales"], sc["quaternions"], sc["opacity"], cam)
        assert pre.points.shape[0] == length and np.array_equal(np.asarray(pre.order), np.arange(length))
        means, inv = np.asarray(pre.points, np.float64), np.asarray(pre.inverse_covariance_2d, np.float64)
        op_arg = np.asarray(pre.sigmoid_opacity, np.float64).reshape(-1)
        bounds = _block_bounds(means, inv, op_arg)
        redraw = np.array([not _clear_of_limits(b) for b in bounds])
        if not redraw.any():
            break
    assert _clear_of_limits(bounds)
    assert np.all((means > X0 + 0.5) & (means < X0 + 15.5))
    sc["points"] = pts.astype(np.float32)
    scene = build(tmp_path / "scene", sc["points"])
    _, _, inst = c_oracle.render(pre, FRAME, FRAME, TILE)
    assert _transmittance(means, inv, op_arg)[-1].min() > 1e-5        # nothing saturates: every sub-batch is walked
    counts, thrs = _stage(bounds)
    assert np.all(thrs == -26.0)
    want = int(sum(int(c.max()) + BATCH_COST for c in counts))
    if length >= 63:
        assert counts.sum() < 4 * length                                          # the blocks' lists differ from the tile's
    lens_at = (64 + 256 + 2048) * 4          # csrc/gsx_plan.h: hints_layout (header, splitters, samples, then the tiles' costs)

    def cost_word():
        torch.cuda.synchronize()
        slots = [s for s in scene._hints._d.values()] if hasattr(scene._hints, "_d") else list(scene._hints.values())
        assert len(slots) == 1
        # (tile ids are column-major: tile (1, 1) of the 2 x 2 tiles the reference renders of a 48x48 frame is tile 3)
        return int(slots[0][0][lens_at:lens_at + 16].cpu().numpy().view(np.uint32)[3])

    st = {}
    a = scene.render_image_hip(1, stats=st).clone()
    assert st["n_instances"] == inst and st["n_redo"] == 0 and not st["plain_footprints"]
    got = cost_word()
    print("cost word, L = %d: %d (host: %d; per sub-batch %s)" % (length, got, want, counts.max(axis=1).tolist()))
    assert got == want
    monkeypatch.setattr(wrapper, "_PLAIN_MIN_TILES", 1)
    st = {}
    b = scene.render_image_hip(1, stats=st)
    assert st["plain_footprints"] and st["n_redo"] == 0 and torch.equal(a, b)
    assert cost_word() == want
