"""gsx_density_accumulate / gsx_density_plan / gsx_density_apply restated in numpy float32 (include/gsx.h), op for op: every
operation a numpy float32 operation, rounded on its own, divide and sqrt correctly rounded as numpy's are.  The three calls
must equal these bit for bit."""
import numpy as np

F = np.float32
KEEP, PRUNE, CLONE, SPLIT = 0, 1, 2, 3                      # the plan's actions
COPY, ZERO_NEW, POINTS, SCALES, QUATS = 0, 1, 2, 3, 4       # GSX_DENSITY_*
ROWS_OF = np.array([1, 0, 2, 2], np.int64)


def rules(grad_threshold, dense_scale, prune_logit, prune_scale, split_shrink=1.6):
    return dict(grad_threshold=F(grad_threshold), dense_scale=F(dense_scale), prune_logit=F(prune_logit),
                prune_scale=F(prune_scale), split_shrink=F(split_shrink))


def accumulate(grad, grad_sum, seen):
    """(grad_sum', seen'), new arrays: norm = sqrt(((g0 g0 + g1 g1) + g2 g2) + ...) added, and one counted, where the row has
    an element that is not +-0."""
    g = np.ascontiguousarray(grad, np.float32)
    g = g.reshape(g.shape[0], -1)
    with np.errstate(all="ignore"):
        total = g[:, 0] * g[:, 0]
        for k in range(1, g.shape[1]):
            total = total + g[:, k] * g[:, k]
        norm = np.sqrt(total)
        live = ((g.view(np.uint32) & np.uint32(0x7FFFFFFF)) != 0).any(axis=1)
        out_sum = np.array(grad_sum, np.float32)
        out_seen = np.array(seen, np.uint32)
        out_sum[live] = out_sum[live] + norm[live]
    out_seen[live] += np.uint32(1)
    assert out_sum.dtype == np.float32 and norm.dtype == np.float32
    return out_sum, out_seen


def plan(grad_sum, seen, scales, opacity_logit, r):
    """(action uint8 (n), prefix int64 (n), counts = (n_out, n_pruned, n_cloned, n_split))."""
    grad_sum = np.ascontiguousarray(grad_sum, np.float32)
    seen = np.ascontiguousarray(seen, np.uint32)
    s = np.ascontiguousarray(scales, np.float32).reshape(-1, 3)
    logit = np.ascontiguousarray(opacity_logit, np.float32).reshape(-1)
    n = s.shape[0]
    with np.errstate(all="ignore"):
        smax = np.maximum(np.maximum(s[:, 0], s[:, 1]), s[:, 2])                # (np.maximum hands a NaN on)
        prune = (logit < r["prune_logit"]) | (smax > r["prune_scale"])
        mean = grad_sum / np.where(seen > 0, seen, 1).astype(np.float32)
        assert mean.dtype == np.float32
        hot = (seen > 0) & (mean >= r["grad_threshold"])
        split = ~prune & hot & (smax > r["dense_scale"])
        clone = ~prune & hot & (smax <= r["dense_scale"])
    action = np.full(n, KEEP, np.uint8)
    action[prune], action[split], action[clone] = PRUNE, SPLIT, CLONE
    count = ROWS_OF[action]
    prefix = np.cumsum(count) - count
    return action, prefix.astype(np.int64), (int(count.sum()), int(prune.sum()), int(clone.sum()), int(split.sum()))


def rotation(q):
    """(n,3,3) float32: the rotation of (w, x, y, z) = q / nrm, the identity where !(nrm > 0); the header's nine formulas."""
    q = np.ascontiguousarray(q, np.float32).reshape(-1, 4)
    one, two = F(1.0), F(2.0)
    with np.errstate(all="ignore"):
        nrm = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        ok = nrm > 0
        w, x, y, z = (np.where(ok, q[:, i] / nrm, F(1.0 if i == 0 else 0.0)) for i in range(4))
        R = np.empty((q.shape[0], 3, 3), np.float32)
        R[:, 0, 0] = one - two * (y * y + z * z)
        R[:, 0, 1] = two * (x * y - w * z)
        R[:, 0, 2] = two * (x * z + w * y)
        R[:, 1, 0] = two * (x * y + w * z)
        R[:, 1, 1] = one - two * (x * x + z * z)
        R[:, 1, 2] = two * (y * z - w * x)
        R[:, 2, 0] = two * (x * z - w * y)
        R[:, 2, 1] = two * (y * z + w * x)
        R[:, 2, 2] = one - two * (x * x + y * y)
    assert w.dtype == np.float32
    return R


def source_rows(action, prefix, n_out):
    """(row int64 (n_out), child int64 (n_out), new bool (n_out), source_row int32 (n_out) as gsx_density_apply writes it)."""
    action = np.asarray(action, np.uint8)
    count = ROWS_OF[action]
    row = np.repeat(np.arange(action.shape[0], dtype=np.int64), count)
    assert row.shape[0] == n_out
    child = np.arange(n_out, dtype=np.int64) - np.asarray(prefix, np.int64)[row]
    new = (action[row] == SPLIT) | ((action[row] == CLONE) & (child == 1))
    return row, child, new, np.where(new, -(row + 1), row).astype(np.int32)


def apply(groups, action, prefix, n_out, noise, split_shrink):
    """groups: [(src (n, width), role)].  Returns ([dst (n_out, width)], source_row)."""
    row, child, new, src_row = source_rows(action, prefix, n_out)
    split = np.asarray(action)[row] == SPLIT
    by_role = {role: np.ascontiguousarray(src, np.float32) for src, role in groups}
    outs = []
    for src, role in groups:
        src = np.ascontiguousarray(src, np.float32)
        src = src.reshape(src.shape[0], -1)
        dst = src[row].copy()
        with np.errstate(all="ignore"):
            if role == ZERO_NEW:
                dst[new] = F(0.0)
            elif role == SCALES:
                dst[split] = src[row[split]] / F(split_shrink)
            elif role == POINTS:
                s = by_role[SCALES].reshape(-1, 3)[row[split]]
                R = rotation(by_role[QUATS].reshape(-1, 4)[row[split]])
                e = np.ascontiguousarray(noise, np.float32).reshape(-1, 2, 3)[row[split], child[split]]
                d = s * e
                for k in range(3):
                    dst[split, k] = src[row[split], k] + ((R[:, k, 0] * d[:, 0] + R[:, k, 1] * d[:, 1]) + R[:, k, 2] * d[:, 2])
        assert dst.dtype == np.float32
        outs.append(dst)
    return outs, src_row
