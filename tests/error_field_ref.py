"""The misprediction field (`dsnt_error_field`, include/dsnt_hip.h) restated in plain numpy, and the inputs its tests share.

`restate` is a double loop over `n` then `j` in fp64: the order in which the entry promises to add, so the fp64 sums it
returns are what the kernel must hold bit for bit.  Reference `bin/investigate.py:62-99` is the same computation, on
the valid joints whose normalised target lies in [-1, 1]^2.
"""
import numpy as np

MASKS = np.array([0, 1, 1, 1, 0.5, 2], np.float32)


def edges_of(bins):
    """The edges `dsnt.evaluator.ErrorField` uses, and `binned_statistic_dd(bins=bins, range=[[-1, 1]] * 2)` too."""
    return np.linspace(-1, 1, bins + 1)


def cell_of(t, edges):
    """The number of edges[1..bins] that are <= t, capped at bins - 1: e_k <= t < e_{k+1}, the last edge closed."""
    return min(int((edges[1:] <= t).sum()), len(edges) - 2)


def distance(pred, target, m, b, head):
    """`pckh_distance` (csrc/pckh.hip) on whole arrays: bmm(x, m) + b on row vectors, the distance over the head length."""
    with np.errstate(all='ignore'):
        p = np.einsum('bji,bik->bjk', pred.astype(np.float64), m) + b[:, None, :]
        t = np.einsum('bji,bik->bjk', target.astype(np.float64), m) + b[:, None, :]
        return np.sqrt((p[..., 0] - t[..., 0]) ** 2 + (p[..., 1] - t[..., 1]) ** 2) / head[:, None]


def in_frame(target, mask, edges):
    """[B, J] bool: the joints that count (mask == 1, both target coordinates inside the closed frame; NaN is outside)."""
    t = target.astype(np.float64)
    with np.errstate(invalid='ignore'):
        inside = (edges[0] <= t) & (t <= edges[-1])
    return (mask == 1) & inside[..., 0] & inside[..., 1]


def empty(J, bins):
    """(total, miss, miss_finite, sum_x, sum_y), all zero."""
    shape = (J, bins, bins)
    return (np.zeros(shape, np.int64), np.zeros(shape, np.int64), np.zeros(shape, np.int64),
            np.zeros(shape, np.float64), np.zeros(shape, np.float64))


def restate(pred, target, m, b, mask, head, threshold, edges, start=None, order=None):
    """(total, miss, miss_finite, sum_x, sum_y), each [J, bins, bins] with cells [by, bx], after the samples were added
    to `start` (default: zeros) in the order `order` (default: ascending n)."""
    B, J = mask.shape
    bins = len(edges) - 1
    total, miss, miss_finite, sum_x, sum_y = [a.copy() for a in (start or empty(J, bins))]
    thr = float(np.float32(threshold))
    lo, hi = float(edges[0]), float(edges[-1])
    with np.errstate(all='ignore'):
        for n in (range(B) if order is None else order):
            mm, bb = m[n], b[n]
            for j in range(J):
                px, py = np.float64(pred[n, j, 0]), np.float64(pred[n, j, 1])
                tx, ty = np.float64(target[n, j, 0]), np.float64(target[n, j, 1])
                if not (mask[n, j] == 1 and lo <= tx <= hi and lo <= ty <= hi):
                    continue
                cy, cx = cell_of(ty, edges), cell_of(tx, edges)
                total[j, cy, cx] += 1
                ox, oy = px * mm[0, 0] + py * mm[1, 0] + bb[0], px * mm[0, 1] + py * mm[1, 1] + bb[1]
                gx, gy = tx * mm[0, 0] + ty * mm[1, 0] + bb[0], tx * mm[0, 1] + ty * mm[1, 1] + bb[1]
                d = np.sqrt((ox - gx) * (ox - gx) + (oy - gy) * (oy - gy)) / np.float64(head[n])
                if d <= thr:
                    continue
                miss[j, cy, cx] += 1
                dx, dy = px - tx, py - ty
                if np.isfinite(dx) and np.isfinite(dy):
                    miss_finite[j, cy, cx] += 1
                    sum_x[j, cy, cx] += dx
                    sum_y[j, cy, cx] += dy
    return total, miss, miss_finite, sum_x, sum_y


def _rest(r, B, J):
    """The transform of `test_pckh_curve_gpu._case`, the head lengths and the masks, drawn in that order."""
    m = np.array([[150.0, 90.0], [-20.0, 60.0]]) + r.uniform(-10, 10, (B, 2, 2))
    b = r.uniform(0, 400, (B, 2))
    head = r.uniform(40, 120, B)
    mask = r.choice(MASKS, (B, J))
    return m, b, mask, head


def spread(B, J, seed=None):
    """Targets over [-1.15, 1.15]^2 (about a quarter outside the frame), about a third of the valid ones missed."""
    r = np.random.default_rng(B * 100 + J if seed is None else seed)
    target = r.uniform(-1.15, 1.15, (B, J, 2)).astype(np.float32)
    pred = (target + r.normal(0, 0.2, (B, J, 2))).astype(np.float32)
    return (pred, target) + _rest(r, B, J)


def crowded(B, J, seed=None):
    """The same noise around targets in [-0.25, 0.25]^2: every target in frame, a few cells with many samples each."""
    r = np.random.default_rng(B * 100 + J if seed is None else seed)
    target = r.uniform(-0.25, 0.25, (B, J, 2)).astype(np.float32)
    pred = (target + r.normal(0, 0.2, (B, J, 2))).astype(np.float32)
    return (pred, target) + _rest(r, B, J)


def wide(B, J, seed=None):
    """`crowded` targets with offsets over twelve orders of magnitude: fp64 sums that depend on the order of the adds."""
    r = np.random.default_rng(B * 100 + J if seed is None else seed)
    target = r.uniform(-0.25, 0.25, (B, J, 2)).astype(np.float32)
    noise = r.normal(0, 1, (B, J, 2))
    pred = (target + noise * 10 ** r.uniform(-3, 9, (B, J, 1))).astype(np.float32)
    return (pred, target) + _rest(r, B, J)
