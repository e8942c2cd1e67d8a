"""The per-joint heat-map statistics restated in numpy fp64 (the definition at the top of csrc/flipmerge.h, DESIGN
section 12), for tests/test_stats_cpu.py and tests/test_stats_gpu.py.

For one map p[y][x], h x w, on the DSNT grid X = (2x + 1)/w - 1, Y = (2y + 1)/h - 1: peak and the first flat index
holding it, mass = sum p, mean = (sum X p, sum Y p), cov = (vxx, vyy, vxy) as central sums about that mean (two sweeps),
and cov_image = M^T S M for a 2 x 2 `transform_m` M."""
import numpy as np


def grid(h, w):
    """X [h, w] and Y [h, w] in fp64."""
    x = (2.0 * np.arange(w) + 1.0) / w - 1.0
    y = (2.0 * np.arange(h) + 1.0) / h - 1.0
    return np.broadcast_to(x[None, :], (h, w)), np.broadcast_to(y[:, None], (h, w))


def cov_image(cov, m):
    """M^T S M in fp64, the products in the kernel's order: T = S M first, then M^T T.  `cov` [..., 3] = (vxx, vyy, vxy),
    `m` [..., 2, 2] broadcastable against it; returns [..., 2, 2]."""
    cov = np.asarray(cov, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64)
    a, d, c = cov[..., 0], cov[..., 1], cov[..., 2]
    m0, m1, m2, m3 = m[..., 0, 0], m[..., 0, 1], m[..., 1, 0], m[..., 1, 1]
    t00, t01 = a * m0 + c * m2, a * m1 + c * m3
    t10, t11 = c * m0 + d * m2, c * m1 + d * m3
    out = np.stack([m0 * t00 + m2 * t10, m0 * t01 + m2 * t11, m1 * t00 + m3 * t10, m1 * t01 + m3 * t11], -1)
    return out.reshape(out.shape[:-1] + (2, 2))


def stats_ref(hm, transform_m=None):
    """`hm` [..., h, w] (any float type, taken to fp64).  A dict of fp64 arrays over the leading dimensions: peak,
    peak_index (int64), mass, mean [..., 2], cov [..., 3], and cov_image [..., 2, 2] when `transform_m` ([..., 2, 2],
    broadcast over the leading dimensions) is given."""
    p = np.asarray(hm, dtype=np.float64)
    h, w = p.shape[-2:]
    flat = p.reshape(p.shape[:-2] + (h * w,))
    X, Y = grid(h, w)
    # numpy's max and argmax are torch.max's: the first maximum, and a NaN is the maximum (the first NaN the arg-max).  That is
    # the gauss decode's rule (`decode_row`); dsnt_heatmap_stats on a map with a NaN is not defined by this file
    out = {'peak': flat.max(-1), 'peak_index': flat.argmax(-1).astype(np.int64),
           'mass': flat.sum(-1)}
    mx, my = (X * p).sum((-2, -1)), (Y * p).sum((-2, -1))
    dx, dy = X - mx[..., None, None], Y - my[..., None, None]
    out['mean'] = np.stack([mx, my], -1)
    out['cov'] = np.stack([(dx * dx * p).sum((-2, -1)), (dy * dy * p).sum((-2, -1)), (dx * dy * p).sum((-2, -1))], -1)
    if transform_m is not None:
        out['cov_image'] = cov_image(out['cov'], transform_m)
    return out
