"""numpy restatement of `dsnt_map_modes` (include/dsnt_hip.h), operation for operation, and the seeded
inputs the CPU and GPU tests share.

  * window scores: fp32, `s = sum_d shift_x(p, d)` then `S = sum_d shift_y(s, d)`, the zero-padded shifts added in ascending
    d onto an accumulator of +0: every add a separately rounded fp32 add, as in the kernel;
  * modes: `np.argmax` (the first maximum) of S with NaN and the centres within 2r (Chebyshev) of an earlier mode masked
    to -inf; -1 when nothing is left above -inf;
  * window sums: fp64 in the kernel's order: per window row in ascending x from +0 (`sm += p; sx += X * p; sy += Y * p`, the
    products rounded first), then the rows that lie in the map in ascending y from +0.
`exact()` evaluates a chosen window without rounding: `math.fsum` over p and over the products (2x + 1 - w) p, which are
exact in fp64 (a 13-bit integer times a 24-bit significand)."""
import functools
import math

import numpy as np

NAN32 = np.float32(np.nan)


def _shift(a, d, axis):
    """a shifted so that out[i] = a[i + d] along `axis`, +0 outside."""
    out = np.zeros_like(a)
    n = a.shape[axis]
    if abs(d) >= n:
        return out
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[axis] = slice(max(d, 0), n + min(d, 0))
    dst[axis] = slice(max(-d, 0), n + min(-d, 0))
    out[tuple(dst)] = a[tuple(src)]
    return out


def scores(p, r):
    """S f32 [n, h, w] of p f32 [n, h, w]."""
    p = np.asarray(p, np.float32)
    with np.errstate(all='ignore'):
        s = np.zeros_like(p)
        for d in range(-r, r + 1):
            s = s + _shift(p, d, 2)
        S = np.zeros_like(p)
        for d in range(-r, r + 1):
            S = S + _shift(s, d, 1)
    assert S.dtype == np.float32
    return S


def choose(S, r, K):
    """index int32 [n, K]."""
    n, h, w = S.shape
    yy, xx = np.arange(h).reshape(1, h, 1), np.arange(w).reshape(1, 1, w)
    cand = np.where(np.isnan(S), -np.inf, S).astype(np.float32)
    index = np.full((n, K), -1, np.int32)
    for k in range(K):
        flat = cand.reshape(n, -1)
        first = np.argmax(flat, 1)
        won = flat[np.arange(n), first] > -np.inf
        index[:, k] = np.where(won, first, -1)
        yc, xc = (first // w).reshape(n, 1, 1), (first % w).reshape(n, 1, 1)
        near = np.maximum(np.abs(yy - yc), np.abs(xx - xc)) <= 2 * r
        cand = np.where(near & won.reshape(n, 1, 1), np.float32(-np.inf), cand)
    return index


def window_sums(p, index, r):
    """(sum p, sum X p, sum Y p) f64 [3, n] over the clipped window about `index` [n] (>= 0), in the kernel's order."""
    n, h, w = p.shape
    P = np.asarray(p, np.float64)
    yc, xc, rows = index // w, index % w, np.arange(n)
    tot = np.zeros((3, n))
    with np.errstate(all='ignore'):
        for dy in range(-r, r + 1):
            y = yc + dy
            in_y, y = (y >= 0) & (y < h), np.clip(y, 0, h - 1)
            Y = (2 * y + 1) / h - 1.0
            acc = np.zeros((3, n))
            for dx in range(-r, r + 1):
                x = xc + dx
                inside, x = in_y & (x >= 0) & (x < w), np.clip(x, 0, w - 1)
                X = (2 * x + 1) / w - 1.0
                v = P[rows, y, x]
                acc = np.where(inside, acc + np.stack([v, X * v, Y * v]), acc)
            tot = np.where(in_y, tot + acc, tot)
    return tot


def modes(p, r, K, J=1, tm=None, tb=None):
    """The outputs of dsnt_map_modes for p f32 [n, h, w]: index i32 [n, K], mass f32 [n, K], coords f32 [n, K, 2] and, with
    tm f64 [n / J, 2, 2] and tb f64 [n / J, 2], image f64 [n, K, 2]."""
    p = np.ascontiguousarray(p, np.float32)
    n, h, w = p.shape
    index = choose(scores(p, r), r, K)
    mass = np.full((n, K), NAN32, np.float32)
    coords = np.full((n, K, 2), NAN32, np.float32)
    with np.errstate(all='ignore'):
        for k in range(K):
            have = index[:, k] >= 0
            sm, sx, sy = window_sums(p, np.where(have, index[:, k], 0), r)
            mass[:, k] = np.where(have, sm.astype(np.float32), NAN32)
            pos = have & (sm > 0)
            coords[:, k, 0] = np.where(pos, (sx / sm).astype(np.float32), NAN32)
            coords[:, k, 1] = np.where(pos, (sy / sm).astype(np.float32), NAN32)
        out = {'index': index, 'mass': mass, 'coords': coords}
        if tm is not None:
            M = np.repeat(np.asarray(tm, np.float64).reshape(-1, 2, 2), J, 0)[:, None]         # [n, 1, 2, 2]
            t = np.repeat(np.asarray(tb, np.float64).reshape(-1, 2), J, 0)[:, None]
            x, y = coords[..., 0].astype(np.float64), coords[..., 1].astype(np.float64)
            out['image'] = np.stack([t[..., 0] + (x * M[..., 0, 0] + y * M[..., 1, 0]),
                                     t[..., 1] + (x * M[..., 0, 1] + y * M[..., 1, 1])], -1)
    return out


def exact(p, index, r):
    """(mass, cx, cy, sum |p|, n) of the clipped window about `index` of ONE map p f32 [h, w], to fp64 rounding of the exact
    values."""
    h, w = p.shape
    yc, xc = divmod(int(index), w)
    ys, xs = range(max(0, yc - r), min(h, yc + r + 1)), range(max(0, xc - r), min(w, xc + r + 1))
    vals = [(y, x, float(p[y, x])) for y in ys for x in xs]
    m = math.fsum(v for _, _, v in vals)
    sx = math.fsum((2 * x + 1 - w) * v for _, x, v in vals)        # exact products, exactly summed
    sy = math.fsum((2 * y + 1 - h) * v for y, _, v in vals)
    cx, cy = (sx / (w * m), sy / (h * m)) if m > 0 else (math.nan, math.nan)
    return m, cx, cy, math.fsum(abs(v) for _, _, v in vals), len(vals)


# ------------------------------------------------------------------ inputs
def bimodal(h=64, w=64, weights=(0.6, 0.4), centres=((20.3, 30.7), (44.6, 31.2)), sigma=1.0):
    """The mixture of the issue's prototype: two Gaussian bumps at (x, y) pixel centres, each normalised over the map."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((h, w))
    for wt, (cx, cy) in zip(weights, centres):
        g = np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sigma * sigma))
        out += wt * g / g.sum()
    return out.astype(np.float32)


def softmax_maps(n, h, w, T, rng):
    z = rng.standard_normal((n, h * w)) * T
    e = np.exp(z - z.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32).reshape(n, h, w)


N_ROWS = 48          # 3 samples of 16 joints
# 1 x 1; odd sizes off the tile; more than one pixel per thread; w % 4 != 0 (scalar loads) over 16 pixels a thread; the
# production map; the limit DSNT_MODES_MAX_PIXELS
SHAPES = [(1, 1), (5, 9), (7, 7), (16, 16), (63, 65), (64, 64), (64, 128)]
RADII = (0, 1, 3, 8)
COUNTS = (1, 2, 4)


@functools.lru_cache(maxsize=None)
def seeded_maps(h, w):
    """The 48 maps [48, h, w] every test of a shape runs on (read-only): rows 0..23 softmax of randn T for T = 0.3, 3, 30
    (8 each), 24..27 the bimodal mixture scaled to the map (and its mirror images), 28..31 one-hot at the four corners, 32
    one-hot inside, 33 a constant map (ties through border clipping), 34 all zero, 35 all NaN, 36..38 a softmax with one NaN
    pixel / a NaN block / zeros in the rest, 39..43 softmax minus half the uniform level (negative pixels), 44 all
    negative, 45 two exactly equal bumps (an exact tie of S), 46..47 softmax T = 3."""
    rng = np.random.RandomState(1000 * h + w)
    p = np.zeros((N_ROWS, h, w), np.float32)
    for k, T in enumerate((0.3, 3.0, 30.0)):
        p[8 * k:8 * k + 8] = softmax_maps(8, h, w, T, rng)
    sx, sy = w / 64.0, h / 64.0
    two = bimodal(h, w, centres=((20.3 * sx, 30.7 * sy), (44.6 * sx, 31.2 * sy)), sigma=max(0.5, min(sx, sy)))
    p[24], p[25], p[26], p[27] = two, two[:, ::-1], two[::-1], two[::-1, ::-1]
    for k, (y, x) in enumerate(((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 3))):
        p[28 + k, y, x] = 1.0
    p[33] = np.float32(1.0 / (h * w))
    p[35] = np.nan
    p[36:39] = softmax_maps(3, h, w, 3.0, rng)
    p[36, h // 2, w // 2] = np.nan
    p[37, : (h + 1) // 2, : (w + 1) // 2] = np.nan
    p[38][p[38] < np.median(p[38])] = 0.0
    p[39:44] = softmax_maps(5, h, w, 3.0, rng) - np.float32(0.5 / (h * w))
    p[44] = -softmax_maps(1, h, w, 3.0, rng)[0]
    p[45, 0, 0] = p[45, h - 1, w - 1] = 0.25
    p[46:48] = softmax_maps(2, h, w, 3.0, rng)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def seeded_transforms(B=N_ROWS // 16):
    rng = np.random.RandomState(7)
    tm = np.eye(2) * 140 + 20 * rng.random_sample((B, 2, 2))
    tb = 200 * rng.random_sample((B, 2))
    tm.setflags(write=False)
    tb.setflags(write=False)
    return tm, tb


@functools.lru_cache(maxsize=None)
def seeded_modes(h, w, r):
    """modes(seeded_maps(h, w), r, K = 4) with the seeded transforms, J = 16: the modes of K < 4 are its first K (a mode
    depends on the earlier ones only).  Computed once per (shape, radius); read-only."""
    tm, tb = seeded_transforms()
    out = modes(seeded_maps(h, w), r, 4, 16, tm, tb)
    for v in out.values():
        v.setflags(write=False)
    return out
