"""numpy restatement of the importance sampler (csrc/sampler.hip; contracts in include/dsnt_hip.h): the fixed-point
quantisation of fp32 row weights and its CDF, the counter-based weighted draw on `loader_ref.philox4x32_10`, and the
per-example scores in fp64.  The quantisation goes through fp64 `ldexp` and `floor` here and through shifts of the
significand on the device: two routes to the same integers.  Shared by tests/test_sampler_cpu.py,
tests/test_sampler_gpu.py and tests/test_weighted_loader_gpu.py."""
import numpy as np

import loader_ref

DOMAIN = 0x57534D50          # DSNT_SAMPLE_DOMAIN
MAX_N = 1 << 24              # DSNT_SAMPLE_MAX_N
TILE = 1024                  # DSNT_SAMPLE_TILE


def counted(w):
    """Which fp32 weights count: finite and positive (NaN, +-inf, negatives and zeros count as 0)."""
    w = np.asarray(w, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        return np.isfinite(w) & (w > 0)


def quantise(w):
    """q uint64 [n] = floor(w 2^(32 - e)), e the frexp exponent of the largest counted weight; all zero if none counts."""
    w = np.asarray(w, dtype=np.float32)
    ok = counted(w)
    q = np.zeros(w.shape, dtype=np.uint64)
    if not ok.any():
        return q
    _, e = np.frexp(np.float64(w[ok].max()))                 # wmax = f 2^e, f in [0.5, 1)
    scaled = np.ldexp(w[ok].astype(np.float64), 32 - int(e))     # a power of two: exact, and < 2^32
    q[ok] = np.floor(scaled).astype(np.uint64)
    return q


def cdf(w):
    """cdf uint64 [n]: the running sum of `quantise(w)` (below 2^56: exact)."""
    return np.cumsum(quantise(w), dtype=np.uint64)


def draw(c, seed, epoch, positions):
    """The row of every position (int64): the smallest j with c[j] > floor(u T / 2^64), u = o0 2^32 + o1 of Philox4x32-10
    with counter (p, epoch lo, epoch hi, DOMAIN); -1 everywhere if T = c[-1] is 0.  The high product is taken in Python
    integers."""
    c = np.asarray(c, dtype=np.uint64)
    p = np.asarray(positions, dtype=np.uint64)
    total = int(c[-1])
    if total == 0:
        return np.full(p.shape, -1, dtype=np.int64)
    o = loader_ref.philox4x32_10(p & loader_ref.M32, epoch & 0xFFFFFFFF, (epoch >> 32) & 0xFFFFFFFF, DOMAIN, seed)
    u = [(int(a) << 32) | int(b) for a, b in zip(o[0].reshape(-1), o[1].reshape(-1))]
    t = np.array([(x * total) >> 64 for x in u], dtype=np.uint64).reshape(p.shape)
    return np.searchsorted(c, t, side='right').astype(np.int64)


def distances(pred, target, m, b, head):
    """The PCKh distance of every joint, fp64 [B, J]: fp32 coordinates back-projected with `x @ m + b`, in head lengths."""
    pred, target = np.asarray(pred, np.float32).astype(np.float64), np.asarray(target, np.float32).astype(np.float64)
    m, b = np.asarray(m, np.float64), np.asarray(b, np.float64).reshape(-1, 1, 2)
    with np.errstate(invalid='ignore', divide='ignore'):
        o, g = pred @ m + b, target @ m + b
        return np.sqrt(((o - g) ** 2).sum(-1)) / np.asarray(head, np.float64)[:, None]


def example_scores(pred, target, m, b, mask, head):
    """score fp64 [B]: the mean of `distances` over the joints with mask == 1, summed in joint order; NaN with none."""
    d = distances(pred, target, m, b, head)
    mask = np.asarray(mask, np.float32)
    out = np.full(d.shape[0], np.nan)
    for n in range(d.shape[0]):
        s, k = 0.0, 0
        for j in range(d.shape[1]):
            if mask[n, j] == 1:
                s, k = s + d[n, j], k + 1
        if k:
            out[n] = s / k
    return out


def table_words(score32, idx, stamp, n, table=None):
    """The table after `dsnt_example_scores`: uint64 [n], max of (stamp << 32) | bits(score) over the examples with a
    finite score and a row inside [0, n); `table` is the state before (default: never seen)."""
    out = np.zeros(n, dtype=np.uint64) if table is None else np.array(table, dtype=np.uint64)
    bits = np.asarray(score32, dtype=np.float32).view(np.uint32)
    for s, v, r in zip(np.asarray(score32, dtype=np.float32), bits, np.asarray(idx)):
        if np.isfinite(s) and 0 <= r < n:
            out[r] = max(int(out[r]), (int(stamp) << 32) | int(v))
    return out
