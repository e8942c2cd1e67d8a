"""numpy restatement of dsnt_pckh_boot (csrc/pckh.hip; the weight rule is in include/dsnt_hip.h and DESIGN.md section 20)
and of the readers of `dsnt.evaluator.PCKhBootstrap`.  Shared by tests/test_pckh_boot_cpu.py and
tests/test_pckh_boot_gpu.py.

The table is int64 `[R + 1][J][T + 1]`: copy 0 of `dsnt_pckh_hist`'s table with weight 1, copy r with the Poisson(1) weight
w(id, r) of the example.  Everything here is integer or fp64 numpy on the host.
"""
import os
import re

import numpy as np

import loader_ref

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dsnt_hip.h')
DOMAIN = 0x424F4F54
# c_k = floor(2^32 e^-1 sum_{i <= k} 1/i!), k = 0..11 (re-derived by tests/test_pckh_boot_cpu.py)
CDF = np.array([1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276,
                4294962463, 4294966817, 4294967252, 4294967292], np.uint64)


def header_macros():
    """The `DSNT_PCKH_BOOT_*` macros of include/dsnt_hip.h: name without the prefix -> int, or a list of ints."""
    out = {}
    for name, value in re.findall(r'^#define DSNT_PCKH_BOOT_(\w+)\s+(.+?)\s*$', open(HEADER).read(), flags=re.M):
        numbers = [int(v.rstrip('uU'), 0) for v in re.findall(r'0[xX][0-9A-Fa-f]+[uU]?|\d+[uU]?', value)]
        out[name] = numbers if value.startswith('{') else numbers[0]
    return out


def uniforms(ids, R, seed, domain=DOMAIN):
    """u of replicate 1..R for every id: uint64 [N, R] of 32-bit values.  Word (r - 1) & 3 of Philox4x32-10 with key
    (seed lo, seed hi) and counter (id lo, id hi, (r - 1) >> 2, domain); the id is an int64 taken as its 64 bits."""
    bits = np.asarray(ids, np.int64).reshape(-1).view(np.uint64)
    quads = (R + 3) // 4
    q = np.arange(quads, dtype=np.uint64)[None, :]
    words = loader_ref.philox4x32_10(bits[:, None] & loader_ref.M32, bits[:, None] >> np.uint64(32), q, domain, seed)
    return np.stack(words, axis=-1).reshape(len(bits), 4 * quads)[:, :R]


def weights(ids, R, seed):
    """w(id, r) for r = 0..R: int64 [N, R + 1].  Column 0 is 1; otherwise the number of c_k that u reaches."""
    u = uniforms(ids, R, seed)
    w = (u[:, :, None] >= CDF[None, None, :]).sum(-1).astype(np.int64)
    return np.concatenate((np.ones((len(w), 1), np.int64), w), axis=1)


def table(columns, valid, ids, R, seed, J, T):
    """int64 [R + 1, J, T + 1]: joint j of example n, where `valid`, adds w(ids[n], r) to [r][j][columns[n, j]]."""
    columns, valid = np.asarray(columns).reshape(-1, J), np.asarray(valid, bool).reshape(-1, J)
    w = weights(ids, R, seed)
    out = np.zeros((R + 1, J, T + 1), np.int64)
    for j in range(J):
        for k in range(T + 1):
            out[:, j, k] = w[valid[:, j] & (columns[:, j] == k)].sum(0)
    return out


def _split(tab, k, rows):
    """(hits, valid) per copy, int64 [R + 1]: the joints `rows` at threshold index k."""
    t = tab[:, rows].sum(1)
    return t[:, :k + 1].sum(1), t.sum(1)


def _ratio(num, den):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(den > 0, num.astype(np.float64) / den.astype(np.float64), np.nan)


def pckh(tab, k, rows):
    hits, n = _split(tab, k, rows)
    return float(_ratio(hits[:1], n[:1])[0])


def replicates(tab, k, rows):
    """fp64 [R]: weighted hits / weighted valid of every replicate, NaN where valid is 0."""
    hits, n = _split(tab, k, rows)
    return _ratio(hits[1:], n[1:])


def stderr(tab, k, rows):
    v = replicates(tab, k, rows)
    return float(np.std(v[np.isfinite(v)], ddof=1))


def _quantiles(v, level):
    v = v[np.isfinite(v)]
    lo, hi = np.quantile(v, [(1 - level) / 2, 1 - (1 - level) / 2], method='linear')
    return float(lo), float(hi)


def interval(tab, k, rows, level=0.95):
    return _quantiles(replicates(tab, k, rows), level)


def compare(tab_a, tab_b, k, rows, level=0.95):
    """`PCKhBootstrap.compare` on two tables over the same examples."""
    assert np.array_equal(tab_a.sum(2), tab_b.sum(2))
    d = replicates(tab_a, k, rows) - replicates(tab_b, k, rows)
    d = d[np.isfinite(d)]
    return {'diff': pckh(tab_a, k, rows) - pckh(tab_b, k, rows), 'interval': _quantiles(d, level),
            'stderr': float(np.std(d, ddof=1)), 'p_greater': float(((d > 0).sum() + 0.5 * (d == 0).sum()) / d.size)}
