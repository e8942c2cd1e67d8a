"""Helpers to compare tensors with the summaries stored in tests/golden/*.npz."""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, name + '.npz'))


def check_summary(g, prefix, t, atol, rtol=0.0):
    """Sampled entries, sum and L2 norm of `t` against the golden summary `prefix`."""
    a = t.detach().double().cpu().reshape(-1).numpy()
    idx, val = g[prefix + '.idx'], g[prefix + '.val']
    scale = max(1.0, float(np.abs(val).max()))
    err = np.abs(a[idx] - val).max()
    assert err <= atol * scale + rtol * scale, (prefix, 'samples', err)
    l2 = float(g[prefix + '.l2'])
    got = float(np.sqrt((a * a).sum()))
    assert abs(got - l2) <= (atol * 50 + rtol) * max(1.0, l2), (prefix, 'l2', got, l2)
    return err


def check_segments(g, prefix, named, tol, scaled=True):
    """A list of (name, tensor) against the segment summary `prefix` (make_golden.segments).  Each tensor is held to
    max|a - ref| <= tol * scale (scale: max(1, max|ref|) of that tensor if `scaled`, else 1) on the stored samples and
    on max|.|; its L2 norm and sum to the bounds that elementwise bar implies (sqrt(n) * and n * tol * scale)."""
    assert [n for n, _ in named] == list(g[prefix + '.names']), prefix
    flat = [t.detach().double().cpu().reshape(-1).numpy() for _, t in named]
    assert [f.size for f in flat] == list(g[prefix + '.numel']), prefix
    scales = np.maximum(1.0, g[prefix + '.max']) if scaled else np.ones(len(flat))
    for i, f in enumerate(flat):
        bar = tol * scales[i]
        assert abs((np.abs(f).max() if f.size else 0.0) - g[prefix + '.max'][i]) <= bar, (prefix, named[i][0], 'max')
        assert abs(np.sqrt((f * f).sum()) - g[prefix + '.l2'][i]) <= bar * np.sqrt(f.size), (prefix, named[i][0], 'l2')
        assert abs(f.sum() - g[prefix + '.sum'][i]) <= bar * f.size, (prefix, named[i][0], 'sum')
    a = np.concatenate(flat)
    idx = g[prefix + '.idx'].astype(np.int64)
    seg = np.searchsorted(np.cumsum([f.size for f in flat]), idx, side='right')
    err = np.abs(a[idx] - g[prefix + '.val'])
    bad = err > tol * scales[seg]
    assert not bad.any(), (prefix, named[seg[bad.argmax()]][0], 'samples', float(err.max()))
