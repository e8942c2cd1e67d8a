"""CPU checks of the per-joint heat-map statistics: the numpy restatement (tests/stats_ref.py) against hand-computed
cases and a closed form, the two new entry points at the C-ABI boundary, and the Python surface on CPU tensors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import stats_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dsnt_heatmap_stats', 'dsnt_flip_merge_head_stats')


# ------------------------------------------------------------------ the reference against hand-computed cases
def test_one_hot_map():
    h, w = 5, 8
    p = np.zeros((h, w))
    p[3, 6] = 1.0
    s = stats_ref.stats_ref(p)
    assert s['peak'] == 1.0 and s['mass'] == 1.0 and s['peak_index'] == 3 * w + 6
    assert np.array_equal(s['mean'], [(2 * 6 + 1) / w - 1, (2 * 3 + 1) / h - 1])
    assert np.array_equal(s['cov'], [0.0, 0.0, 0.0])


@pytest.mark.parametrize('h,w', [(7, 7), (4, 16), (64, 64)])
def test_uniform_map(h, w):
    s = stats_ref.stats_ref(np.full((h, w), 1.0 / (h * w)))
    assert abs(s['mass'] - 1) <= 1e-14 and s['peak_index'] == 0
    assert np.abs(s['mean']).max() <= 1e-15
    # the variance of w equally likely grid points of spacing 2/w: (w^2 - 1) / (3 w^2)
    want = [(w * w - 1) / (3.0 * w * w), (h * h - 1) / (3.0 * h * h), 0.0]
    assert np.abs(s['cov'] - want).max() <= 1e-14


def test_two_pixels_give_the_sign_of_vxy():
    h = w = 8
    for (y0, x0, y1, x1), sign in [((1, 1, 6, 6), 1), ((1, 6, 6, 1), -1)]:
        p = np.zeros((h, w))
        p[y0, x0] = p[y1, x1] = 0.5
        s = stats_ref.stats_ref(p)
        # two points 10/8 apart on each axis, half the mass each: every central moment is (5/8)^2
        assert np.abs(s['cov'] - [25 / 64, 25 / 64, sign * 25 / 64]).max() <= 1e-15
        assert np.abs(s['mean']).max() <= 1e-15


def test_ties_return_the_first_index():
    p = np.zeros((3, 6, 6))
    p[0, 2, 3] = p[0, 4, 1] = 0.4
    p[1, 5, 5] = p[1, 0, 2] = p[1, 0, 4] = 0.3
    s = stats_ref.stats_ref(p)                        # p[2] is constant: index 0
    assert s['peak_index'].tolist() == [2 * 6 + 3, 2, 0] and s['peak'].tolist() == [0.4, 0.3, 0.0]


def test_cov_image_is_the_covariance_of_the_back_projected_points():
    """img = t + c . M on row vectors, so the weighted sample covariance of the back-projected grid points of a map is
    M^T S M: a closed form, to 1e-12 of the matrix' largest entry (fp64 rounding of ~1e3 terms of that size is ~1e-13;
    an entry that cancels to near zero has no relative bound of its own)."""
    r = np.random.default_rng(0)
    h, w = 12, 9
    p = r.random((4, h, w)) ** 6
    p /= p.sum((-2, -1), keepdims=True)
    th = 0.7
    rot = np.array([[np.cos(th), np.sin(th)], [-np.sin(th), np.cos(th)]])
    M = np.diag([180.0, 55.0]) @ rot                  # anisotropic and rotated: not symmetric
    t = np.array([310.0, -40.0])
    s = stats_ref.stats_ref(p, M)
    X, Y = stats_ref.grid(h, w)
    pts = np.stack([X, Y], -1).reshape(-1, 2) @ M + t                       # [h w, 2]
    for k in range(4):
        wgt = p[k].reshape(-1)
        mu = wgt @ pts
        d = pts - mu
        want = (d * wgt[:, None]).T @ d
        assert np.abs(s['cov_image'][k] - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(s['mean'][k] @ M + t - mu).max() <= 1e-12 * np.abs(mu).max()
    assert abs(s['cov_image'][0][0, 1] - s['cov_image'][0][1, 0]) <= 1e-12 * np.abs(s['cov_image'][0]).max()


# ------------------------------------------------------------------ the C ABI without a GPU
def test_new_symbols_exported_declared_and_bound():
    from dsnt import _lib
    lib = _lib.load()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dsnt_hip.h')).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name
        assert name in _lib.SIGNATURES
    assert lib.dsnt_version() >= 120


FAKE = C.c_void_p(1 << 20)      # never dereferenced: every case below is refused before a launch
HFLIP = [5, 4, 3, 2, 1, 0, 6, 7, 8, 9, 15, 14, 13, 12, 11, 10]


def _standalone(**kw):
    from dsnt import _lib
    lib = _lib.load()
    a = dict(hm=FAKE, rows=4, h=8, w=8, stats=FAKE, index=FAKE)
    a.update(kw)
    rc = lib.dsnt_heatmap_stats(a['hm'], a['rows'], a['h'], a['w'], a['stats'], a['index'], None)
    return rc, lib.dsnt_last_error().decode()


def _fused(**kw):
    from dsnt import _lib
    lib = _lib.load()
    a = dict(logits=FAKE, B=2, J=16, h=8, w=8, perm=(C.c_int * 16)(*HFLIP), strategy=0, preact=0, thr=0.0, eps=0.0,
             tm=FAKE, tb=FAKE, hm=None, coords=FAKE, img=FAKE, stats=FAKE, index=FAKE, cov_image=FAKE)
    a.update(kw)
    rc = lib.dsnt_flip_merge_head_stats(a['logits'], a['B'], a['J'], a['h'], a['w'], a['perm'], a['strategy'],
                                        a['preact'], a['thr'], a['eps'], a['tm'], a['tb'], a['hm'], a['coords'], a['img'],
                                        a['stats'], a['index'], a['cov_image'], None)
    return rc, lib.dsnt_last_error().decode()


@pytest.mark.parametrize('name', ['hm', 'stats', 'index'])
def test_heatmap_stats_refuses_null_pointers(name):
    rc, msg = _standalone(**{name: None})
    assert rc == 3 and 'null' in msg and 'dsnt_heatmap_stats' in msg


@pytest.mark.parametrize('kw', [dict(rows=0), dict(rows=-2), dict(rows=1 << 31), dict(h=0), dict(w=-1),
                                dict(h=4096, w=4096)])
def test_heatmap_stats_refuses_bad_shapes(kw):
    rc, msg = _standalone(**kw)
    assert rc == 1 and 'dsnt_heatmap_stats' in msg


@pytest.mark.parametrize('name', ['logits', 'perm', 'tm', 'tb', 'coords', 'img', 'stats', 'index', 'cov_image'])
def test_flip_merge_head_stats_refuses_null_pointers(name):
    rc, msg = _fused(**{name: None})
    assert rc == 3 and 'null' in msg and 'dsnt_flip_merge_head_stats' in msg


@pytest.mark.parametrize('kw,code', [(dict(h=0), 1), (dict(h=4096, w=4096), 1), (dict(B=0), 1), (dict(J=33), 1),
                                     (dict(strategy=2), 3), (dict(preact=5), 3),
                                     (dict(perm=(C.c_int * 16)(*([0] * 16))), 3)])
def test_flip_merge_head_stats_refuses_bad_arguments(kw, code):
    rc, msg = _fused(**kw)
    assert rc == code and 'dsnt_flip_merge_head_stats' in msg


# ------------------------------------------------------------------ the Python surface on CPU tensors
def test_python_surface_refuses_cpu_tensors():
    import torch
    import dsnt.nn as dn
    from dsnt import inference
    from dsnt.model import build_mpii_pose_model
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dn.heatmap_stats(torch.zeros(1, 2, 4, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        inference.flip_merge_head(torch.zeros(2, 16, 4, 4), torch.zeros(1, 2, 2, dtype=torch.float64),
                                  torch.zeros(1, 1, 2, dtype=torch.float64), stats=True)
    m = build_mpii_pose_model(base='hg1', output_strat='dsnt')
    tm, tb = torch.eye(2, dtype=torch.float64)[None], torch.zeros(1, 1, 2, dtype=torch.float64)
    for flip in (True, False):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            inference.predict(m, torch.zeros(1, 3, 64, 64), tm, tb, use_flipped=flip, return_stats=True)
