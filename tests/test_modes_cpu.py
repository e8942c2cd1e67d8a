"""The mode-seeking read-out without a GPU: known answers of the numpy restatement (tests/modes_ref.py), the restatement
against an exact evaluation of the windows it chose on the seeded inputs of tests/test_modes_gpu.py, every refusal of
`dsnt_map_modes` with its exact text, the ctypes row, and the argument errors of `nn.heatmap_modes` and `predict`.

The bounds of the exact comparison are derived, not measured (n <= 289 the number of pixels of the window):
  * mass: the window sum is n - 1 fp64 adds of partial sums no larger than sum |p|, each off by at most 2^-53 of its result,
    then one rounding to fp32: one fp32 ulp plus n 2^-53 sum |p|;
  * coords: |X| < 1, so sum X p carries the same bound as the mass plus n roundings of the products, and the quotient of
    two sums that are each right to n 2^-52 relative is right to a few n 2^-52 < 2^-42 for a window of non-negative
    pixels (|c| <= 1); then one rounding to fp32: one fp32 ulp plus 2^-40."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import modes_ref as ref


def _px(c, size):
    """normalised coordinate -> pixel"""
    return ((c + 1.0) * size - 1.0) / 2.0


# ------------------------------------------------------------------ known answers
def test_bimodal_map_of_the_prototype():
    p = ref.bimodal()[None]
    X = (2 * np.arange(64) + 1) / 64.0 - 1.0
    mean_x = float((p[0].astype(np.float64).sum(0) * X).sum())
    assert abs(_px(mean_x, 64) - 30.02) < 0.01            # about 10 px from either bump
    out = ref.modes(p, 3, 2)
    assert out['index'].tolist() == [[31 * 64 + 20, 31 * 64 + 45]]
    got = [(_px(float(out['coords'][0, k, 0]), 64), _px(float(out['coords'][0, k, 1]), 64), float(out['mass'][0, k]))
           for k in range(2)]
    for (x, y, m), (wx, wy, wm) in zip(got, [(20.299, 30.701, 0.5994), (44.602, 31.199, 0.3996)]):
        assert abs(x - wx) < 1e-3 and abs(y - wy) < 1e-3 and abs(m - wm) < 1e-4, got


def test_one_hot_map_takes_the_top_left_window_and_keeps_the_pixel():
    p = np.zeros((1, 8, 8), np.float32)
    p[0, 5, 5] = 1.0
    out = ref.modes(p, 2, 2)
    assert out['index'].tolist() == [[3 * 8 + 3, -1]]      # every centre lies within 2r = 4 of (3, 3): no mode 1
    assert out['coords'][0, 0].tolist() == [11 / 8 - 1, 11 / 8 - 1] and out['mass'][0, 0] == 1.0
    assert np.isnan(out['mass'][0, 1]) and np.isnan(out['coords'][0, 1]).all()
    # a corner: the tie set is clipped, and centres further than 2r exist: an empty second mode, not a missing one
    p = np.zeros((1, 8, 8), np.float32)
    p[0, 0, 7] = 0.5
    out = ref.modes(p, 2, 2)
    assert out['index'].tolist() == [[5, 0]] and out['mass'].tolist() == [[0.5, 0.0]]
    assert out['coords'][0, 0].tolist() == [15 / 8 - 1, 1 / 8 - 1] and np.isnan(out['coords'][0, 1]).all()


def test_zero_nan_and_negative_maps():
    z = ref.modes(np.zeros((1, 6, 6), np.float32), 1, 2)
    assert z['index'].tolist() == [[0, 3]] and z['mass'].tolist() == [[0.0, 0.0]] and np.isnan(z['coords']).all()
    n = ref.modes(np.full((1, 6, 6), np.nan, np.float32), 1, 4)
    assert (n['index'] == -1).all() and np.isnan(n['mass']).all() and np.isnan(n['coords']).all()
    # one NaN pixel: no window that holds it is ever chosen, though the largest pixel sits beside it
    p = np.full((1, 9, 9), 0.01, np.float32)
    p[0, 4, 4], p[0, 4, 5] = np.nan, 1.0
    out = ref.modes(p, 1, 1)
    y, x = divmod(int(out['index'][0, 0]), 9)
    assert x == 6 and y in (3, 4, 5) and abs(float(out['mass'][0, 0]) - 1.08) < 1e-6
    # all negative: the least negative window wins, its mass is reported and it has no centroid
    p = -np.ones((1, 5, 5), np.float32)
    out = ref.modes(p, 1, 1)
    assert out['index'].tolist() == [[0]] and out['mass'].tolist() == [[-4.0]] and np.isnan(out['coords']).all()
    # -inf everywhere: S > -inf never holds
    assert ref.modes(np.full((1, 4, 4), -np.inf, np.float32), 0, 1)['index'].tolist() == [[-1]]


def test_radius_zero_is_the_arg_max_and_a_covering_radius_the_global_mean():
    p = ref.seeded_maps(7, 7)[:24]
    out = ref.modes(p, 0, 1)
    assert out['index'][:, 0].tolist() == p.reshape(24, -1).argmax(1).tolist()
    assert np.array_equal(out['mass'][:, 0], p.reshape(24, -1).max(1))
    out = ref.modes(p, 8, 2)
    assert (out['index'] == [0, -1]).all()                 # every window is the whole map: all tie, the first centre wins
    X = (2 * np.arange(7) + 1) / 7.0 - 1.0
    P = p.astype(np.float64)
    mean = np.stack([(P.sum(1) * X).sum(1), (P.sum(2) * X).sum(1)], -1) / P.sum((1, 2))[:, None]
    assert np.abs(out['coords'][:, 0] - mean).max() < 1e-6
    assert np.abs(out['mass'][:, 0] - P.sum((1, 2))).max() < 1e-6


def test_scores_add_in_the_documented_order():
    """Against a scalar loop on a map whose sums round: the order of the adds is part of the definition."""
    rng = np.random.RandomState(0)
    p = (rng.standard_normal((1, 6, 7)) * 10 ** rng.uniform(-3, 3, (1, 6, 7))).astype(np.float32)
    for r in (1, 2, 8):
        s = np.zeros((6, 7), np.float32)
        S = np.zeros((6, 7), np.float32)
        for y in range(6):
            for x in range(7):
                acc = np.float32(0)
                for d in range(-r, r + 1):
                    acc = np.float32(acc + (p[0, y, x + d] if 0 <= x + d < 7 else np.float32(0)))
                s[y, x] = acc
        for y in range(6):
            for x in range(7):
                acc = np.float32(0)
                for d in range(-r, r + 1):
                    acc = np.float32(acc + (s[y + d, x] if 0 <= y + d < 6 else np.float32(0)))
                S[y, x] = acc
        assert np.array_equal(ref.scores(p, r)[0], S)


# ------------------------------------------------------------------ the restatement against an exact evaluation
@pytest.mark.parametrize('h,w', ref.SHAPES)
def test_restatement_against_exact_window_sums(h, w):
    p = ref.seeded_maps(h, w)
    worst = [0.0, 0.0]
    for r in ref.RADII:
        out = ref.seeded_modes(h, w, r)
        for row in range(ref.N_ROWS):
            for k in range(4):
                idx = int(out['index'][row, k])
                mass, c = float(out['mass'][row, k]), out['coords'][row, k].astype(np.float64)
                if idx < 0:
                    assert math.isnan(mass) and np.isnan(c).all()
                    continue
                m, cx, cy, sabs, n = ref.exact(p[row], idx, r)
                assert not math.isnan(m)                   # a window with a NaN is never chosen
                bar = float(np.spacing(np.float32(abs(m)))) + n * 2.0 ** -53 * sabs
                assert abs(mass - m) <= bar, (r, row, k, mass, m, bar)
                worst[0] = max(worst[0], abs(mass - m) / bar)
                if not m > 0:
                    assert np.isnan(c).all(), (r, row, k)
                    continue
                for got, want in ((c[0], cx), (c[1], cy)):
                    bar = float(np.spacing(np.float32(abs(want)))) + 2.0 ** -40
                    assert abs(got - want) <= bar, (r, row, k, got, want, bar)
                    worst[1] = max(worst[1], abs(got - want) / bar)
    print('%dx%d: worst mass err / bar %.3f, coords %.3f' % (h, w, worst[0], worst[1]))


def test_fewer_modes_are_a_prefix():
    p = ref.seeded_maps(16, 16)
    four = ref.seeded_modes(16, 16, 1)
    two = ref.modes(p, 1, 2, 16, *ref.seeded_transforms())
    for k, v in two.items():
        assert np.array_equal(v, four[k][:, :2], equal_nan=True), k


# ------------------------------------------------------------------ the C ABI
def test_map_modes_refusals_without_gpu():
    """Return code and exact text of everything dsnt_map_modes refuses, in its order; nothing here reaches a device."""
    from dsnt import _lib
    lib = _lib.load()
    X, N = C.c_void_p(4096), None

    def call(hm=X, rows=32, J=16, h=64, w=64, r=3, K=2, tm=N, tb=N, coords=X, mass=X, index=X, image=N):
        rc = lib.dsnt_map_modes(hm, rows, J, h, w, r, K, tm, tb, coords, mass, index, image, None)
        return rc, lib.dsnt_last_error().decode()

    ARG, SHAPE = 3, 1
    for kw in ({'hm': N}, {'coords': N}, {'mass': N}, {'index': N}, {'hm': N, 'rows': 0, 'r': 9, 'h': 0}):
        assert call(**kw) == (ARG, 'dsnt_map_modes: null pointer'), kw
    for rows, J in ((0, 16), (-16, 16), (1 << 31, 16), (32, 0), (32, -1), (33, 16)):
        assert call(rows=rows, J=J, r=9) == \
            (ARG, 'dsnt_map_modes: rows=%d must be a positive multiple of J=%d below 2^31' % (rows, J))
    for r in (-1, 9):
        assert call(r=r, K=0) == (ARG, 'dsnt_map_modes: radius=%d outside 0..8' % r)
    for K in (0, 5):
        assert call(K=K, tm=X) == (ARG, 'dsnt_map_modes: K=%d outside 1..4' % K)
    for kw in ({'tm': X}, {'tb': X}, {'image': X}, {'tm': X, 'tb': X}, {'tm': X, 'image': X}, {'tb': X, 'image': X}):
        assert call(h=0, **kw) == \
            (ARG, 'dsnt_map_modes: transform_m, transform_b and image must be all null or all non-null'), kw
    for h, w in ((0, 64), (64, 0), (-1, -1), (64, 129), (8193, 1), (1 << 16, 1 << 16)):
        assert call(h=h, w=w) == (SHAPE, 'dsnt_map_modes: map %dx%d outside 1..8192 pixels (the row lives in LDS); '
                                  'dsnt_heatmap_stats takes larger maps' % (h, w))
    # accepted arguments are recorded by a launch list without touching a device, the limit shape and rows >= 2^16 included
    lst = lib.dsnt_list_create()
    assert lib.dsnt_list_begin(lst) == 0
    try:
        assert call(h=64, w=128, rows=1 << 20, J=16, r=8, K=4, tm=X, tb=X, image=X)[0] == 0
        assert call(h=1, w=1, rows=1, J=1, r=0, K=1)[0] == 0
        assert lib.dsnt_list_size(lst) == 2
        assert call(K=5)[0] == ARG and lib.dsnt_list_size(lst) == 2
    finally:
        lib.dsnt_list_end()
        lib.dsnt_list_destroy(lst)


def test_ctypes_row_and_version():
    from dsnt import _lib
    P, L, I = _lib.P, _lib.L, _lib.I
    assert _lib.SIGNATURES['dsnt_map_modes'] == [P, L, I, I, I, I, I, P, P, P, P, P, P, P]
    lib = _lib.load()
    assert lib.dsnt_version() >= 129
    assert lib.dsnt_map_modes.argtypes == [P, L, I, I, I, I, I, P, P, P, P, P, P, P] and lib.dsnt_map_modes.restype is I


# ------------------------------------------------------------------ Python argument errors
def test_heatmap_modes_argument_errors():
    import dsnt.nn as dn
    hm = torch.zeros(1, 2, 8, 8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dn.heatmap_modes(hm)
    with pytest.raises(RuntimeError, match=r'needs \[\.\.\., J, H, W\]'):
        dn.heatmap_modes(torch.zeros(8, 8))
    with pytest.raises(RuntimeError, match='expected float32'):
        dn.heatmap_modes(hm.double())
    with pytest.raises(ValueError, match='radius=9 outside 0..8'):
        dn.heatmap_modes(hm, radius=9)
    with pytest.raises(ValueError, match='count=5 outside 1..4'):
        dn.heatmap_modes(hm, count=5)
    with pytest.raises(ValueError, match='count=0 outside 1..4'):
        dn.heatmap_modes(hm, count=0)
    with pytest.raises(ValueError, match='transform_m and transform_b together'):
        dn.heatmap_modes(hm, transform_m=torch.eye(2, dtype=torch.float64)[None])


def test_predict_argument_errors():
    from dsnt import inference
    from dsnt.model import build_mpii_pose_model
    x, tm, tb = torch.zeros(1, 3, 64, 64), torch.eye(2, dtype=torch.float64)[None], torch.zeros(1, 1, 2, dtype=torch.float64)
    fc = build_mpii_pose_model(base='hg1', output_strat='fc')
    with pytest.raises(ValueError, match="'fc' strategy predicts from its linear layer"):
        inference.predict(fc, x, tm, tb, readout='mode')
    with pytest.raises(ValueError, match="'fc' strategy predicts from its linear layer"):
        inference.predict_boxes(fc, None, None, None, None, None, readout='mode')
    with pytest.raises(ValueError, match="'fc' strategy predicts from its linear layer"):
        inference.predict_dataset(fc, [], readout='mode')
    m = build_mpii_pose_model(base='hg1', output_strat='dsnt')
    for bad in ('median', None, 'Mode'):
        with pytest.raises(ValueError, match="readout must be 'mean' or 'mode'"):
            inference.predict(m, x, tm, tb, readout=bad)
    with pytest.raises(RuntimeError, match='no CPU fallback'):         # the keywords are accepted; the device is still needed
        inference.predict(m, x, tm, tb, readout='mode', mode_radius=2, return_modes=True)
