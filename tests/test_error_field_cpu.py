"""The misprediction field without a GPU: the numpy restatement of `dsnt_error_field` (tests/error_field_ref.py) against
`scipy.stats.binned_statistic_dd` used as reference `bin/investigate.py:86-99` uses it, every reading method of
`dsnt.evaluator.ErrorField` on a hand-written state loaded through `load_state_dict`, and the entry's host-side refusals.

The hand-written state (bins = 2, 16 joints; cells [by, bx]; planes total / miss / miss_finite, then sum_x / sum_y):

    rankle   total [[4, 0], [2, 6]]   miss [[2, 0], [2, 3]]   finite [[2, 0], [0, 3]]   sx [[1, 0], [0, -1.5]]  sy [[0.5, 0], [0, 3]]
    rwrist   total [[1, 0], [0, 2]]   miss [[0, 0], [0, 2]]   finite [[0, 0], [0, 1]]   sx [[0, 0], [0, 0.25]]  sy [[0, 0], [0, -1]]
    every other joint 0.

Cell [1, 0] of rankle: two joints, both missed, neither with a finite offset: rate 1, mean NaN.  Cell [0, 1]: nothing
there at all: rate 0, mean NaN.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import error_field_ref as ref

NAN = float('nan')


def _state():
    counts = torch.zeros(3, 16, 2, 2, dtype=torch.int64)
    sums = torch.zeros(2, 16, 2, 2, dtype=torch.float64)
    counts[:, 0] = torch.tensor([[[4, 0], [2, 6]], [[2, 0], [2, 3]], [[2, 0], [0, 3]]])
    counts[:, 10] = torch.tensor([[[1, 0], [0, 2]], [[0, 0], [0, 2]], [[0, 0], [0, 1]]])
    sums[:, 0] = torch.tensor([[[1, 0], [0, -1.5]], [[0.5, 0], [0, 3]]])
    sums[:, 10] = torch.tensor([[[0, 0], [0, 0.25]], [[0, 0], [0, -1]]])
    return {'bins': 2, 'threshold': 0.5, 'counts': counts, 'sums': sums}


def _loaded():
    from dsnt.evaluator import ErrorField
    ev = ErrorField(bins=2)
    ev.load_state_dict(_state())
    return ev


def _same(a, b):
    return a.shape == np.shape(b) and np.array_equal(a, np.asarray(b, dtype=a.dtype), equal_nan=True)


# ---------------------------------------------------------------------------------- restatement vs scipy
def _planted(bins, J=2):
    """Targets on every edge and one fp32 ulp to either side of it (so also just outside -1 and 1), along x with y drawn,
    along y with x drawn and both at once, and 64 drawn ones; all valid, predictions a noisy copy, about a third missed."""
    r = np.random.default_rng(bins)
    e32 = ref.edges_of(bins).astype(np.float32)
    near = np.concatenate([e32, np.nextafter(e32, np.float32(-2)), np.nextafter(e32, np.float32(2))])
    rows = []
    for v in near:
        rows += [(v, np.float32(r.uniform(-1, 1))), (np.float32(r.uniform(-1, 1)), v), (v, v), (v, -v)]
    rows += [tuple(v) for v in r.uniform(-1.1, 1.1, (64, 2)).astype(np.float32)]
    target = np.array(rows, np.float32)[:, None, :].repeat(J, 1)
    target[:, 1] = target[::-1, 1]                     # the second joint sees them in another order
    B = len(rows)
    pred = (target + r.normal(0, 0.2, (B, J, 2))).astype(np.float32)
    m = np.array([[150.0, 90.0], [-20.0, 60.0]]) + r.uniform(-10, 10, (B, 2, 2))
    return pred, target, m, r.uniform(0, 400, (B, 2)), np.ones((B, J), np.float32), r.uniform(40, 120, B)


@pytest.mark.parametrize('bins', [1, 5, 7, 8, 32])
def test_restatement_matches_scipy(bins):
    """investigate.py:73-99 per joint: the joints with |t| <= 1 go to `binned_statistic_dd(bins=, range=[[-1, 1]] * 2)`,
    transposed to [y, x].  Counts are equal and the means equal to the last bit: scipy sums a cell in sample order too."""
    from dsnt.evaluator import ErrorField
    binned = pytest.importorskip('scipy.stats').binned_statistic_dd
    args = _planted(bins)
    pred, target, m, b, mask, head = args
    edges = ref.edges_of(bins)
    total, miss, finite, sx, sy = ref.restate(*args, 0.5, edges)
    assert np.array_equal(miss, finite)                # finite predictions only: scipy takes nothing else
    d = ref.distance(pred, target, m, b, head)
    rng = [[-1, 1], [-1, 1]]
    outside = 0
    for j in range(pred.shape[1]):
        t, p = target[:, j].astype(np.float64), pred[:, j].astype(np.float64)
        keep = (np.abs(t[:, 0]) <= 1) & (np.abs(t[:, 1]) <= 1)
        outside += (~keep).sum()
        missed = keep & (d[:, j] > 0.5)
        assert 10 <= missed.sum() <= keep.sum() - 10
        want_total = binned(t[keep], None, statistic='count', bins=bins, range=rng).statistic.T
        want_miss = binned(t[missed], None, statistic='count', bins=bins, range=rng).statistic.T
        mean_x = binned(t[missed], p[missed, 0] - t[missed, 0], statistic='mean', bins=bins, range=rng)
        mean_y = binned(t[missed], p[missed, 1] - t[missed, 1], statistic='mean', bins=bins, range=rng)
        assert np.array_equal(mean_x.bin_edges[0], edges) and np.array_equal(mean_x.bin_edges[1], edges)
        assert np.array_equal(total[j], want_total) and np.array_equal(miss[j], want_miss), (bins, j)
        with np.errstate(invalid='ignore'):
            assert np.array_equal(sx[j] / finite[j], mean_x.statistic.T, equal_nan=True), (bins, j)
            assert np.array_equal(sy[j] / finite[j], mean_y.statistic.T, equal_nan=True), (bins, j)
        # and through the class: the same field, the same quiver arrays
        ev = ErrorField(bins=bins, n_joints=pred.shape[1])
        ev.load_state_dict({'bins': bins, 'threshold': 0.5, 'counts': torch.from_numpy(np.stack([total, miss, finite])),
                            'sums': torch.from_numpy(np.stack([sx, sy]))})
        assert np.array_equal(ev.mean_offset(j), np.stack([mean_x.statistic.T, mean_y.statistic.T], -1), equal_nan=True)
        with np.errstate(divide='ignore', invalid='ignore'):
            assert np.array_equal(ev.miss_rate(j), np.nan_to_num(want_miss / want_total))
    assert outside >= 8                                # the targets one ulp outside the frame were there, and left out


def test_cell_of_on_the_edges():
    e = ref.edges_of(8)
    assert [ref.cell_of(t, e) for t in (-1.0, -0.75, np.nextafter(-0.75, -1), 0.0, 0.75, np.nextafter(1.0, 0), 1.0)] \
        == [0, 1, 0, 4, 7, 7, 7]
    assert ref.cell_of(0.3, ref.edges_of(1)) == 0 and ref.cell_of(1.0, ref.edges_of(1)) == 0


# ---------------------------------------------------------------------------------- the class on a hand-written state
def test_defaults_and_constructor_refusals():
    from dsnt.evaluator import ErrorField, PCKhEvaluator
    ev = ErrorField()
    assert ev.bins == 8 and ev.threshold == 0.5 and ev.n_joints == 16
    assert ev.joint_names == PCKhEvaluator.JOINT_NAMES and set(ev.groups) == set(PCKhEvaluator.JOINT_GROUPS)
    assert np.array_equal(ev.edges, np.linspace(-1, 1, 9)) and ev.edges.dtype == np.float64
    assert np.array_equal(ev.centres, np.arange(-7, 8, 2) / 8)
    assert ev.totals().shape == (8, 8) and ev.totals().dtype == np.int64 and not ev.totals().any()
    assert not ev.miss_rate().any() and np.isnan(ev.mean_offset()).all() and ev.mean_offset().shape == (8, 8, 2)
    assert not hasattr(ev, 'add')                      # image-space coordinates carry no cell
    for bad in (dict(bins=0), dict(bins=33), dict(bins=-1), dict(n_joints=0), dict(n_joints=-3),
                dict(n_joints=3, joint_names=['a', 'b'])):
        with pytest.raises(ValueError):
            ErrorField(**bad)
    assert ErrorField(bins=1).centres.tolist() == [0.0] and ErrorField(bins=32).edges.shape == (33,)
    assert list(ErrorField(n_joints=7).groups) == ['all'] and ErrorField(n_joints=7).joint_names == []


def test_reading_a_hand_written_state():
    ev = _loaded()
    assert _same(ev.totals('rankle'), [[4, 0], [2, 6]]) and ev.totals('rankle').dtype == np.int64
    assert _same(ev.misses('rankle'), [[2, 0], [2, 3]]) and ev.misses('rankle').dtype == np.int64
    assert _same(ev.miss_rate('rankle'), [[0.5, 0.0], [1.0, 0.5]]) and ev.miss_rate('rankle').dtype == np.float64
    # the mean is over the misses with a finite offset: [1, 0] has misses and none of them finite
    assert _same(ev.mean_offset('rankle'), [[[0.5, 0.25], [NAN, NAN]], [[NAN, NAN], [-0.5, 1.0]]])
    assert _same(ev.mean_offset('rwrist'), [[[NAN, NAN], [NAN, NAN]], [[NAN, NAN], [0.25, -1.0]]])
    assert _same(ev.miss_rate('rwrist'), [[0.0, 0.0], [0.0, 1.0]])
    # a joint index reads the same planes as its name; a joint nobody saw: zeros, rate 0, mean NaN
    assert _same(ev.totals(0), ev.totals('rankle')) and _same(ev.mean_offset(np.int64(10)), ev.mean_offset('rwrist'))
    assert not ev.totals('lknee').any() and not ev.miss_rate('lknee').any() and np.isnan(ev.mean_offset('lknee')).all()
    # groups: ubody holds rwrist alone; the others rankle and rwrist; the default is 'all'
    assert _same(ev.totals('ubody'), ev.totals('rwrist')) and _same(ev.mean_offset('ubody'), ev.mean_offset('rwrist'))
    for g in ('total_anewell', 'total_mpii', 'all'):
        assert _same(ev.totals(g), [[5, 0], [2, 8]]) and _same(ev.misses(g), [[2, 0], [2, 5]])
        assert _same(ev.miss_rate(g), [[0.4, 0.0], [1.0, 0.625]])
        assert _same(ev.mean_offset(g), [[[0.5, 0.25], [NAN, NAN]], [[NAN, NAN], [-1.25 / 4, 0.5]]])
    assert _same(ev.totals(), ev.totals('all')) and _same(ev.mean_offset(), ev.mean_offset('all'))
    for bad in ('nose', 16, -1, True):
        with pytest.raises(KeyError):
            ev.totals(bad)
    counts, sums = ev.tables()
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (3, 16, 2, 2) and tuple(sums.shape) == (2, 16, 2, 2)


def test_quiver():
    """investigate.py:112-121: centres on a meshgrid (x along the columns), everything flattened in the order of
    `argsort(C.flatten())`.  Rates of 'all': [[0.4, 0], [1, 0.625]], so the order of the cells is [0,1] [0,0] [1,1] [1,0]."""
    ev = _loaded()
    X, Y, U, V, Cc = ev.quiver()
    assert all(a.shape == (4,) and a.dtype == np.float64 for a in (X, Y, U, V, Cc))
    assert Cc.tolist() == [0.0, 0.4, 0.625, 1.0]
    assert X.tolist() == [0.5, -0.5, 0.5, -0.5] and Y.tolist() == [-0.5, -0.5, 0.5, 0.5]
    assert _same(U, [NAN, 0.5, -1.25 / 4, NAN]) and _same(V, [NAN, 0.25, 0.5, NAN])
    # restated as the reference writes it
    C2, field = ev.miss_rate('rankle'), ev.mean_offset('rankle')
    gx, gy = np.meshgrid(ev.centres, ev.centres)
    at = np.unravel_index(np.argsort(C2.flatten()), C2.shape)
    got = ev.quiver('rankle')
    for a, b in zip(got, (gx[at], gy[at], field[..., 0][at], field[..., 1][at], C2[at])):
        assert _same(a, b)
    from dsnt.evaluator import ErrorField
    assert all(a.shape == (64,) for a in ErrorField().quiver())


def test_merge_state_and_reset():
    from dsnt.evaluator import ErrorField
    a, b = _loaded(), _loaded()
    a.merge(b)
    assert _same(a.totals(), [[10, 0], [4, 16]]) and _same(b.totals(), [[5, 0], [2, 8]])
    assert _same(a.mean_offset(), b.mean_offset()) and _same(a.miss_rate(), b.miss_rate())
    c = ErrorField(bins=2)
    c.merge(a)
    assert torch.equal(c.tables()[0], 2 * _state()['counts']) and torch.equal(c.tables()[1], 2 * _state()['sums'])
    for other in (ErrorField(), ErrorField(bins=2, threshold=0.2), ErrorField(bins=2, n_joints=15)):
        with pytest.raises(ValueError):
            a.merge(other)
    # the round trip, into an object that never saw a batch; the state is a copy
    state = a.state_dict()
    assert set(state) == {'bins', 'threshold', 'counts', 'sums'} and state['bins'] == 2 and state['threshold'] == 0.5
    assert state['counts'].dtype == torch.int64 and state['sums'].dtype == torch.float64
    d = ErrorField(bins=2)
    d.load_state_dict(state)
    assert all(torch.equal(x, y) for x, y in zip(d.tables(), a.tables()))
    for name in ('all', 'ubody', 'rankle', 10):
        assert _same(d.mean_offset(name), a.mean_offset(name)) and _same(d.misses(name), a.misses(name))
    state['counts'][0, 0, 0, 0] += 100
    state['sums'][0, 0, 0, 0] += 100
    assert _same(a.totals(), [[10, 0], [4, 16]]) and a.tables()[1][0, 0, 0, 0] == 2.0
    d.load_state_dict(_state())                        # loading replaces, it does not add
    assert _same(d.totals(), [[5, 0], [2, 8]])
    for bad in (dict(_state(), bins=3), dict(_state(), threshold=0.2), dict(_state(), counts=_state()['counts'][:2]),
                dict(_state(), sums=_state()['sums'][:, :15])):
        with pytest.raises(ValueError):
            a.load_state_dict(bad)
    with pytest.raises(ValueError):
        ErrorField(bins=2, n_joints=7).load_state_dict(_state())
    a.reset()
    assert not a.tables()[0].any() and not a.tables()[1].any() and a.bins == 2
    a.all_reduce()                                     # no process group: nothing to do
    assert not a.totals().any()


def test_unnamed_joints_and_custom_groups():
    from dsnt.evaluator import ErrorField
    counts = torch.zeros(3, 3, 1, 1, dtype=torch.int64)
    counts[:, 0, 0, 0] = torch.tensor([4, 2, 1])
    counts[:, 2, 0, 0] = torch.tensor([4, 4, 3])
    sums = torch.tensor([[1.0, 0.0, 2.0], [0.0, 0.0, -4.0]]).double().reshape(2, 3, 1, 1)
    state = {'bins': 1, 'threshold': 0.5, 'counts': counts, 'sums': sums}
    ev = ErrorField(bins=1, n_joints=3)
    ev.load_state_dict(state)
    assert ev.totals().tolist() == [[8]] and ev.miss_rate().tolist() == [[0.75]] and ev.mean_offset().tolist() == [[[0.75, -1.0]]]
    assert ev.miss_rate(1).tolist() == [[0.0]] and ev.mean_offset(0).tolist() == [[[1.0, 0.0]]]
    for bad in ('total_mpii', 3, 'rankle'):
        with pytest.raises(KeyError):
            ev.totals(bad)
    named = ErrorField(bins=1, n_joints=3, joint_names=['a', 'b', 'c'], joint_groups={'ends': {'a', 'c'}, 'mid': {'b'}})
    named.load_state_dict(state)
    assert named.totals('ends').tolist() == [[8]] and named.totals('mid').tolist() == [[0]] and named.misses('c').tolist() == [[4]]
    assert set(named.groups) == {'ends', 'mid', 'all'}


# ---------------------------------------------------------------------------------- the entry's refusals, on the host
def test_entry_point_refuses_bad_arguments_without_gpu():
    """The argument checks of `dsnt_error_field` run before anything is launched: no device is needed to see them."""
    from dsnt import _lib
    fn = _lib.fn('dsnt_error_field')
    assert _lib.load().dsnt_version() >= 124
    p = C.c_void_p(4096)                               # never dereferenced: every call below is refused

    def rc(edges, bins=None, B=4, J=3, ptrs=(p,) * 6, counts=p, sums=p):
        arr = (C.c_double * max(len(edges), 1))(*edges)
        return fn(*ptrs, 0.5, arr, len(edges) - 1 if bins is None else bins, counts, sums, B, J, None)
    nan, inf = NAN, float('inf')
    for edges, bins, what in (([-1, 1], 0, b'bins=0 outside 1..32'), (list(np.linspace(-1, 1, 34)), None, b'bins=33 outside 1..32'),
                              ([-1, 1], -1, b'bins=-1 outside 1..32'), ([1, -1], None, b'strictly ascending (index 1)'),
                              ([-1, 0, 0], None, b'strictly ascending (index 2)'), ([-1, nan, 1], None, b'edge 1 is not finite'),
                              ([-inf, 1], None, b'edge 0 is not finite'), ([-1, inf], None, b'edge 1 is not finite')):
        assert rc(edges, bins) == 3, edges
        err = _lib.fn('dsnt_last_error')()
        assert err.startswith(b'dsnt_error_field: ') and what in err, (edges, err)
    ok = [-1, 0, 1]
    for k in range(6):
        assert rc(ok, ptrs=(p,) * k + (None,) + (p,) * (5 - k)) == 3
    assert rc(ok, counts=None) == 3 and rc(ok, sums=None) == 3 and rc(ok, B=0) == 3 and rc(ok, J=0) == 3 and rc(ok, B=-1) == 3
    assert fn(p, p, p, p, p, p, 0.5, None, 2, p, p, 4, 3, None) == 3
    assert _lib.fn('dsnt_last_error')() == b'dsnt_error_field: bad argument'
