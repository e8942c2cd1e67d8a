"""`dsnt.evaluator.Reliability`, `ScoreCalibration` and `stat_score` without a GPU: the constructor, every reading method
on a hand-written table, pool-adjacent-violators on hand-worked cases and by its properties, combining and saving, the
refusals of `dsnt_score_hist` and `dsnt_score_lookup`, and the numpy restatement of tests/score_ref.py against a plain loop.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import score_ref
from dsnt import _lib
from dsnt.evaluator import PCKhCurve, Reliability, ScoreCalibration, stat_score

NAN, INF = float('nan'), float('inf')


def _same(a, b):
    """Equal, NaN in the same places."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


# ------------------------------------------------------------------ construction
def test_defaults_and_constructor_refusals():
    ev = Reliability(score_ref.EDGES20)
    assert (ev.n_joints, ev.S, ev.T, ev.higher_is_better) == (16, 20, 1, True)
    assert ev.joint_names == PCKhCurve.JOINT_NAMES and set(ev.groups) == set(PCKhCurve.JOINT_GROUPS)
    assert ev.thresholds.tolist() == [0.5] and np.array_equal(ev.score_edges.numpy(), score_ref.EDGES20)
    assert ev.counts().dtype == torch.int64 and tuple(ev.counts().shape) == (16, 22, 2) and not ev.counts().any()
    assert (Reliability.MAX_EDGES, Reliability.MAX_THRESHOLDS) == (64, 64)
    # held as the fp64 values of the fp32 roundings
    ev = Reliability([0.1, 0.7], thresholds=[0.1, 0.3], n_joints=3)
    assert ev.score_edges.tolist() == [float(np.float32(0.1)), float(np.float32(0.7))]
    assert ev.thresholds.tolist() == [float(np.float32(0.1)), float(np.float32(0.3))]
    assert ev.joint_names == [] and ev.groups == {'all': [0, 1, 2]}
    for bad in ([], list(range(65)), [0.1, NAN], [INF], [-INF, 0.0], [0.2, 0.1], [0.1, 0.1],
                [1.0, 1.0 + 1e-9]):                                       # the last pair is one fp32 value
        with pytest.raises(ValueError):
            Reliability(bad)
        with pytest.raises(ValueError):
            Reliability([0.5], thresholds=bad)
        if bad:
            with pytest.raises(ValueError):
                ScoreCalibration(bad, np.zeros((1, len(bad) + 2), np.float32))
    with pytest.raises(ValueError):
        Reliability([0.5], n_joints=0)
    with pytest.raises(ValueError):
        Reliability([0.5], n_joints=2, joint_names=['a'])
    with pytest.raises(ValueError):
        ScoreCalibration([0.5], np.zeros((1, 4), np.float32))             # S + 2 = 3 columns
    Reliability(np.arange(64), thresholds=np.arange(64))                  # the most of either


# ------------------------------------------------------------------ reading, on a table written by hand
EDGES3, THR2 = [0.25, 0.5, 0.75], [0.25, 0.5]
TABLE = np.array([[[1, 1, 8], [2, 2, 6], [0, 0, 0], [6, 3, 1], [1, 0, 1]],          # joint 'a'
                  [[0, 3, 7], [1, 0, 4], [2, 2, 0], [3, 0, 1], [0, 0, 0]]])         # joint 'b'


def _hand(higher=True):
    ev = Reliability([0.5], n_joints=2, joint_names=['a', 'b'], joint_groups={'both': {'a', 'b'}})
    ev.load_state_dict({'score_edges': torch.tensor(EDGES3, dtype=torch.float64),
                        'thresholds': torch.tensor(THR2, dtype=torch.float64), 'higher_is_better': higher,
                        'table': torch.from_numpy(TABLE)})
    return ev


def test_reading_a_hand_written_table():
    """TABLE[j][r] = (d <= 0.25, 0.25 < d <= 0.5, beyond) for the score rows < 0.25, [0.25, 0.5), [0.5, 0.75), >= 0.75
    and NaN.  Joint a at 0.5: hits (2, 4, 0, 9, 1) of (10, 10, 0, 10, 2), 32 valid.
      accuracy         0.2, 0.4, NaN, 0.9, 0.5
      risk_coverage    cut -inf, 0.25, 0.5, 0.75 keeps 30, 20, 10, 10 of 32 at PCKh 15/30, 13/20, 9/10, 9/10
      operating_point  0.6 -> (0.25, 20/32, 0.65); 0.9 -> the looser of the two cuts that keep 10: (0.5, 10/32, 0.9);
                       0.95 -> None
      calibration      monotone as it is; the empty row takes the row below: 0.2, 0.4, 0.4, 0.9 | unscored 0.5
    Joint a at 0.25: hits (1, 2, 0, 6, 1).
    Joint b at 0.5: 3/10, 1/5, 4/4, 3/4: two violations, pooled to 4/15, 4/15, 7/8, 7/8 | unscored NaN.
    Group both at 0.5: 5/20, 5/15, 4/4, 12/14: one violation, pooled to 1/4, 1/3, 16/18, 16/18 | unscored 1/2.
    Read as lower-is-better, joint a at 0.5:
      risk_coverage    cut 0.25, 0.5, 0.75, +inf keeps 10, 20, 20, 30 at PCKh 2/10, 6/20, 6/20, 15/30
      operating_point  0.3 -> (+inf, 30/32, 0.5)
      calibration      0.2, 0.4, 0.9 must not rise: one pool, 15/30 everywhere | unscored 0.5"""
    ev = _hand()
    assert ev.S == 3 and ev.T == 2 and np.array_equal(ev.counts().numpy(), TABLE)
    rate, n = ev.accuracy(0.5, 'a')
    assert _same(rate, np.array([0.2, 0.4, NAN, 0.9, 0.5])) and _same(n, np.array([10, 10, 0, 10, 2]))
    assert _same(ev.accuracy(0.25, 'a')[0], np.array([0.1, 0.2, NAN, 0.6, 0.5]))
    assert _same(ev.accuracy(0.5, 0)[0], rate) and _same(ev.accuracy(0.5, 'both')[1], np.array([20, 15, 4, 14, 2]))
    rc = ev.risk_coverage(0.5, 'a')
    assert sorted(rc) == ['coverage', 'cut', 'kept', 'pckh']
    assert _same(rc['cut'], np.array([-INF, 0.25, 0.5, 0.75])) and _same(rc['kept'], np.array([30, 20, 10, 10]))
    assert _same(rc['coverage'], np.array([30, 20, 10, 10]) / 32)
    assert _same(rc['pckh'], np.array([15 / 30, 13 / 20, 9 / 10, 9 / 10]))
    assert ev.operating_point(0.6, 0.5, 'a') == (0.25, 20 / 32, 0.65)
    assert ev.operating_point(0.9, 0.5, 'a') == (0.5, 10 / 32, 0.9)
    assert ev.operating_point(0.95, 0.5, 'a') is None and ev.operating_point(0.0, 0.5, 'a') == (-INF, 30 / 32, 0.5)
    cal = ev.calibration(0.5)
    assert cal.score == 'peak' and cal.values.dtype == torch.float32 and tuple(cal.values.shape) == (2, 5)
    assert np.array_equal(cal.score_edges.numpy(), EDGES3)
    want = np.array([[0.2, 0.4, 0.4, 0.9, 0.5], [4 / 15, 4 / 15, 7 / 8, 7 / 8, NAN]]).astype(np.float32)
    assert _same(cal.values.numpy(), want)
    assert _same(ev.calibration(0.5, 'b').values.numpy(), want[1:])
    named = ev.calibration(0.5, score='spread')                           # the statistic the caller says it fed
    assert named.score == 'spread' and _same(named.values.numpy(), want)
    assert _same(ev.calibration(0.5, 'both').values.numpy(),
                 np.array([[1 / 4, 1 / 3, 16 / 18, 16 / 18, 1 / 2]]).astype(np.float32))
    assert _same(ev.calibration(0.25, 'a').values.numpy(), np.array([[0.1, 0.2, 0.2, 0.6, 0.5]]).astype(np.float32))
    for call in (ev.accuracy, ev.risk_coverage, ev.calibration):
        with pytest.raises(KeyError):
            call(0.3, 'a')                                                # not a constructed threshold
        with pytest.raises(KeyError):
            call(0.5, 'total_mpii')
    with pytest.raises(KeyError):
        ev.operating_point(0.5, 0.5, 2)
    low = _hand(higher=False)
    assert not low.higher_is_better
    rc = low.risk_coverage(0.5, 'a')
    assert _same(rc['cut'], np.array([0.25, 0.5, 0.75, INF])) and _same(rc['kept'], np.array([10, 20, 20, 30]))
    assert _same(rc['coverage'], np.array([10, 20, 20, 30]) / 32)
    assert _same(rc['pckh'], np.array([2 / 10, 6 / 20, 6 / 20, 15 / 30]))
    assert low.operating_point(0.3, 0.5, 'a') == (INF, 30 / 32, 0.5)
    assert low.operating_point(0.2, 0.5, 'b') == (INF, 1.0, 11 / 23) and low.operating_point(0.6, 0.5, 'a') is None
    cal = low.calibration(0.5, 'a')
    assert cal.score == 'spread' and _same(cal.values.numpy(), np.full((1, 5), 0.5, np.float32))
    assert _same(low.accuracy(0.5, 'a')[0], rate)                         # the table reads the same either way


# ------------------------------------------------------------------ pool-adjacent-violators
def _calibrated(rows, higher=True):
    """The values of one joint whose score rows hold `rows` = (hits, n), at the one threshold of the table."""
    S = len(rows) - 1
    table = np.zeros((1, S + 2, 2), np.int64)
    for r, (h, n) in enumerate(rows):
        table[0, r] = (h, n - h)
    ev = Reliability(np.arange(max(S, 1)), n_joints=1, higher_is_better=higher)
    ev.load_state_dict({'score_edges': torch.arange(S, dtype=torch.float64), 'thresholds': torch.tensor([0.5]),
                        'higher_is_better': higher, 'table': torch.from_numpy(table)})
    return ev.calibration(0.5).values.numpy()[0, :S + 1]


def _f32(*fractions):
    return np.array([np.float32(h / n) if n else np.float32(NAN) for h, n in fractions], np.float32)


def test_pav_by_hand():
    # already monotone
    assert _same(_calibrated([(1, 4), (2, 4), (3, 4)]), _f32((1, 4), (2, 4), (3, 4)))
    # one violation: the two rows share 3 / 8
    assert _same(_calibrated([(2, 4), (1, 4), (3, 4)]), _f32((3, 8), (3, 8), (3, 4)))
    # a falling chain is one pool
    assert _same(_calibrated([(3, 4), (2, 4), (1, 4), (0, 4)]), _f32(*[(6, 16)] * 4))
    # a pool that falls below its neighbour takes it in as well: 6/10, 0/10 -> 6/20 < 5/10 -> 11/30 >= 1/10
    assert _same(_calibrated([(1, 10), (5, 10), (6, 10), (0, 10)]), _f32((1, 10), (11, 30), (11, 30), (11, 30)))
    # weighted by support: 1/1 and 0/9 pool to 1/10, not to the mean of the rates
    assert _same(_calibrated([(1, 1), (0, 9)]), _f32((1, 10), (1, 10)))
    # empty rows below, between and above: the supported row below, else the one above
    assert _same(_calibrated([(0, 0), (1, 4), (0, 0), (3, 4), (0, 0)]), _f32((1, 4), (1, 4), (1, 4), (3, 4), (3, 4)))
    # ... and a violation across an empty row still pools
    assert _same(_calibrated([(3, 4), (0, 0), (1, 4)]), _f32((4, 8), (4, 8), (4, 8)))
    # lower is better: the values must not rise with the score
    assert _same(_calibrated([(1, 4), (2, 4), (3, 4)], higher=False), _f32(*[(6, 12)] * 3))
    assert _same(_calibrated([(3, 4), (1, 4), (2, 4)], higher=False), _f32((3, 4), (3, 8), (3, 8)))
    assert _same(_calibrated([(0, 0), (3, 4), (0, 0), (1, 4)], higher=False), _f32((3, 4), (3, 4), (3, 4), (1, 4)))
    # ties: equal rates from different counts are one value, pooled or not
    assert _same(_calibrated([(2, 4), (1, 2), (3, 6)]), _f32(*[(1, 2)] * 3))
    assert _same(_calibrated([(1, 3), (2, 6), (3, 9)]), _f32(*[(1, 3)] * 3))
    assert _same(_calibrated([(1, 3), (2, 6)], higher=False), _f32(*[(1, 3)] * 2))
    # nothing at all: NaN everywhere
    assert np.isnan(_calibrated([(0, 0), (0, 0), (0, 0)])).all()
    # counts past 2^53 still compare exactly: (2^60 + 1) / 2^61 > 2^59 / 2^60 by one part in 2^61
    big = [((1 << 60) + 1, 1 << 61), (1 << 59, 1 << 60)]
    assert _same(_calibrated(big), _f32(*[((1 << 60) + 1 + (1 << 59), (1 << 61) + (1 << 60))] * 2))


@pytest.mark.parametrize('higher', [True, False])
def test_pav_properties_on_random_tables(higher):
    """Monotone in the right direction over all S + 1 rows, rows without support included, and the support-weighted mean
    of the values is hits / valid: pooling moves hits between rows and loses none.  Each value is an fp64 quotient rounded
    to fp32, a relative error of at most 2^-24 on values of at most 1, so the mean is held to 2^-23."""
    r = np.random.default_rng(11 + higher)
    for trial in range(200):
        S = int(r.integers(1, 12))
        n = r.integers(0, 40, S + 1) * (r.random(S + 1) < 0.7)
        if not n.sum():
            continue
        trend = np.linspace(0.2, 0.9, S + 1) if higher else np.linspace(0.9, 0.2, S + 1)
        h = r.binomial(n, np.clip(trend + r.normal(0, 0.15, S + 1), 0, 1))
        v = _calibrated(list(zip(h.tolist(), n.tolist())), higher).astype(np.float64)
        assert not np.isnan(v).any() and (0 <= v).all() and (v <= 1).all()
        steps = np.diff(v)
        assert (steps >= 0).all() if higher else (steps <= 0).all(), (trial, h, n, v)
        assert abs((n * v).sum() / n.sum() - h.sum() / n.sum()) <= 2.0 ** -23, (trial, h, n, v)
        # rows that did not violate keep their own rate
        own = h[n > 0] / n[n > 0]
        if ((np.diff(own) >= 0).all() if higher else (np.diff(own) <= 0).all()):
            assert np.array_equal(v[n > 0], own.astype(np.float32).astype(np.float64))


# ------------------------------------------------------------------ combining and saving
def test_merge_state_dict_and_reset():
    a, b = _hand(), _hand()
    a.merge(b)
    assert np.array_equal(a.counts().numpy(), 2 * TABLE) and np.array_equal(b.counts().numpy(), TABLE)
    assert _same(a.accuracy(0.5, 'a')[0], b.accuracy(0.5, 'a')[0]) and a.accuracy(0.5, 'a')[1].sum() == 64
    state = a.state_dict()
    assert sorted(state) == ['higher_is_better', 'score_edges', 'table', 'thresholds']
    assert state['table'].dtype == torch.int64 and state['score_edges'].tolist() == EDGES3
    c = Reliability([0.1], thresholds=[0.3], n_joints=2, higher_is_better=False)
    c.load_state_dict(state)
    assert c.higher_is_better and (c.S, c.T) == (3, 2) and torch.equal(c.counts(), a.counts())
    assert _same(c.calibration(0.5).values.numpy(), b.calibration(0.5).values.numpy())
    state['table'][0, 0, 0] += 5                                          # the state is a copy
    assert torch.equal(c.counts(), a.counts())
    for other in (Reliability(EDGES3, THR2, n_joints=3), Reliability(EDGES3, [0.5], n_joints=2),
                  Reliability([0.25, 0.5], THR2, n_joints=2)):
        with pytest.raises(ValueError):
            a.merge(other)
    with pytest.raises(ValueError):
        Reliability([0.5], n_joints=3).load_state_dict(state)             # another joint count
    a.all_reduce()                                                        # no process group: nothing to do
    assert np.array_equal(a.counts().numpy(), 2 * TABLE)
    a.reset()
    assert not a.counts().any() and a.S == 3
    rate, n = a.accuracy(0.5, 'a')
    assert np.isnan(rate).all() and not n.any() and a.operating_point(0.0, 0.5, 'a') is None
    assert np.isnan(a.calibration(0.5).values.numpy()).all()
    assert np.isnan(a.risk_coverage(0.5, 'a')['coverage']).all()


def test_score_calibration_state_and_stat_score():
    cal = ScoreCalibration(EDGES3, [[0.1, 0.2, 0.3, 0.4, NAN]], score='spread')
    assert cal.S == 3 and cal.values.dtype == torch.float32 and cal.score == 'spread'
    state = cal.state_dict()
    assert sorted(state) == ['score', 'score_edges', 'values']
    other = ScoreCalibration([0.5], np.zeros((4, 3), np.float32))
    other.load_state_dict(state)
    assert other.score == 'spread' and other.S == 3 and _same(other.values.numpy(), cal.values.numpy())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        cal(torch.zeros(2, 3))
    with pytest.raises(ValueError):
        ScoreCalibration(EDGES3, np.zeros((4, 5), np.float32))(torch.zeros(2, 3))     # 4 joints' values, 3 scores a row
    cov = torch.tensor([[[[9.0, 1.0], [1.0, 16.0]], [[NAN, 0.0], [0.0, 1.0]]]], dtype=torch.float64)
    stats = {'peak': torch.tensor([[0.25, 0.5]]), 'cov_image': cov}
    assert stat_score(stats, 'peak') is stats['peak']
    spread = stat_score(stats, 'spread')
    assert spread.dtype == torch.float32 and spread[0, 0] == 5.0 and torch.isnan(spread[0, 1])
    with pytest.raises(KeyError):
        stat_score(stats, 'mass')


# ------------------------------------------------------------------ the C ABI refuses without a device
def test_entry_points_refuse_bad_arguments_without_gpu():
    lib = _lib.load()
    assert lib.dsnt_version() >= 126
    X = C.c_void_p(4096)                                                  # non-null, never followed

    def arr(v):
        return C.cast((C.c_double * max(len(v), 1))(*v), C.c_void_p)

    def hist(edges=(0.5,), thr=(0.5,), S=None, T=None, B=4, J=3, null=None):
        ptrs = [X] * 7 + [arr(edges), arr(thr), X]                       # pred .. score, edges, thresholds, table
        if null is not None:
            ptrs[null] = None
        rc = lib.dsnt_score_hist(*ptrs[:8], len(edges) if S is None else S, ptrs[8], len(thr) if T is None else T,
                                 ptrs[9], B, J, None)
        return rc, lib.dsnt_last_error().decode()

    def look(edges=(0.5,), S=None, per_joint=1, n=5, J=3, null=None):
        ptrs = [X, arr(edges), X, X]                                      # score, edges, values, out
        if null is not None:
            ptrs[null] = None
        rc = lib.dsnt_score_lookup(ptrs[0], ptrs[1], len(edges) if S is None else S, ptrs[2], per_joint, ptrs[3], n, J,
                                   None)
        return rc, lib.dsnt_last_error().decode()
    for who, fn in (('dsnt_score_hist', hist), ('dsnt_score_lookup', look)):
        assert fn(S=0) == (3, who + ': S=0 outside 1..64') and fn(S=-1) == (3, who + ': S=-1 outside 1..64')
        assert fn(edges=list(range(65))) == (3, who + ': S=65 outside 1..64')
        assert fn(edges=[0.1, NAN]) == (3, who + ': score edge 1 is not finite')
        assert fn(edges=[INF]) == (3, who + ': score edge 0 is not finite')
        assert fn(edges=[-INF, 0.1]) == (3, who + ': score edge 0 is not finite')
        assert fn(edges=[0.2, 0.1]) == (3, who + ': score edges must be strictly ascending (index 1)')
        assert fn(edges=[0.1, 0.2, 0.2]) == (3, who + ': score edges must be strictly ascending (index 2)')
        assert fn(J=0) == (3, who + ': bad argument')
    for k in range(10):
        assert hist(null=k) == (3, 'dsnt_score_hist: bad argument'), k
    for k in range(4):
        assert look(null=k) == (3, 'dsnt_score_lookup: bad argument'), k
    assert hist(B=0) == (3, 'dsnt_score_hist: bad argument') and hist(B=-2) == (3, 'dsnt_score_hist: bad argument')
    assert hist(T=0) == (3, 'dsnt_score_hist: T=0 outside 1..64')
    assert hist(thr=list(range(65))) == (3, 'dsnt_score_hist: T=65 outside 1..64')
    assert hist(thr=[0.1, INF]) == (3, 'dsnt_score_hist: threshold 1 is not finite')
    assert hist(thr=[NAN]) == (3, 'dsnt_score_hist: threshold 0 is not finite')
    assert hist(thr=[0.2, 0.1]) == (3, 'dsnt_score_hist: thresholds must be strictly ascending (index 1)')
    assert hist(thr=[0.1, 0.1]) == (3, 'dsnt_score_hist: thresholds must be strictly ascending (index 1)')
    assert hist(J=1 << 20, edges=list(range(64)), thr=list(range(64))) == (
        3, 'dsnt_score_hist: J * (S + 2) * (T + 1) does not fit an int')
    assert look(n=0) == (3, 'dsnt_score_lookup: bad argument') and look(n=-1) == (3, 'dsnt_score_lookup: bad argument')
    assert look(per_joint=2) == (3, 'dsnt_score_lookup: bad argument')


# ------------------------------------------------------------------ the restatement itself
def test_restatement_against_a_plain_loop():
    for (B, J), thr in (((9, 5), score_ref.THR3), ((16, 16), score_ref.THR15), ((3, 1), score_ref.THR1)):
        args = list(score_ref.case(B, J, seed=B * 100 + J))
        score = args[6]
        score.reshape(-1)[:4] = (NAN, INF, -INF, score_ref.EDGES20[7])[:min(4, score.size)]
        want = score_ref.restate_loop(*args, score_ref.EDGES20, thr)
        got = score_ref.restate(*args, score_ref.EDGES20, thr)
        assert np.array_equal(got, want) and got.sum() == (args[4] == 1).sum()
        # the marginal over the score rows is the PCKh histogram
        k = score_ref.column(score_ref.distance(args[0], args[1], args[2], args[3], args[5]), thr)
        hist = np.zeros((J, len(thr) + 1), np.int64)
        np.add.at(hist, (np.broadcast_to(np.arange(J), (B, J))[args[4] == 1], k[args[4] == 1]), 1)
        assert np.array_equal(got.sum(1), hist)
    edges = np.array([0.0, 1.0])
    s = np.array([-0.0, 0.0, np.nextafter(np.float32(1), np.float32(0)), 1.0, NAN, -INF, INF, 1e-45], np.float32)
    assert score_ref.row(s, edges).tolist() == [1, 1, 1, 2, 3, 0, 2, 1]
    values = np.arange(8, dtype=np.float32).reshape(2, 4)
    pair = np.array([[0.5, 2.0], [NAN, -1.0]], np.float32)
    assert np.array_equal(score_ref.lookup(pair, edges, values, 1), np.array([[1, 6], [3, 4]], np.float32))
    assert np.array_equal(score_ref.lookup(pair, edges, values, 0), np.array([[1, 2], [3, 0]], np.float32))
