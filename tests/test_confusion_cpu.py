"""Joint confusion and heat-map mass at the target without a GPU: the known answers of the numpy restatement
(tests/confusion_ref.py), the host mathematics of `dsnt.evaluator.JointConfusion` on tables put in through
`load_state_dict`, every refusal of `dsnt_joint_confusion` and `dsnt_target_mass` with its exact text, and the margins of
the seeded inputs that tests/test_confusion_gpu.py and tests/test_target_mass_gpu.py feed the device."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import confusion_ref as ref
import score_ref
from dsnt import evaluator
from dsnt.evaluator import JointConfusion


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('name', sorted(ref.HAND))
def test_restatement_known_answers(name):
    args = ref.hand([ref.HAND[name][0]])
    table, mutual = ref.restate(*args, ref.HAND_MIRROR)
    want = ref.hand_tables(name)
    assert np.array_equal(table, want[0]) and np.array_equal(mutual, want[1]), (name, table, mutual)
    assert table.sum() == (args[4] == 1).sum()                 # one cell per counted joint


def test_restatement_edges():
    d = ref.distances(*[a for k, a in enumerate(ref.hand([ref.HAND['at_threshold'][0]])) if k != 4])
    assert d[0, 0, 0] == 0.5                                    # exactly: 5 / 10
    d = ref.distances(*[a for k, a in enumerate(ref.hand([ref.HAND['tie'][0]])) if k != 4])
    assert d[0, 0, 1] == d[0, 0, 2] == 0.5
    # one fp32 ulp less head length and the joint at the threshold is a miss that landed nowhere
    args = list(ref.hand([ref.HAND['at_threshold'][0]]))
    args[5] = np.array([np.nextafter(10.0, 0.0)])
    assert ref.restate(*args, ref.HAND_MIRROR)[0][0].tolist() == [0, 0, 0, 1]
    # the NaN target of a masked joint changes nothing
    a, b = ref.hand_tables('unannotated'), ref.hand_tables('nan_target_masked')
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # the hand-built persons as one batch: the tables add
    names = sorted(ref.HAND)
    table, mutual = ref.restate(*ref.hand([ref.HAND[n][0] for n in names]), ref.HAND_MIRROR)
    assert np.array_equal(table, sum(ref.hand_tables(n)[0] for n in names))
    assert np.array_equal(mutual, sum(ref.hand_tables(n)[1] for n in names))


def test_restated_mass_known_answers():
    """An 8 x 8 map under the identity-like transform x -> 8 x + 8 (pixel centres at 1, 3, ..., 15): the disc of radius 2.5
    round (5, 5) holds the centres (3..7 step 2)^2 less the corners at distance sqrt(8) > 2.5: five of them."""
    hm = np.arange(64, dtype=np.float32).reshape(1, 1, 8, 8)
    target = np.array([[[-0.375, -0.375]]], np.float32)                             # -> (5, 5)
    m, b = np.array([[[8.0, 0.0], [0.0, 8.0]]]), np.array([[8.0, 8.0]])
    out, pixels, margin = ref.restate_mass(hm, target, m, b, np.ones((1, 1), np.float32), np.array([5.0]), [0])
    assert pixels[0, 0].tolist() == [5, -1] and math.isnan(out[0, 0, 1])
    assert out[0, 0, 0] == hm[0, 0, 2, 2] + hm[0, 0, 1, 2] + hm[0, 0, 3, 2] + hm[0, 0, 2, 1] + hm[0, 0, 2, 3]
    assert margin > 0.1
    # two joints that mirror each other, the second not annotated
    hm2 = np.ones((1, 2, 8, 8), np.float32)
    target2 = np.array([[[-0.375, -0.375], [0.5, 0.5]]], np.float32)
    out, pixels, _ = ref.restate_mass(hm2, target2, m, b, np.array([[1, 0]], np.float32), np.array([5.0]), [1, 0])
    assert pixels[0].tolist() == [[5, -1], [-1, -1]] and out[0, 0, 0] == 5 and np.isnan(out[0, 1]).all()
    out, pixels, _ = ref.restate_mass(hm2, target2, m, b, np.array([[1, 1]], np.float32), np.array([5.0]), [1, 0])
    assert pixels[0, 0].tolist() == [5, pixels[0, 1, 0]] and pixels[0, 1].tolist() == [pixels[0, 0, 1], 5]


# ------------------------------------------------------------------ the class on the host
def _loaded(table, mutual, **kw):
    ev = JointConfusion(**kw)
    ev.load_state_dict({'threshold': ev.threshold, 'mirror': ev.mirror, 'table': torch.as_tensor(table),
                        'mutual': torch.as_tensor(mutual)})
    return ev


def _random_tables(J, mirror, seed=3):
    r = np.random.default_rng(seed)
    table = r.integers(0, 40, (J, J + 1))
    table[np.arange(J), np.arange(J)] += 200
    mutual = np.array([r.integers(0, min(table[j, mirror[j]], table[mirror[j], j]) + 1) if mirror[j] > j else 0
                       for j in range(J)])
    for j in range(J):
        if mirror[j] < j:
            mutual[j] = mutual[mirror[j]]
    return table.astype(np.int64), mutual.astype(np.int64)


def test_default_mirror_is_the_flip_permutation():
    from dsnt.inference import HFLIP_INDICES
    assert JointConfusion().mirror == HFLIP_INDICES.tolist() == ref.MPII_MIRROR
    assert JointConfusion(n_joints=5).mirror == [0, 1, 2, 3, 4]
    names = JointConfusion.JOINT_NAMES
    for j, mj in enumerate(ref.MPII_MIRROR):                   # r<name> <-> l<name>, the rest alone
        assert names[mj] == ({'r': 'l', 'l': 'r'}[names[j][0]] + names[j][1:] if mj != j else names[j])


def test_readers():
    mirror = ref.MPII_MIRROR
    table, mutual = _random_tables(16, mirror)
    ev = _loaded(table, mutual)
    assert torch.equal(ev.counts(), torch.from_numpy(table)) and torch.equal(ev.mutual(), torch.from_numpy(mutual))
    assert ev.counts().dtype == torch.int64 and np.array_equal(ev.matrix(), table)
    for name in list(range(16)) + ['rwrist', 'ubody', 'total_mpii', 'all']:
        rows = ev._rows(name)
        n = int(table[rows].sum())
        rates = ev.rates(name)
        assert ev.valid(name) == n and set(rates) == {'hit', 'mirror', 'other', 'nowhere', 'mutual'}
        assert abs(rates['hit'] + rates['mirror'] + rates['other'] + rates['nowhere'] - 1) < 1e-12
        assert rates['hit'] == ev.pckh(name) == sum(table[j, j] for j in rows) / n
        assert rates['mirror'] == sum(table[j, mirror[j]] for j in rows if mirror[j] != j) / n      # each row its own column
        assert rates['nowhere'] == table[rows, 16].sum() / n and rates['mutual'] == mutual[rows].sum() / n
        assert rates['mutual'] <= rates['mirror']
    assert ev.rates(6)['mirror'] == 0 and ev.rates('pelvis')['mutual'] == 0          # no partner
    assert ev.summary()['lwrist'] == ev.rates(15) and set(ev.summary()) == set(ev.joint_names) | set(ev.groups)
    norm = ev.matrix(normalize=True)
    assert norm.dtype == np.float64 and np.allclose(norm.sum(1), 1) and norm[3, 16] == table[3, 16] / table[3].sum()


def test_top_ordering():
    table = np.zeros((4, 5), np.int64)
    table[np.arange(4), np.arange(4)] = 10
    table[2, 0], table[0, 1], table[0, 3], table[3, 1], table[1, 4] = 7, 7, 2, 9, 50       # (column 4: nowhere, never listed)
    ev = _loaded(table, np.zeros(4, np.int64), n_joints=4, joint_names=['a', 'b', 'c', 'd'])
    assert ev.top() == [('d', 'b', 9, 1.0), ('a', 'b', 7, 7 / 9), ('c', 'a', 7, 1.0), ('a', 'd', 2, 2 / 9)]
    assert ev.top(2) == ev.top()[:2] and ev.top(0) == []
    assert _loaded(table, np.zeros(4, np.int64), n_joints=4).top(1) == [(3, 1, 9, 1.0)]      # unnamed joints: indices


def test_empty_rows_read_nan():
    table = np.zeros((3, 4), np.int64)
    table[0, 0], table[0, 3] = 3, 1
    ev = _loaded(table, np.zeros(3, np.int64), n_joints=3, joint_names=['a', 'b', 'c'],
                 joint_groups={'rest': {'b', 'c'}}, mirror=[0, 2, 1])
    assert ev.valid('rest') == 0 and all(math.isnan(v) for v in ev.rates('rest').values()) and math.isnan(ev.pckh('rest'))
    assert ev.rates('all') == {'hit': 0.75, 'mirror': 0.0, 'other': 0.0, 'nowhere': 0.25, 'mutual': 0.0}
    assert np.isnan(ev.matrix(normalize=True)[1]).all() and ev.top() == []
    with pytest.raises(KeyError):
        ev.rates('total_mpii')


def test_merge_state_and_what_they_refuse():
    mirror = ref.MPII_MIRROR
    a, b = _random_tables(16, mirror, seed=4), _random_tables(16, mirror, seed=5)
    one, two = _loaded(*a), _loaded(*b)
    one.merge(two)
    assert np.array_equal(one.counts().numpy(), a[0] + b[0]) and np.array_equal(one.mutual().numpy(), a[1] + b[1])
    assert np.array_equal(two.counts().numpy(), b[0])
    state = one.state_dict()
    assert set(state) == {'threshold', 'mirror', 'table', 'mutual'} and state['threshold'] == 0.5
    back = JointConfusion()
    back.load_state_dict(state)
    assert torch.equal(back.counts(), one.counts()) and torch.equal(back.mutual(), one.mutual())
    back.reset()
    assert not back.counts().any() and not back.mutual().any()
    # the threshold is held as the fp64 value of its fp32 rounding
    assert JointConfusion(threshold=0.1).threshold == float(np.float32(0.1)) != 0.1
    for other in (JointConfusion(threshold=0.25), JointConfusion(mirror=range(16)), JointConfusion(n_joints=15)):
        with pytest.raises(ValueError, match='merge needs the same joints, threshold and mirror'):
            one.merge(other)
        with pytest.raises(ValueError):
            other.load_state_dict(state)
    with pytest.raises(ValueError, match='tables of shape'):
        JointConfusion().load_state_dict(dict(state, mutual=torch.zeros(15, dtype=torch.int64)))
    for methods in ('merge', 'all_reduce', 'reset', '_rows', '_names'):      # from the base, not copies
        assert methods not in vars(JointConfusion) and methods in vars(evaluator._JointTables)


def test_constructor_refuses():
    with pytest.raises(ValueError, match=r'mirror is not an involution of 0\.\.2 \(mirror\[0\] = 1\)'):
        JointConfusion(n_joints=3, mirror=[1, 2, 0])
    with pytest.raises(ValueError, match=r'mirror is not an involution of 0\.\.2 \(mirror\[1\] = 3\)'):
        JointConfusion(n_joints=3, mirror=[0, 3, 2])
    with pytest.raises(ValueError, match='15 mirror indices for 16 joints'):
        JointConfusion(mirror=range(15))
    with pytest.raises(ValueError, match='at most 64 joints'):
        JointConfusion(n_joints=65)
    for t in (-0.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='threshold'):
            JointConfusion(threshold=t)


def test_wrong_joint_count_is_refused_before_the_library(monkeypatch):
    def touched(*a):
        raise AssertionError('the library was called: %r' % (a[0],))
    monkeypatch.setattr(evaluator, 'call', touched)
    monkeypatch.setattr(evaluator, 'ptr', touched)
    args = score_ref.awkward(*score_ref.case(5, 3, seed=1)[:6])
    ev = JointConfusion(n_joints=4)
    with pytest.raises(ValueError, match='3 joints, the tables have 4'):
        ev.add_normalized(*args)
    assert not ev._tables and not ev._identity
    pred, target, mask, head, m, b = args
    with pytest.raises(ValueError, match='3 joints, the tables have 4'):
        ev.add(pred, target, mask, head)
    assert not ev._tables
    # target_mass: the shapes and the mirror, before the library
    hm = torch.zeros(5, 3, 8, 8)
    with pytest.raises(ValueError, match='heat-maps'):
        evaluator.target_mass(hm[0], target, mask, head, m, b)
    with pytest.raises(ValueError, match='targets of shape'):
        evaluator.target_mass(hm[:, :2], target, mask, head, m, b)
    with pytest.raises(ValueError, match='between 1 and 64 joints'):
        evaluator.target_mass(torch.zeros(5, 65, 8, 8), target, mask, head, m, b)
    with pytest.raises(ValueError, match='mirror is not an involution'):
        evaluator.target_mass(hm, target, mask, head, m, b, mirror=[1, 2, 0])
    with pytest.raises(ValueError, match='threshold'):
        evaluator.target_mass(hm, target, mask, head, m, b, threshold=-1.0)


# ------------------------------------------------------------------ the C ABI
def _refusals():
    """(entry point, arguments without the stream, return code, dsnt_last_error()); X is a non-null pointer that is never
    followed, the mirrors are host arrays."""
    X, N = C.c_void_p(4096), None
    ints = lambda *v: C.cast((C.c_int * len(v))(*v), C.c_void_p)
    ok3, ok64 = ints(0, 2, 1), ints(*[j ^ 1 for j in range(64)])
    keep = [ok3, ok64]
    rows = []

    def both(text, rc=3, ptrs=(X,) * 6, thr=0.5, mirror=ok3, outs=(X, X), B=4, J=3):
        keep.append(mirror)
        rows.append(('dsnt_joint_confusion', ptrs + (thr, mirror) + outs + (B, J), rc, b'dsnt_joint_confusion: ' + text))
        rows.append(('dsnt_target_mass', ptrs + (thr, mirror) + outs[:1] + (B, J, 8, 8), rc, b'dsnt_target_mass: ' + text))

    for k in range(6):
        both(b'null pointer', ptrs=(X,) * k + (N,) + (X,) * (5 - k))
    both(b'null pointer', mirror=N)
    both(b'null pointer', outs=(N, X))
    rows.append(('dsnt_joint_confusion', (X,) * 6 + (0.5, ok3, X, N, 4, 3), 3, b'dsnt_joint_confusion: null pointer'))
    both(b'B=0 out of range', B=0)
    both(b'B=-3 out of range', B=-3)
    both(b'J=0 outside 1..64', J=0)
    both(b'J=65 outside 1..64', J=65, mirror=ok64)
    both(b'J=-1 outside 1..64', J=-1)
    both(b'threshold -0.5 is negative or not finite', thr=-0.5)
    both(b'threshold nan is negative or not finite', thr=float('nan'))
    both(b'threshold inf is negative or not finite', thr=float('inf'))
    both(b'mirror is not an involution of 0..2 (mirror[0] = 1)', mirror=ints(1, 2, 0))
    both(b'mirror is not an involution of 0..2 (mirror[1] = 0)', mirror=ints(0, 0, 1))
    both(b'mirror is not an involution of 0..2 (mirror[1] = 3)', mirror=ints(0, 3, 2))
    both(b'mirror is not an involution of 0..2 (mirror[0] = -1)', mirror=ints(-1, 1, 2))
    both(b'mirror is not an involution of 0..63 (mirror[63] = 62)', J=64, mirror=ints(*([j ^ 1 for j in range(62)] + [62, 62])))
    # the order: the first of several faults is the one reported
    both(b'B=0 out of range', B=0, J=65, thr=-1.0)
    both(b'J=65 outside 1..64', J=65, thr=-1.0)
    both(b'threshold -1 is negative or not finite', thr=-1.0, mirror=ints(1, 2, 0))

    def maps(text, rc, B=4, J=3, h=8, w=8, mirror=ok3):
        rows.append(('dsnt_target_mass', (X,) * 6 + (0.5, mirror, X, B, J, h, w), rc, b'dsnt_target_mass: ' + text))
    maps(b'bad map size 0x8', 1, h=0)
    maps(b'bad map size 8x-2', 1, w=-2)
    maps(b'bad map size 4096x4096', 1, h=4096, w=4096)
    maps(b'B=33554432 out of range', 3, B=1 << 25, J=64, mirror=ok64)
    return rows, keep


def test_entry_points_refuse_bad_arguments_without_gpu():
    from dsnt import _lib
    lib = _lib.load()
    assert lib.dsnt_version() >= 128
    P, I, F = _lib.P, _lib.I, _lib.F
    assert _lib.SIGNATURES['dsnt_joint_confusion'] == [P, P, P, P, P, P, F, P, P, P, I, I, P]
    assert _lib.SIGNATURES['dsnt_target_mass'] == [P, P, P, P, P, P, F, P, P, I, I, I, I, P]
    rows, keep = _refusals()
    assert len(rows) >= 50
    for name, args, rc, text in rows:
        got = getattr(lib, name)(*args, None)
        assert (got, lib.dsnt_last_error()) == (rc, text), (name, args)


# ------------------------------------------------------------------ the inputs of the GPU tests
@pytest.mark.parametrize('B,J', ref.SHAPES, ids=['%dx%d' % s for s in ref.SHAPES])
def test_confusion_cases_are_clear_of_every_edge(B, J):
    """No d_jk within 1e-9 relative of the threshold and no two candidate distances of a joint within 1e-9 relative of
    each other, so that a contraction on the device changes no cell; and every kind of cell that J joints allow."""
    args = ref.shape_case(B, J)
    pred, target, m, b, mask, head = args
    assert pred.dtype == target.dtype == mask.dtype == np.float32 and m.dtype == b.dtype == head.dtype == np.float64
    edge, gap = ref.margins(*args)
    assert edge > 1e-9 and gap > 1e-9, (edge, gap)
    mirror = ref.mirror_of(J)
    assert all(mirror[mirror[j]] == j for j in range(J))
    table, mutual = ref.restate(*args, mirror)
    kinds = ref.kinds(table, mutual, mirror)
    assert table.sum() == (mask == 1).sum() and all(mutual[j] == mutual[mirror[j]] for j in range(J))
    for kind in ('hit', 'nowhere') + (('mirror', 'other', 'mutual') if J >= 3 else ()):
        assert kinds[kind] > 0, (kind, kinds)
    assert kinds['mutual'] < kinds['mirror'] or J < 3           # collapses too, not only exchanges
    assert np.isnan(target[mask != 1]).all() and np.isnan(pred[mask == 1]).any() and (mask == 0).all(1).any()


@pytest.mark.parametrize('shape', ref.MASS_SHAPES, ids=['%dx%d-%dx%d' % s for s in ref.MASS_SHAPES])
def test_mass_cases_are_clear_of_every_edge(shape):
    """No pixel centre within 1e-9 relative of the edge of a disc; every case holds a disc without a pixel, one with
    pixels, a joint that is not counted and one without an annotated mirror."""
    B, J, h, w = shape
    hm, target, m, b, mask, head = ref.mass_shape_case(*shape)
    assert hm.dtype == np.float32 and hm.shape == shape and np.allclose(hm.sum((2, 3)), 1, atol=1e-5)
    mirror = ref.mirror_of(J)
    out, pixels, margin = ref.restate_mass(hm, target, m, b, mask, head, mirror)
    assert margin > 1e-9, margin
    assert (pixels > 0).any() and (out[pixels == 0] == 0).all()
    assert np.array_equal(np.isnan(out), pixels < 0) and np.isnan(out[mask != 1]).all()
    if B * J > 2:                                              # (one person of two joints is the bimodal map alone)
        assert (pixels == 0).any() and (mask != 1).any() and (np.isnan(out[..., 1]) & ~np.isnan(out[..., 0])).any()
    # the predictions that go with it into `Reliability`: clear of the threshold, hits and misses
    d = score_ref.distance(ref.mass_pred(target), target, m, b, head)[mask == 1]
    assert score_ref.clear_of_thresholds(d, score_ref.THR1)
    assert (d <= 0.5).any() and (d > 0.5).any() or shape != (3, 16, 64, 64)        # (the shape that test feeds it)
    # the bimodal map: most of its mass in the two discs, a good part of it in each
    assert out[0, 0, 0] > 0.5 and out[0, 0, 1] > 0.2 and out[0, 0].sum() > 0.8, out[0, 0]
