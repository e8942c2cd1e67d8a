"""`dsnt.evaluator.PCKhCurve` without a GPU: every reading method on a hand-written table loaded through
`load_state_dict`, and `all_reduce` over a world-2 gloo group.

The table (thresholds 0.1, 0.2, 0.5; columns: d <= 0.1, <= 0.2, <= 0.5, beyond):

    rankle  1 2 3 4      valid 10, curve 0.1 0.3 0.6
    pelvis  4 0 0 0      valid  4, curve 1 1 1
    rwrist  0 0 5 5      valid 10, curve 0 0 0.5
    every other joint 0: nothing valid, NaN

ubody holds rwrist alone; total_anewell and total_mpii hold rankle and rwrist: 1 2 8 9, valid 20, curve 0.05 0.15 0.55;
all adds pelvis: 5 2 8 9, valid 24, curve 5/24 7/24 15/24.
"""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

THR = [0.1, 0.2, 0.5]
T32 = [float(np.float32(t)) for t in THR]


def _table():
    t = torch.zeros(16, 4, dtype=torch.int64)
    t[0] = torch.tensor([1, 2, 3, 4])
    t[6] = torch.tensor([4, 0, 0, 0])
    t[10] = torch.tensor([0, 0, 5, 5])
    return t


def _loaded():
    from dsnt.evaluator import PCKhCurve
    ev = PCKhCurve()                                   # 51 default thresholds: the state brings its own
    ev.load_state_dict({'thresholds': torch.tensor(T32, dtype=torch.float64), 'table': _table()})
    return ev


def _trapezoid(c):
    return ((T32[1] - T32[0]) * (c[0] + c[1]) / 2 + (T32[2] - T32[1]) * (c[1] + c[2]) / 2) / (T32[2] - T32[0])


def test_defaults():
    from dsnt.evaluator import PCKhCurve, PCKhEvaluator
    ev = PCKhCurve()
    want = [float(np.float32(k / 100)) for k in range(51)]
    assert ev.thresholds.dtype == torch.float64 and ev.thresholds.tolist() == want and ev.T == 51
    assert ev.counts().shape == (16, 52) and ev.counts().dtype == torch.int64 and not ev.counts().any()
    assert ev.JOINT_NAMES is PCKhEvaluator.JOINT_NAMES and ev.JOINT_GROUPS is PCKhEvaluator.JOINT_GROUPS
    assert math.isnan(ev.pckh(0.5)) and ev.valid() == 0 and torch.isnan(ev.curve()).all()
    # 0.2 is held as the fp32 value the single-threshold kernel compares against, and found again from the Python float
    assert ev.thresholds[20].item() == float(np.float32(0.2)) != 0.2 and ev._index(0.2) == 20
    for bad in ([], list(range(65)), [0.2, 0.1], [0.1, 0.1], [0.1, float('nan')], [0.1, float('inf')],
                [0.1, 0.1 + 1e-12]):                   # (the last pair is one fp32 value)
        with pytest.raises(ValueError):
            PCKhCurve(thresholds=bad)


def test_reading_a_hand_written_table():
    ev = _loaded()
    assert ev.T == 3 and ev.thresholds.tolist() == T32 and torch.equal(ev.counts(), _table())
    want = {'rankle': (10, [0.1, 0.3, 0.6]), 'pelvis': (4, [1.0, 1.0, 1.0]), 'rwrist': (10, [0.0, 0.0, 0.5]),
            'ubody': (10, [0.0, 0.0, 0.5]), 'total_anewell': (20, [0.05, 0.15, 0.55]),
            'total_mpii': (20, [0.05, 0.15, 0.55]), 'all': (24, [5 / 24, 7 / 24, 15 / 24])}
    for name, (n, curve) in want.items():
        assert ev.valid(name) == n, name
        got = ev.curve(name)
        assert got.dtype == torch.float64 and got.shape == (3,) and got.tolist() == curve, name
        for t, c in zip(THR, curve):
            assert ev.pckh(t, name) == c
        assert ev.auc(name) == pytest.approx(_trapezoid(curve), rel=1e-15)
    assert ev.curve().tolist() == want['total_mpii'][1] and ev.valid() == 20          # the default name
    assert ev.auc() == pytest.approx(0.2875, abs=1e-7)           # (0.1 * 0.1 + 0.3 * 0.35) / 0.4, but for fp32's 0.1 and 0.2
    # a joint index reads the same row as its name
    assert ev.valid(0) == 10 and ev.curve(10).tolist() == [0.0, 0.0, 0.5] and ev.pckh(0.5, np.int64(6)) == 1.0
    # nothing valid: NaN, not an error
    assert ev.valid('lknee') == 0 and torch.isnan(ev.curve('lknee')).all() and math.isnan(ev.pckh(0.5, 'lknee'))
    assert math.isnan(ev.auc('lknee'))
    for bad in ('nose', 16, -1, True):
        with pytest.raises(KeyError):
            ev.curve(bad)
    for bad in (0.3, 0.25, 0.1 + 1e-6):
        with pytest.raises(KeyError):
            ev.pckh(bad)
    assert ev.pckh(np.float32(0.2)) == 0.15


def test_summary():
    from dsnt.evaluator import PCKhCurve
    ev = _loaded()
    s = ev.summary()
    assert set(s) == set(PCKhCurve.JOINT_NAMES) | set(PCKhCurve.JOINT_GROUPS) | {'auc'}
    assert s['rankle'] == 0.6 and s['pelvis'] == 1.0 and s['rwrist'] == 0.5 and s['total_mpii'] == 0.55
    assert s['all'] == 15 / 24 and math.isnan(s['headtop'])
    assert set(s['auc']) == set(PCKhCurve.JOINT_GROUPS)
    assert s['auc']['total_mpii'] == ev.auc() and s['auc']['all'] == ev.auc('all') and s['auc']['ubody'] == ev.auc('ubody')
    assert ev.summary(0.2)['total_anewell'] == 0.15
    with pytest.raises(KeyError):
        ev.summary(0.3)
    # one threshold: no area, and the summary leaves it out
    one = PCKhCurve(thresholds=[0.5])
    one.load_state_dict({'thresholds': torch.tensor([0.5], dtype=torch.float64), 'table': _table()[:, :2]})
    assert one.pckh(0.5, 'rankle') == 1 / 3 and 'auc' not in one.summary()
    with pytest.raises(ValueError):
        one.auc()


def test_merge_state_and_reset():
    from dsnt.evaluator import PCKhCurve
    a, b = _loaded(), _loaded()
    a.merge(b)
    assert torch.equal(a.counts(), 2 * _table()) and torch.equal(b.counts(), _table())
    assert a.valid('all') == 48 and a.curve('all').tolist() == b.curve('all').tolist()
    c = PCKhCurve(thresholds=THR)
    c.merge(a)                                             # constructed from Python floats: the same fp32 thresholds
    assert torch.equal(c.counts(), 2 * _table())
    for other in (PCKhCurve(), PCKhCurve(thresholds=[0.1, 0.2, 0.4]), PCKhCurve(thresholds=THR, n_joints=15)):
        with pytest.raises(ValueError):
            a.merge(other)
    state = a.state_dict()
    assert set(state) == {'thresholds', 'table'} and state['table'].dtype == torch.int64
    state['table'][0, 0] += 100                            # a copy, not the evaluator's own table
    assert torch.equal(a.counts(), 2 * _table())
    with pytest.raises(ValueError):
        a.load_state_dict({'thresholds': torch.tensor(T32, dtype=torch.float64), 'table': _table()[:, :3]})
    with pytest.raises(ValueError):
        PCKhCurve(n_joints=7).load_state_dict(state)
    a.reset()
    assert not a.counts().any() and a.T == 3
    a.all_reduce()                                         # no process group: nothing to do
    assert not a.counts().any()


def test_unnamed_joints_and_custom_groups():
    from dsnt.evaluator import PCKhCurve
    ev = PCKhCurve(thresholds=THR, n_joints=3)
    ev.load_state_dict({'thresholds': ev.thresholds, 'table': torch.tensor([[1, 0, 0, 1], [0, 0, 0, 0], [0, 2, 0, 0]])})
    assert set(ev.summary()) == {0, 1, 2, 'all', 'auc'} and set(ev.summary()['auc']) == {'all'}
    assert ev.curve('all').tolist() == [0.25, 0.75, 0.75] and ev.valid(2) == 2 and math.isnan(ev.pckh(0.5, 1))
    with pytest.raises(KeyError):
        ev.curve()                                         # no 'total_mpii' here
    named = PCKhCurve(thresholds=THR, n_joints=3, joint_names=['a', 'b', 'c'], joint_groups={'ends': {'a', 'c'}, 'mid': {'b'}})
    named.load_state_dict(ev.state_dict())
    assert named.curve('ends').tolist() == [0.25, 0.75, 0.75] and named.valid('mid') == 0
    assert math.isnan(named.summary()['mid']) and set(named.summary()['auc']) == {'ends', 'mid', 'all'}
    with pytest.raises(ValueError):
        PCKhCurve(n_joints=3, joint_names=['a', 'b'])


def test_entry_point_refuses_bad_thresholds_without_gpu():
    """The argument checks of `dsnt_pckh_hist` run on the host before anything is launched: no device is needed to see them."""
    import ctypes as C
    from dsnt import _lib
    fn = _lib.fn('dsnt_pckh_hist')
    assert _lib.load().dsnt_version() >= 122
    p = C.c_void_p(4096)                                   # never dereferenced: every call below is refused

    def rc(thr, T=None, table=p, B=4, J=3):
        arr = (C.c_double * max(len(thr), 1))(*thr)
        return fn(p, p, p, p, p, p, arr, len(thr) if T is None else T, table, None, B, J, None)
    nan, inf = float('nan'), float('inf')
    for thr, T, what in (([0.5], 0, b'T=0 outside 1..64'), ([0.01 * k for k in range(65)], None, b'T=65 outside 1..64'),
                         ([0.2, 0.1], None, b'strictly ascending (index 1)'), ([0.1, 0.2, 0.2], None, b'(index 2)'),
                         ([0.1, nan], None, b'threshold 1 is not finite'), ([inf], None, b'threshold 0 is not finite')):
        assert rc(thr, T) == 3 and what in _lib.fn('dsnt_last_error')(), (thr, _lib.fn('dsnt_last_error')())
    assert rc([0.5], table=None) == 3 and rc([0.5], B=0) == 3 and rc([0.5], J=0) == 3
    assert fn(p, p, p, p, p, p, None, 1, p, None, 4, 3, None) == 3


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        ev = _loaded()
        for _ in range(rank):                              # rank r holds (r + 1) tables
            ev.merge(_loaded())
        ev.all_reduce()
        q.put((rank, ev.counts(), ev.curve().tolist()))
    finally:
        dist.destroy_process_group()


def test_all_reduce_world2():
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r[0] for r in results) == [0, 1]
    for _, counts, curve in results:
        assert torch.equal(counts, 3 * _table()) and curve == [0.05, 0.15, 0.55]
