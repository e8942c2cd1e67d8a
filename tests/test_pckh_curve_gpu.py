"""The PCKh histogram (`pckh_hist_kernel`, csrc/pckh.hip, through `dsnt_pckh_hist`) and `dsnt.evaluator.PCKhCurve`
against a numpy fp64 restatement.

The table is integer, so it must equal the restatement exactly: every case first checks on the CPU that no distance lies
within 1e-9 relative of a threshold, so that an fp64 contraction difference cannot move a joint across a bin edge (the
boundary cases use values that are exact).  `dist` is held to 1e-9 head lengths: coordinates below 1e3 px in fp64 round
at about 1e-13 px, over heads of at least 40 px, which leaves five orders of margin and is still seven orders below the
bin width of 0.01.

Shapes are chosen around the two constants of include/dsnt_hip.h: DSNT_PCKH_HIST_MAX_BLOCKS x DSNT_PCKH_HIST_BLOCK
joints are one grid stride, and J * (T + 1) <= DSNT_PCKH_HIST_LDS_CELLS selects the LDS path.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from dsnt import _lib
from dsnt._lib import call, ptr

pytestmark = pytest.mark.gpu

MAX_T, LDS_CELLS, BLOCK, MAX_BLOCKS = 64, 4096, 256, 64        # include/dsnt_hip.h: DSNT_PCKH_HIST_*
SENTINEL = -7


def thr32(values):
    """Thresholds as `PCKhCurve` holds them: the fp64 values of their fp32 roundings."""
    return np.asarray(values, np.float64).astype(np.float32).astype(np.float64)


DEFAULT = thr32(np.arange(51) / 100)


def distance(pred, target, m, b, head):
    """`pckh_distance` of tests/test_fc_pckh_gpu.py: bmm(x, m) + b on row vectors, the distance over the head length."""
    with np.errstate(all='ignore'):
        p = np.einsum('bji,bik->bjk', pred.astype(np.float64), m) + b[:, None, :]
        t = np.einsum('bji,bik->bjk', target.astype(np.float64), m) + b[:, None, :]
        return np.sqrt((p[..., 0] - t[..., 0]) ** 2 + (p[..., 1] - t[..., 1]) ** 2) / head[:, None]


def restate(pred, target, m, b, mask, head, thr):
    """(table [J, T + 1], dist [B, J]): a joint with mask == 1 counts in the first bin whose threshold it does not exceed;
    NaN, inf and anything beyond the last threshold count in bin T; dist is NaN where the mask is not 1."""
    B, J = mask.shape
    T = len(thr)
    d = distance(pred, target, m, b, head)
    valid = mask == 1
    k = np.searchsorted(thr, np.where(np.isfinite(d), d, 0.0), side='left')
    k[~np.isfinite(d)] = T
    table = np.zeros((J, T + 1), np.int64)
    jj = np.broadcast_to(np.arange(J), (B, J))
    np.add.at(table, (jj[valid], k[valid]), 1)
    return table, np.where(valid, d, np.nan)


def hist_dev(pred, target, m, b, mask, head, thr, fill=0, want_dist=True):
    """One `dsnt_pckh_hist` call into a table pre-filled with `fill`; table and dist carry 8 guard cells behind them."""
    B, J = mask.shape
    T = len(thr)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (pred, target, m, b, mask, head)]
    assert dev[0].dtype == dev[1].dtype == dev[4].dtype == torch.float32 and dev[2].dtype == dev[5].dtype == torch.float64
    cells = J * (T + 1)
    table = torch.full((cells + 8,), SENTINEL, dtype=torch.int64, device='cuda')
    table[:cells] = fill
    dist = torch.full((B * J + 8,), float(SENTINEL), dtype=torch.float64, device='cuda') if want_dist else None
    call('dsnt_pckh_hist', *[ptr(t) for t in dev], (C.c_double * T)(*thr), T, ptr(table), ptr(dist), B, J)
    assert (table[cells:] == SENTINEL).all().item()
    if want_dist:
        assert (dist[B * J:] == SENTINEL).all().item()
        dist = dist[:B * J].view(B, J).cpu().numpy()
    return table[:cells].view(J, T + 1).cpu().numpy(), dist


def _identity(B):
    return np.tile(np.eye(2), (B, 1, 1)), np.zeros((B, 2))


def _case(B, J, seed):
    """`_pckh_case` of tests/test_fc_pckh_gpu.py: about half the predictions within 0.5 head lengths, a non-symmetric
    transform per image, masks of 0, 1, 0.5 and 2."""
    r = np.random.default_rng(seed)
    target = r.uniform(-0.9, 0.9, (B, J, 2)).astype(np.float32)
    pred = (target + r.normal(0, 0.2, (B, J, 2))).astype(np.float32)
    m = np.array([[150.0, 90.0], [-20.0, 60.0]]) + r.uniform(-10, 10, (B, 2, 2))
    b = r.uniform(0, 400, (B, 2))
    head = r.uniform(40, 120, B)
    mask = r.choice(np.array([0, 1, 1, 1, 0.5, 2], np.float32), (B, J))
    return pred, target, m, b, mask, head


def _clear_of_edges(d, thr):
    """No distance within 1e-9 relative of a threshold (for the threshold 0: no distance of exactly 0)."""
    gap = np.abs(d[..., None] - thr)
    return bool((gap > 1e-9 * thr).all())


ONE_STRIDE = MAX_BLOCKS * BLOCK // 16 + 1                      # the smallest B with B * 16 past one grid stride
T64 = thr32(np.arange(1, 65) / 128)                            # 64 thresholds ending in 0.5
T63 = T64[1:]
assert 64 * (len(T63) + 1) == LDS_CELLS < 64 * (len(T64) + 1)  # J = 64: the largest LDS table, and the direct-global path
CASES = [(1, 1, DEFAULT), (37, 7, DEFAULT), (16, 16, DEFAULT), (70, 16, DEFAULT), (ONE_STRIDE, 16, DEFAULT),
         (37, 7, thr32([0.5])), (40, 64, T63), (40, 64, T64)]


@pytest.mark.parametrize('B,J,thr', CASES, ids=['%dx%d-T%d' % (B, J, len(t)) for B, J, t in CASES])
def test_table_and_dist_match_restatement(B, J, thr):
    args = _case(B, J, seed=B * 100 + J)
    T = len(thr)
    want, want_d = restate(*args, thr)
    assert _clear_of_edges(distance(args[0], args[1], args[2], args[3], args[5]), thr)
    table, dist = hist_dev(*args, thr)
    valid = args[4] == 1
    print('B=%d J=%d T=%d: %d valid, %d in bin T, %d hits at %g' % (B, J, T, valid.sum(), want[:, T].sum(),
                                                                     want[:, :T].sum(), thr[-1]))
    assert np.array_equal(table, want), (B, J, T)
    assert table.sum() == valid.sum()
    if B * J >= 256:                                           # the case tests both outcomes, and the overflow bin
        assert thr[-1] == 0.5 and 0.1 < want[:, :T].sum() / valid.sum() < 0.9 and want[:, T].sum() > 0
        assert (want[:, :T].sum(0) > 0).sum() >= T // 2        # and the bins below 0.5 are in use
    # dist: d where the mask is 1, NaN elsewhere
    assert np.isnan(dist[~valid]).all() and not np.isnan(dist[valid]).any()
    err = np.abs(dist[valid] - want_d[valid]).max() if valid.any() else 0.0
    print('dist: worst error %.3e head lengths' % err)
    assert err <= 1e-9
    # dist = NULL: the same table
    assert np.array_equal(hist_dev(*args, thr, want_dist=False)[0], want)
    # a transposed multiply fills other bins on these inputs, so the comparison above tells the two apart
    wrong = restate(args[0], args[1], args[2].transpose(0, 2, 1), *args[3:], thr)[0]
    assert B * J < 256 or np.abs(wrong - want).sum() >= 10


def test_kernel_adds_and_never_stores():
    """A table that holds 7 in every cell comes back as 7 + the restatement, on the LDS path and on the direct one."""
    for B, J, thr in ((16, 16, DEFAULT), (40, 64, T64)):
        args = _case(B, J, seed=B * 100 + J)
        want = restate(*args, thr)[0]
        assert _clear_of_edges(distance(args[0], args[1], args[2], args[3], args[5]), thr)
        assert np.array_equal(hist_dev(*args, thr, fill=7)[0], want + 7)


def test_edges():
    """m = I, b = 0, |(3, 4)| = 5 and head 10: d = 0.5 exactly, the bin of 0.5 (a hit at 0.5, a miss at 0.49); one ulp less
    head: bin T; d = 0: bin 0 when the first threshold is 0.  Through `PCKhCurve.add`, which supplies the identity."""
    from dsnt.evaluator import PCKhCurve
    T = len(DEFAULT)
    one = np.ones((1, 1), np.float32)
    m, b = _identity(1)
    p, z = np.array([[[3.0, 4.0]]], np.float32), np.zeros((1, 1, 2), np.float32)
    at = int(np.flatnonzero(DEFAULT == 0.5)[0])
    assert at == T - 1 and DEFAULT[0] == 0.0
    for pred, target, head, want_bin in ((p, z, 10.0, at), (z, p, 10.0, at), (p, z, np.nextafter(10.0, 0.0), T),
                                         (p, z, np.nextafter(10.0, 20.0), at), (p, p, 10.0, 0), (z, z, 10.0, 0)):
        head = np.array([head])
        want = np.zeros((1, T + 1), np.int64)
        want[0, want_bin] = 1
        assert np.array_equal(restate(pred, target, m, b, one, head, DEFAULT)[0], want)
        assert np.array_equal(hist_dev(pred, target, m, b, one, head, DEFAULT)[0], want), (head, want_bin)
        ev = PCKhCurve(n_joints=1)
        for _ in range(2):                                     # the second call takes the cached identity
            ev.add(*[torch.from_numpy(a).cuda() for a in (pred, target, one, head)])
        assert np.array_equal(ev.counts().numpy(), 2 * want)
        assert ev.pckh(0.5, 0) == (1.0 if want_bin < T else 0.0) and ev.pckh(0.49, 0) == (1.0 if want_bin < at else 0.0)
    assert len(ev._identity) == 1


def test_non_finite_coordinates_and_masks():
    """The cases of `test_pckh_non_finite_coordinates`: NaN and inf coordinates under mask 0 change no cell, under mask 1
    they count in bin T, and the joints beside them are untouched; a zero head length sends every valid joint to bin T."""
    nan, inf = float('nan'), float('inf')
    bad = [((nan, 0.0), (0.0, 0.0)), ((0.0, 0.0), (0.0, nan)), ((inf, 0.0), (0.0, 0.0)), ((0.0, 0.0), (-inf, 0.0)),
           ((inf, inf), (inf, inf)), ((nan, nan), (nan, nan))]
    B, J, T = len(bad), 4, len(DEFAULT)    # joint 0: bad under mask 0; joint 1: bad under mask 1; joints 2, 3: d = 0.5, 1
    pred, target = np.zeros((B, J, 2), np.float32), np.zeros((B, J, 2), np.float32)
    for n, (p, t) in enumerate(bad):
        pred[n, 0] = pred[n, 1] = p
        target[n, 0] = target[n, 1] = t
    pred[:, 2] = (3.0, 4.0)
    pred[:, 3] = (6.0, 8.0)
    mask = np.tile(np.array([0, 1, 1, 1], np.float32), (B, 1))
    mask[0, 0], mask[1, 0] = 0.5, 2        # neither counts
    m, b = _identity(B)
    head = np.full(B, 10.0)
    want = np.zeros((J, T + 1), np.int64)
    want[1, T] = want[2, T - 1] = want[3, T] = B
    table, dist = hist_dev(pred, target, m, b, mask, head, DEFAULT)
    assert np.array_equal(table, want) and np.array_equal(restate(pred, target, m, b, mask, head, DEFAULT)[0], want)
    assert np.isnan(dist[:, 0]).all() and (dist[:, 2] == 0.5).all() and (dist[:, 3] == 1.0).all()
    assert not np.isfinite(dist[:, 1]).any()
    head[:] = 0.0                          # 5 / 0 = inf
    want[:] = 0
    want[1:, T] = B
    table, dist = hist_dev(pred, target, m, b, mask, head, DEFAULT)
    assert np.array_equal(table, want) and np.array_equal(restate(pred, target, m, b, mask, head, DEFAULT)[0], want)
    assert np.isinf(dist[:, 2:]).all() and np.isnan(dist[:, 0]).all()


def _batches(n=3, B=16, J=16, seed=40):
    out = []
    for k in range(n):
        args = _case(B, J, seed=seed + k)
        assert _clear_of_edges(distance(args[0], args[1], args[2], args[3], args[5]), DEFAULT)
        out.append(args)
    return out


def _feed(ev, args, **kw):
    pred, target, m, b, mask, head = [torch.from_numpy(a).cuda() for a in args]
    return ev.add_normalized(pred, target, mask, head, m, b, **kw)


def test_same_counts_as_the_single_threshold_evaluator():
    """Three batches into one PCKhCurve and into PCKhEvaluator(t): every joint and group holds the same counts at 0.5, 0.2
    and 0.1, and the oracle's evaluator on the back-projected coordinates holds them at 0.5."""
    from dsnt.evaluator import PCKhCurve, PCKhEvaluator
    from dsnt_oracle.evaluator import PCKhEvaluator as OracleEval
    batches = _batches()
    curve = PCKhCurve()
    singles = {t: PCKhEvaluator(t) for t in (0.5, 0.2, 0.1)}
    oracle = OracleEval(0.5)
    for args in batches:
        _feed(curve, args)
        for ev in singles.values():
            _feed(ev, args)
        pred, target, m, b, mask, head = [torch.from_numpy(a) for a in args]
        oracle.add(torch.baddbmm(b[:, None], pred.double(), m), torch.baddbmm(b[:, None], target.double(), m), mask, head)
    names = PCKhEvaluator.JOINT_NAMES + list(PCKhEvaluator.JOINT_GROUPS)
    for t, ev in singles.items():
        for name in names:
            assert curve.pckh(t, name) == ev.meters[name].value()[0], (t, name)
            assert curve.valid(name) == int(ev.meters[name].count), (t, name)
    counts = curve.counts()
    for j, name in enumerate(PCKhEvaluator.JOINT_NAMES):
        assert curve.pckh(0.5, j) == curve.pckh(0.5, name)
        assert oracle.meters[name].n == counts[j].sum() and oracle.meters[name].total == counts[j, :-1].sum(), name
    for g in PCKhEvaluator.JOINT_GROUPS:
        assert curve.pckh(0.5, g) == oracle.meters[g].value()[0] and curve.valid(g) == oracle.meters[g].n, g
    assert 0.1 < curve.pckh(0.5) < 0.9 and curve.pckh(0.1) < curve.pckh(0.2) < curve.pckh(0.5)


def test_class_behaviour():
    from dsnt.evaluator import PCKhCurve
    batches = _batches(4)
    want = sum(restate(*a, DEFAULT)[0] for a in batches)
    whole, first, second, again = PCKhCurve(), PCKhCurve(), PCKhCurve(), PCKhCurve()
    for k, args in enumerate(batches):
        d = _feed(whole, args, return_distances=True)
        assert _feed(again, args) is None
        _feed(first if k < 2 else second, args)
        ref = restate(*args, DEFAULT)[1]
        valid = args[4] == 1
        assert d.dtype == torch.float64 and d.shape == valid.shape and d.is_cuda
        d = d.cpu().numpy()
        assert np.isnan(d[~valid]).all() and np.abs(d[valid] - ref[valid]).max() <= 1e-9
    assert whole.counts().dtype == torch.int64 and np.array_equal(whole.counts().numpy(), want)
    assert torch.equal(again.counts(), whole.counts())                   # two identical passes: the same table
    first.merge(second)
    assert torch.equal(first.counts(), whole.counts())
    assert np.array_equal(second.counts().numpy(), sum(restate(*a, DEFAULT)[0] for a in batches[2:]))
    # the state loads into an object that never sees a GPU, and answers the same
    state = whole.state_dict()
    assert not state['table'].is_cuda and not state['thresholds'].is_cuda
    cpu = PCKhCurve(thresholds=[0.1, 0.2])
    cpu.load_state_dict(state)
    for name in ('total_mpii', 'ubody', 'all', 'lwrist', 3):
        assert torch.equal(cpu.curve(name), whole.curve(name)) and cpu.auc(name) == whole.auc(name)
    t, c = whole.thresholds.numpy(), whole.curve().numpy()
    assert np.array_equal(t, DEFAULT)
    area = (getattr(np, 'trapezoid', None) or np.trapz)(c, t) / (t[-1] - t[0])       # np.trapz, by its newer name where it has one
    assert abs(whole.auc() - area) <= 4 * np.spacing(area) and 0.05 < area < 0.6
    with pytest.raises(KeyError):
        whole.pckh(0.123)
    with pytest.raises(ValueError):
        whole.merge(PCKhCurve(thresholds=[0.1, 0.5]))
    with pytest.raises(ValueError):
        _feed(PCKhCurve(n_joints=7), batches[0])
    # reset zeroes the table, and the evaluator counts again from there
    whole.reset()
    assert not whole.counts().any().item()
    _feed(whole, batches[0])
    assert np.array_equal(whole.counts().numpy(), restate(*batches[0], DEFAULT)[0])


def test_other_joint_counts_and_thresholds_through_the_class():
    """7 unnamed joints and four thresholds given as Python floats: per-index rows and the group 'all'."""
    from dsnt.evaluator import PCKhCurve
    thr = [0.05, 0.1, 0.3, 0.5]
    args = _case(37, 7, seed=3707)
    assert _clear_of_edges(distance(args[0], args[1], args[2], args[3], args[5]), thr32(thr))
    ev = PCKhCurve(thresholds=thr, n_joints=7)
    _feed(ev, args)
    want = restate(*args, thr32(thr))[0]
    assert np.array_equal(ev.counts().numpy(), want)
    assert ev.valid('all') == want.sum() and ev.valid(6) == want[6].sum()
    assert ev.pckh(0.3, 'all') == want[:, :3].sum() / want.sum()
    with pytest.raises(KeyError):
        ev.curve('total_mpii')
    with pytest.raises(KeyError):
        ev.curve(7)


def test_refusals_launch_nothing():
    """T outside 1..64, a descending pair, an equal pair, a NaN and an inf threshold, a null pointer and an empty batch are
    refused on the host with DSNT_ERR_ARG; the table is unchanged."""
    fn = _lib.fn('dsnt_pckh_hist')
    B, J = 4, 3
    args = _case(B, J, seed=9)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
    table = torch.full((J * (MAX_T + 2),), SENTINEL, dtype=torch.int64, device='cuda')
    stream = _lib.stream_ptr()

    def rc(thr, T=None, table_ptr=ptr(table), B=B, J=J):
        T = len(thr) if T is None else T
        arr = (C.c_double * max(len(thr), 1))(*thr)
        return fn(*[ptr(t) for t in dev], arr, T, table_ptr, None, B, J, stream)
    nan, inf = float('nan'), float('inf')
    bad = [rc([0.5], T=0), rc([0.5], T=-1), rc(list(np.arange(65) / 100.0)), rc([0.2, 0.1]), rc([0.1, 0.3, 0.2]),
           rc([0.1, 0.1]), rc([0.1, nan]), rc([nan]), rc([0.1, inf]), rc([-inf, 0.1]), rc([0.5], table_ptr=None),
           rc([0.5], B=0), rc([0.5], J=0)]
    assert bad == [3] * len(bad), bad
    assert b'dsnt_pckh_hist' in _lib.fn('dsnt_last_error')()
    assert fn(*[ptr(t) for t in dev], None, 1, ptr(table), None, B, J, stream) == 3
    torch.cuda.synchronize()
    assert (table == SENTINEL).all().item()
    # the same table takes a call that is in order
    assert rc(list(np.arange(64) / 100.0)) == 0
    torch.cuda.synchronize()
    got = table[:J * (MAX_T + 1)].view(J, MAX_T + 1).cpu().numpy() - SENTINEL
    assert _clear_of_edges(distance(args[0], args[1], args[2], args[3], args[5]), np.arange(64) / 100.0)
    assert np.array_equal(got, restate(*args, np.arange(64) / 100.0)[0]) and (table[J * (MAX_T + 1):] == SENTINEL).all().item()


def test_add_without_host_sync():
    """After the first call has allocated the table, `add_normalized` and `add` enqueue and return."""
    from dsnt.evaluator import PCKhCurve
    batches = _batches(2)
    dev = [[torch.from_numpy(a).cuda() for a in args] for args in batches]
    ev = PCKhCurve()

    def step(k, **kw):
        pred, target, m, b, mask, head = dev[k]
        out = ev.add_normalized(pred, target, mask, head, m, b, **kw)
        ev.add(pred, target, mask, head)
        return out
    step(0)                                         # first call: the table and the identity transform are set up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')         # any synchronising call raises
    try:
        step(1)
        d = step(1, return_distances=True)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    want = restate(*batches[0], DEFAULT)[0] + 2 * restate(*batches[1], DEFAULT)[0]
    for k in (0, 1, 1):                             # what `add` saw: the same coordinates under the identity
        pred, target, _, _, mask, head = batches[k]
        assert _clear_of_edges(distance(pred, target, *_identity(16), head), DEFAULT)
        want = want + restate(pred, target, *_identity(16), mask, head, DEFAULT)[0]
    assert np.array_equal(ev.counts().numpy(), want)
    assert d.shape == (16, 16) and torch.isfinite(d).any().item()
