"""`dsnt_score_hist` and `dsnt_score_lookup` (csrc/pckh.hip), `dsnt.evaluator.Reliability` and `ScoreCalibration`, and the
`calibration=` keyword of `dsnt.inference.predict`, against the numpy restatement of tests/score_ref.py.

The table is integer and must equal the restatement exactly.  Its distance column compares fp64 values whose last bits may
differ by a contraction, so every case first checks on the CPU that no distance lies within 1e-9 relative of a threshold
(tests/test_pckh_curve_gpu.py has the reasoning); the hand-made cases use exact values.  Score rows need no margin: an
fp32 score widened to fp64 against fp32-valued edges compares exactly.  The comparison with `dsnt_pckh_hist` is device
against device on one distance expression and needs none either.

Shapes sit around the constants of include/dsnt_hip.h: DSNT_PCKH_HIST_MAX_BLOCKS x DSNT_PCKH_HIST_BLOCK joints are one
grid stride of the table kernel, J * (S + 2) * (T + 1) <= DSNT_SCORE_HIST_LDS_CELLS selects its LDS path, and
DSNT_SCORE_LOOKUP_MAX_BLOCKS x DSNT_SCORE_LOOKUP_BLOCK scores are one grid stride of the lookup.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import score_ref
from score_ref import EDGES20, THR1, THR3, THR15, f32
from dsnt import _lib
from dsnt._lib import call, ptr

pytestmark = pytest.mark.gpu

MAX_S, LDS_CELLS, BLOCK, MAX_BLOCKS = 64, 8192, 256, 64         # DSNT_SCORE_HIST_*, DSNT_PCKH_HIST_BLOCK / _MAX_BLOCKS
LOOKUP_STRIDE = 1024 * 256                                      # DSNT_SCORE_LOOKUP_MAX_BLOCKS x DSNT_SCORE_LOOKUP_BLOCK
SENTINEL = -7
NAN, INF = float('nan'), float('inf')


def edges_for(S):
    """S edges from 2^-10 up to below 1: the 20 half-octave edges of tests/score_ref.py, or thirds of an octave for more."""
    return EDGES20 if S == 20 else f32(2.0 ** (-10 + np.arange(S) / 3))


def thr_for(T):
    return {1: THR1, 3: THR3, 15: THR15}[T]


def _upload(args):
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
    assert [t.dtype for t in dev] == [torch.float32, torch.float32, torch.float64, torch.float64, torch.float32,
                                      torch.float64, torch.float32]
    return dev


def hist_dev(args, edges, thr, fill=0):
    """One `dsnt_score_hist` call into a table pre-filled with `fill`, with 8 guard cells behind it."""
    B, J = args[4].shape
    S, T = len(edges), len(thr)
    dev = _upload(args)
    cells = J * (S + 2) * (T + 1)
    table = torch.full((cells + 8,), SENTINEL, dtype=torch.int64, device='cuda')
    table[:cells] = fill
    call('dsnt_score_hist', *[ptr(t) for t in dev], (C.c_double * S)(*edges), S, (C.c_double * T)(*thr), T, ptr(table),
         B, J)
    assert (table[cells:] == SENTINEL).all().item()
    return table[:cells].view(J, S + 2, T + 1).cpu().numpy()


ONE_STRIDE = MAX_BLOCKS * BLOCK // 16 + 1                       # the smallest B with B * 16 past one grid stride
assert ONE_STRIDE == 1025 and 16 * 32 * 16 == LDS_CELLS < 16 * 33 * 16 and 64 * 22 * 16 > LDS_CELLS
CASES = [(1, 1, 20, 3), (37, 7, 20, 3), (16, 16, 20, 3), (70, 16, 20, 1), (ONE_STRIDE, 16, 20, 3),
         (40, 16, 30, 15),                                      # the largest LDS table
         (40, 16, 31, 15), (40, 64, 20, 15)]                    # the direct path


@pytest.mark.parametrize('B,J,S,T', CASES, ids=['%dx%d-S%d-T%d' % c for c in CASES])
def test_table_matches_restatement(B, J, S, T):
    args = score_ref.case(B, J, seed=B * 100 + J)
    edges, thr = edges_for(S), thr_for(T)
    assert score_ref.case_is_clear(args, thr)
    want = score_ref.restate(*args, edges, thr)
    valid = args[4] == 1
    if B * J >= 256 and S == 20:
        # the inputs exercise the table: many score rows in use, and a confidence that tracks the error
        at = int(np.flatnonzero(thr == 0.5)[0])
        hits, n = want[:, :21, :at + 1].sum((0, 2)), want[:, :21].sum((0, 2))            # the 21 scored rows (no score
        assert not want[:, 21].any()                                                     # of these inputs is NaN)
        lo, hi = hits[:16].sum() / n[:16].sum(), hits[16:].sum() / n[16:].sum()          # edge 16 is 2^-2
        print('B=%d J=%d: %d valid, %d score rows in use, PCKh@0.5 %.3f below a score of 0.25 and %.3f from there up'
              % (B, J, valid.sum(), (n > 0).sum(), lo, hi))
        # at least 12 of the 21 rows; the 16 x 16 case, the smallest here with its 121 valid joints, reaches 11 of them
        # under this generator and seed (tests/score_ref.case, restated on the CPU), so that one is held to 11
        assert (n > 0).sum() >= (11 if (B, J) == (16, 16) else 12) and lo < 0.4 and hi > 0.8
    table = hist_dev(args, edges, thr)
    assert np.array_equal(table, want), (B, J, S, T)
    assert table.sum() == valid.sum()
    # a transposed multiply and a shifted score fill other cells on these inputs: the comparison tells them apart
    if B * J >= 256:
        wrong_d = score_ref.restate(args[0], args[1], args[2].transpose(0, 2, 1), *args[3:], edges, thr)
        wrong_s = score_ref.restate(*args[:6], args[6] * np.float32(1.5), edges, thr)
        assert np.abs(wrong_d - want).sum() >= 10 and np.abs(wrong_s - want).sum() >= 10


def test_kernel_adds_and_never_stores():
    """A table that holds 7 in every cell comes back as 7 + the restatement, on the LDS path and on the direct one."""
    for B, J, S, T in ((16, 16, 20, 3), (40, 16, 31, 15)):
        args = score_ref.case(B, J, seed=B * 100 + J)
        edges, thr = edges_for(S), thr_for(T)
        assert score_ref.case_is_clear(args, thr)
        assert np.array_equal(hist_dev(args, edges, thr, fill=7), score_ref.restate(*args, edges, thr) + 7)


def _scores_only(scores):
    """One joint, one sample per score: pred == target (d = 0: column 0 of every table), mask 1."""
    n = len(scores)
    z = np.zeros((n, 1, 2), np.float32)
    return (z, z, np.tile(np.eye(2), (n, 1, 1)), np.zeros((n, 2)), np.ones((n, 1), np.float32), np.ones(n),
            np.asarray(scores, np.float32).reshape(n, 1))


def test_score_rows_by_hand():
    """A score on an edge belongs to the row above it, one ulp below to the row below; -inf is row 0, +inf row S, NaN row
    S + 1; -0.0 reaches an edge of 0 and the smallest denormals fall on either side of it; S = 1 and S = 64."""
    below = lambda v: np.nextafter(np.float32(v), np.float32(-INF))
    tiny = np.float32(1e-45)                                    # the smallest denormal
    assert tiny > 0 and float(below(0.25)) < 0.25
    hand = [
        (f32([0.0, 0.25, 1.0]), [0.25, below(0.25), INF, -INF, NAN, -0.0, 0.0, tiny, -tiny, 1.0, below(1.0), 0.5],
         [2, 1, 3, 0, 4, 1, 1, 1, 0, 3, 2, 2]),
        (f32([0.5]), [0.5, below(0.5), NAN, INF, -INF, 0.75], [1, 0, 2, 1, 0, 1]),
        (f32(np.arange(64)), [63.0, 62.5, 0.0, -1.0, INF, NAN, 7.0, below(7.0), 1e30], [64, 63, 1, 0, 64, 65, 8, 7, 64]),
    ]
    for edges, scores, rows in hand:
        S = len(edges)
        want = np.zeros((1, S + 2, 2), np.int64)
        np.add.at(want, (0, np.array(rows), 0), 1)
        args = _scores_only(scores)
        assert score_ref.row(args[6][:, 0], edges).tolist() == rows
        assert np.array_equal(score_ref.restate(*args, edges, THR1), want)
        assert np.array_equal(hist_dev(args, edges, THR1), want), (S, scores)


def test_non_finite_coordinates_and_masks():
    """The cases of tests/test_pckh_curve_gpu.py: NaN and inf coordinates under mask 0 change no cell, under mask 1 they
    count in column T; masks of 0.5 and 2 do not count, whatever their score; a zero head length sends every valid joint
    to column T.  Every score is 0.3, row 1 of the edges (0.25, 0.5, 0.75), but for a NaN score on joint 3 of sample 0."""
    bad = [((NAN, 0.0), (0.0, 0.0)), ((0.0, 0.0), (0.0, NAN)), ((INF, 0.0), (0.0, 0.0)), ((0.0, 0.0), (-INF, 0.0)),
           ((INF, INF), (INF, INF)), ((NAN, NAN), (NAN, NAN))]
    B, J, T = len(bad), 4, 3          # joint 0: bad under mask 0; joint 1: bad under mask 1; joints 2, 3: d = 0.5, 1
    edges = f32([0.25, 0.5, 0.75])
    pred, target = np.zeros((B, J, 2), np.float32), np.zeros((B, J, 2), np.float32)
    for n, (p, t) in enumerate(bad):
        pred[n, 0] = pred[n, 1] = p
        target[n, 0] = target[n, 1] = t
    pred[:, 2] = (3.0, 4.0)
    pred[:, 3] = (6.0, 8.0)
    mask = np.tile(np.array([0, 1, 1, 1], np.float32), (B, 1))
    mask[0, 0], mask[1, 0] = 0.5, 2
    score = np.full((B, J), 0.3, np.float32)
    score[0, 3], score[2, 0] = NAN, NAN                         # (the second under mask 0)
    m, b, head = np.tile(np.eye(2), (B, 1, 1)), np.zeros((B, 2)), np.full(B, 10.0)
    want = np.zeros((J, 5, T + 1), np.int64)
    want[1, 1, T] = want[2, 1, T - 1] = B
    want[3, 1, T], want[3, 4, T] = B - 1, 1
    args = (pred, target, m, b, mask, head, score)
    assert np.array_equal(score_ref.restate(*args, edges, THR3), want)
    assert np.array_equal(hist_dev(args, edges, THR3), want)
    head[:] = 0.0                                               # 5 / 0 = inf
    want[:] = 0
    want[1:3, 1, T] = B
    want[3, 1, T], want[3, 4, T] = B - 1, 1
    assert np.array_equal(score_ref.restate(*args, edges, THR3), want)
    assert np.array_equal(hist_dev(args, edges, THR3), want)


def test_marginal_is_the_pckh_histogram_bit_for_bit():
    """Summed over the score rows the table is `dsnt_pckh_hist`'s on the same device inputs: the same distance, the same
    column.  No margin is needed, so a fifth of the coordinates are made non-finite as well."""
    for B, J, S, T in ((16, 16, 20, 3), (300, 16, 20, 15), (40, 64, 20, 15), (40, 16, 31, 15)):
        args = list(score_ref.case(B, J, seed=7 * B + J))
        r = np.random.default_rng(B)
        args[0][r.random((B, J)) < 0.2] = (NAN, INF)
        edges, thr = edges_for(S), thr_for(T)
        table = hist_dev(args, edges, thr)
        dev = _upload(args)[:6]
        hist = torch.zeros(J, T + 1, dtype=torch.int64, device='cuda')
        call('dsnt_pckh_hist', *[ptr(t) for t in dev], (C.c_double * T)(*thr), T, ptr(hist), None, B, J)
        assert np.array_equal(table.sum(1), hist.cpu().numpy()), (B, J, S, T)
        assert table.sum() == (args[4] == 1).sum() and table[:, :, T].sum() > 0


def _lookup_dev(score, edges, values, per_joint, J):
    n, S = score.size, len(edges)
    s, v = torch.from_numpy(score).cuda(), torch.from_numpy(values).cuda()
    out = torch.full((n + 8,), float(SENTINEL), dtype=torch.float32, device='cuda')
    call('dsnt_score_lookup', ptr(s), (C.c_double * S)(*edges), S, ptr(v), per_joint, ptr(out), n, J)
    assert (out[n:] == SENTINEL).all().item()
    return out[:n].cpu().numpy()


@pytest.mark.parametrize('n', [1, 7, LOOKUP_STRIDE + 1])
@pytest.mark.parametrize('per_joint', [0, 1])
def test_lookup_matches_numpy(n, per_joint):
    J, S = 7, 20
    r = np.random.default_rng(n + per_joint)
    score = (2.0 ** r.uniform(-12, 1, n)).astype(np.float32)
    special = np.array([NAN, INF, -INF, 0.0, -0.0, EDGES20[0], EDGES20[19], np.nextafter(np.float32(EDGES20[5]), np.float32(0))],
                       np.float32)
    at = r.permutation(n)[:min(n, 64)]
    score[at] = special[np.arange(len(at)) % len(special)]
    if n == 1:
        score[0] = NAN
    values = r.uniform(0, 1, (J if per_joint else 1, S + 2)).astype(np.float32)
    values[0, 3] = values[-1, S + 1] = NAN
    rows = score_ref.row(score, EDGES20)
    want = values[np.arange(n) % J if per_joint else np.zeros(n, np.int64), rows]
    got = _lookup_dev(score, EDGES20, values, per_joint, J)
    assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True)
    assert n < 64 or (np.isnan(want).sum() > 0 and len(np.unique(rows)) == S + 2)
    if n % J == 0 or not per_joint:                             # ... and as score_ref.lookup states it, on [n / J, J]
        shaped = score.reshape(-1, J) if n % J == 0 else score.reshape(-1, 1)
        assert np.array_equal(score_ref.lookup(shaped, EDGES20, values, per_joint).reshape(-1), want, equal_nan=True)


# ------------------------------------------------------------------ the classes
def _batches(n=3, B=16, J=16, seed=40):
    out = []
    for k in range(n):
        args = score_ref.case(B, J, seed=seed + k)
        assert score_ref.case_is_clear(args, THR3)
        out.append(args)
    return out


def _feed(ev, args):
    pred, target, m, b, mask, head, score = [torch.from_numpy(a).cuda() for a in args]
    return ev.add_normalized(pred, target, mask, head, m, b, score)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_class_behaviour():
    from dsnt.evaluator import Reliability, ScoreCalibration
    batches = _batches(4)
    want = sum(score_ref.restate(*a, EDGES20, THR3) for a in batches)
    whole, first, second = (Reliability(EDGES20, [0.1, 0.2, 0.5]) for _ in range(3))
    for k, args in enumerate(batches):
        assert _feed(whole, args) is None
        _feed(first if k < 2 else second, args)
    assert whole.counts().dtype == torch.int64 and np.array_equal(whole.counts().numpy(), want)
    first.merge(second)
    assert torch.equal(first.counts(), whole.counts())
    assert np.array_equal(second.counts().numpy(), sum(score_ref.restate(*a, EDGES20, THR3) for a in batches[2:]))
    # the state loads into an object that never sees a GPU, and answers the same
    state = whole.state_dict()
    assert not state['table'].is_cuda and not state['score_edges'].is_cuda
    cpu = Reliability([0.5], thresholds=[0.3])
    cpu.load_state_dict(state)
    for name in ('total_mpii', 'ubody', 'all', 'lwrist', 3):
        for t in (0.1, 0.5):
            assert all(_same(a, b) for a, b in zip(cpu.accuracy(t, name), whole.accuracy(t, name)))
            ours, theirs = cpu.risk_coverage(t, name), whole.risk_coverage(t, name)
            assert all(_same(ours[k], theirs[k]) for k in theirs)
            assert cpu.operating_point(0.8, t, name) == whole.operating_point(0.8, t, name)
            assert _same(cpu.calibration(t, name).values, whole.calibration(t, name).values)
    assert _same(cpu.calibration(0.5).values, whole.calibration(0.5).values)
    # the readings say what the inputs were built to say: confident joints are kept first, and they are the better ones
    rc = whole.risk_coverage(0.5, 'all')
    assert rc['kept'][0] == want[:, :21].sum() == want.sum() and rc['coverage'][0] == 1.0
    assert (np.diff(rc['kept']) <= 0).all() and rc['pckh'][0] < 0.7 < np.nanmax(rc['pckh'])
    cut, coverage, pckh = whole.operating_point(0.85, 0.5, 'all')
    assert pckh >= 0.85 and 0.05 < coverage < 0.9 and cut in EDGES20
    # the calibration applied on the device is the table looked up on the host
    cal = whole.calibration(0.5)
    score = batches[0][6]
    p = cal(torch.from_numpy(score).cuda())
    assert p.dtype == torch.float32 and p.shape == score.shape
    assert _same(p.cpu().numpy(), score_ref.lookup(score, EDGES20, cal.values.numpy(), 1))
    shared = whole.calibration(0.5, 'all')
    cube = torch.from_numpy(score).cuda().view(2, 8, 16)
    assert _same(shared(cube).cpu().numpy().reshape(16, 16), score_ref.lookup(score, EDGES20, shared.values.numpy(), 0))
    again = ScoreCalibration([0.5], np.zeros((1, 3), np.float32))
    again.load_state_dict(cal.state_dict())
    assert torch.equal(again(cube.view(16, 16)), p) and again(torch.empty(0, 16, device='cuda')).shape == (0, 16)
    vals = cal.values.numpy()
    assert (np.diff(vals[:, :21], axis=1) >= 0).all() and vals[:, 20].min() > vals[:, 0].max()
    with pytest.raises(ValueError):
        _feed(Reliability(EDGES20, n_joints=7), batches[0])
    with pytest.raises(ValueError):
        whole.add_normalized(*[torch.from_numpy(a).cuda() for a in batches[0][:2]], None, None, None, None,
                             torch.zeros(16, 15, device='cuda'))
    whole.reset()
    assert not whole.counts().any().item()
    _feed(whole, batches[0])
    assert np.array_equal(whole.counts().numpy(), score_ref.restate(*batches[0], EDGES20, THR3))


def test_non_contiguous_scores_and_add():
    """`stats['peak']` is column 0 of a packed `[B, J, 7]` tensor; `add` supplies the identity transform."""
    from dsnt.evaluator import Reliability
    args = _batches(1)[0]
    pred, target, m, b, mask, head, score = [torch.from_numpy(a).cuda() for a in args]
    packed = torch.full((16, 16, 7), NAN, device='cuda')
    packed[..., 0] = score
    view = packed[..., 0]
    assert not view.is_contiguous()
    ev = Reliability(EDGES20, [0.1, 0.2, 0.5])
    ev.add_normalized(pred, target, mask, head, m, b, view)
    assert np.array_equal(ev.counts().numpy(), score_ref.restate(*args, EDGES20, THR3))
    ident = (np.tile(np.eye(2), (16, 1, 1)), np.zeros((16, 2)))
    flat = (args[0], args[1], *ident, args[4], args[5], args[6])
    assert score_ref.case_is_clear(flat, THR3)
    ev.reset()
    for _ in range(2):                                          # the second call takes the cached identity
        ev.add(pred, target, mask, head, view)
    assert np.array_equal(ev.counts().numpy(), 2 * score_ref.restate(*flat, EDGES20, THR3)) and len(ev._identity) == 1


def test_add_and_lookup_without_host_sync():
    """After the first call has set up the table, the identity and the uploaded values, `add_normalized`, `add` and
    `ScoreCalibration.__call__` enqueue and return."""
    from dsnt.evaluator import Reliability
    batches = _batches(2)
    dev = [[torch.from_numpy(a).cuda() for a in args] for args in batches]
    packed = torch.zeros(16, 16, 7, device='cuda')
    ev = Reliability(EDGES20, [0.1, 0.2, 0.5])
    _feed(ev, batches[0])
    cal = ev.calibration(0.5)
    ev.reset()
    out = []

    def step(k):
        pred, target, m, b, mask, head, score = dev[k]
        packed[..., 0] = score
        ev.add_normalized(pred, target, mask, head, m, b, packed[..., 0])
        ev.add(pred, target, mask, head, score)
        out.append(cal(packed[..., 0]))
    step(0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')                     # any synchronising call raises
    try:
        step(1)
        step(1)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    want = score_ref.restate(*batches[0], EDGES20, THR3) + 2 * score_ref.restate(*batches[1], EDGES20, THR3)
    ident = (np.tile(np.eye(2), (16, 1, 1)), np.zeros((16, 2)))
    for k in (0, 1, 1):
        a = batches[k]
        flat = (a[0], a[1], *ident, a[4], a[5], a[6])
        assert score_ref.case_is_clear(flat, THR3)
        want = want + score_ref.restate(*flat, EDGES20, THR3)
    assert np.array_equal(ev.counts().numpy(), want)
    assert _same(out[2].cpu().numpy(), score_ref.lookup(batches[1][6], EDGES20, cal.values.numpy(), 1))


def test_refusals_launch_nothing():
    """Bad S, T, edges, thresholds, a null pointer and an empty batch are refused on the host with DSNT_ERR_ARG: the table
    and the lookup's output are unchanged, and both then take a call that is in order."""
    hist, look = _lib.fn('dsnt_score_hist'), _lib.fn('dsnt_score_lookup')
    B, J, S, T = 4, 3, 20, 3
    args = score_ref.case(B, J, seed=9)
    assert score_ref.case_is_clear(args, THR3)
    dev = _upload(args)
    cells = J * (S + 2) * (T + 1)
    table = torch.full((cells + 8,), SENTINEL, dtype=torch.int64, device='cuda')
    values = torch.rand(J, S + 2, device='cuda')
    out = torch.full((B * J + 8,), float(SENTINEL), device='cuda')
    stream = _lib.stream_ptr()

    def arr(v):
        return (C.c_double * max(len(v), 1))(*v)

    def rc_hist(edges=EDGES20, thr=THR3, S=None, T=None, table_ptr=ptr(table), B=B, J=J):
        return hist(*[ptr(t) for t in dev], arr(edges), len(edges) if S is None else S, arr(thr),
                    len(thr) if T is None else T, table_ptr, B, J, stream)

    def rc_look(edges=EDGES20, S=None, out_ptr=ptr(out), n=B * J, J=J, per_joint=1):
        return look(ptr(dev[6]), arr(edges), len(edges) if S is None else S, ptr(values), per_joint, out_ptr, n, J, stream)
    bad = [rc_hist(S=0), rc_hist(edges=np.arange(65.0)), rc_hist(edges=[0.2, 0.1]), rc_hist(edges=[0.1, 0.1]),
           rc_hist(edges=[0.1, NAN]), rc_hist(edges=[0.1, INF]), rc_hist(T=0), rc_hist(thr=np.arange(65.0)),
           rc_hist(thr=[0.2, 0.1]), rc_hist(thr=[NAN]), rc_hist(table_ptr=None), rc_hist(B=0), rc_hist(J=0),
           hist(*[ptr(t) for t in dev], None, 1, arr(THR3), 3, ptr(table), B, J, stream),
           rc_look(S=0), rc_look(S=65), rc_look(edges=[0.2, 0.1]), rc_look(edges=[NAN]), rc_look(out_ptr=None),
           rc_look(n=0), rc_look(J=0), rc_look(per_joint=2)]
    assert bad == [3] * len(bad), bad
    assert b'dsnt_score_lookup: bad argument' == _lib.fn('dsnt_last_error')()
    torch.cuda.synchronize()
    assert (table == SENTINEL).all().item() and (out == SENTINEL).all().item()
    assert rc_hist() == 0 and rc_look() == 0
    torch.cuda.synchronize()
    got = table[:cells].view(J, S + 2, T + 1).cpu().numpy() - SENTINEL
    assert np.array_equal(got, score_ref.restate(*args, EDGES20, THR3)) and (table[cells:] == SENTINEL).all().item()
    assert _same(out[:B * J].cpu().numpy().reshape(B, J), score_ref.lookup(args[6], EDGES20, values.cpu().numpy(), 1))
    assert (out[B * J:] == SENTINEL).all().item()


# ------------------------------------------------------------------ end to end
def test_predict_feeds_reliability_and_takes_a_calibration():
    """hg1 + DSNT with synthetic weights, batch 4: `predict(return_stats=True)` feeds `Reliability.add_normalized` with
    `stats['peak']` as it comes (a view), the counts equal the restatement on the returned tensors, and
    `predict(calibration=cal)` returns the same coordinates and the same six statistics, plus `p_correct`."""
    from dsnt import inference, synthetic
    from dsnt.evaluator import Reliability
    from dsnt.model import build_mpii_pose_model
    B, J, size = 4, 16, 128
    model = build_mpii_pose_model(base='hg1', output_strat='dsnt', reg='js')
    synthetic.fill_state_dict(model, seed=0)
    model.cuda().train()
    for mod in model.modules():                                 # running statistics of one batch, as tests/test_stats_gpu.py
        if isinstance(mod, torch.nn.BatchNorm2d):               # sets them: without, the synthetic maps saturate
            mod.momentum = 1.0
    with torch.no_grad():
        model(synthetic.batch(2, size=size, seed=5, mask_p=1.0)[0].cuda())
    x, _, _ = synthetic.batch(B, size=size, seed=21, mask_p=1.0)
    g = torch.Generator().manual_seed(3)
    tm = (torch.eye(2, dtype=torch.float64) * 140 + 20 * torch.rand(B, 2, 2, generator=g, dtype=torch.float64)).cuda()
    tb = (200 * torch.rand(B, 1, 2, generator=g, dtype=torch.float64)).cuda()
    img, norm, st = inference.predict(model, x.cuda(), tm, tb, return_normalized=True, return_stats=True)
    r = np.random.default_rng(5)
    target = (norm.cpu().numpy() + r.normal(0, 0.25, (B, J, 2))).astype(np.float32)
    mask = r.choice(np.array([0, 1, 1, 1], np.float32), (B, J))
    head = r.uniform(40, 120, B)
    peak = st['peak'].cpu().numpy()
    seen = np.unique(peak)                                      # edges ON scores the model gave, whatever they are: up
    edges = f32(seen[1:][::max(1, (len(seen) - 1) // 4)][:4])   # to four of them, each the lowest score of its row
    print('%d distinct peaks from %g to %g, edges %s' % (len(seen), seen[0], seen[-1], edges))
    assert len(seen) >= 3 and np.isin(edges.astype(np.float32), peak).all()
    host = (norm.cpu().numpy(), target, tm.cpu().numpy(), tb.cpu().numpy().reshape(B, 2), mask, head, peak)
    assert score_ref.case_is_clear(host, THR3)
    ev = Reliability(edges, [0.1, 0.2, 0.5])
    ev.add_normalized(norm, torch.from_numpy(target), torch.from_numpy(mask), torch.from_numpy(head), tm, tb, st['peak'])
    want = score_ref.restate(*host, edges, THR3)
    assert np.array_equal(ev.counts().numpy(), want) and (want.sum((0, 2)) > 0).sum() >= 2 and want.sum() == mask.sum()
    cal = ev.calibration(0.5, 'all')
    img1, norm1, st1 = inference.predict(model, x.cuda(), tm, tb, return_normalized=True, return_stats=True,
                                         calibration=cal)
    assert torch.equal(img1, img) and torch.equal(norm1, norm)
    assert set(st1) == set(st) | {'p_correct'} and len(st) == 6
    assert all(torch.equal(st1[k], st[k]) for k in st)
    assert st1['p_correct'].dtype == torch.float32 and st1['p_correct'].shape == (B, J)
    assert torch.equal(st1['p_correct'], cal(st['peak']))
    assert _same(st1['p_correct'].cpu().numpy(), score_ref.lookup(peak, edges, cal.values.numpy(), 0))
    # without return_stats there is nowhere to put it
    with pytest.raises(ValueError):
        inference.predict(model, x.cuda(), tm, tb, calibration=cal)
    # predict_dataset carries it through its batches
    data = [{'input': x[i], 'transform_m': tm[i].cpu(), 'transform_b': tb[i].cpu()} for i in range(B)]
    preds, std = inference.predict_dataset(model, data, batch_size=3, return_stats=True, calibration=cal)
    assert set(std) == set(st1) and not std['p_correct'].is_cuda and std['p_correct'].shape == (B, J)
    assert _same(std['p_correct'].numpy(), score_ref.lookup(std['peak'].numpy(), edges, cal.values.numpy(), 0))


def test_predict_boxes_gives_a_sample_without_a_crop_nan():
    """The box cases of tests/test_stats_gpu.py with a calibration of the spread (lower is better, `stat_score` on the
    device): `p_correct` is the lookup of `sqrt(trace(cov_image))` where there is a crop and NaN where there is none,
    though no value of the calibration is NaN."""
    import golden_util
    from dsnt import inference, synthetic
    from dsnt.data import ImagePool
    from dsnt.evaluator import ScoreCalibration, stat_score
    from dsnt.model import build_mpii_pose_model
    model = build_mpii_pose_model(base='hg1', output_strat='dsnt', reg='js')
    synthetic.fill_state_dict(model, seed=0)
    model.cuda().eval()
    g = golden_util.load('crop')
    n = sum(1 for k in g.files if k.startswith('img.'))
    pool = ImagePool.from_images([g['img.%d' % k] for k in range(n)], chunk_bytes=1 << 16)
    names = [str(k) for k in g['names'] if int(g[str(k) + '.R']) == 96]
    idx = torch.tensor([int(g[k + '.image']) for k in names], device='cuda')
    mat = torch.from_numpy(np.stack([g[k + '.matrix'] for k in names])).cuda()
    idx[2] = len(pool)                                          # no such image: no crop
    edges = f32([1.0, 4.0, 16.0, 64.0])                         # pixels
    values = np.array([[0.9, 0.7, 0.5, 0.3, 0.1, 0.05]], np.float32)
    cal = ScoreCalibration(edges, values, score='spread')
    norm_stats = (synthetic.IMAGE_MEAN, (0.25, 0.26, 0.27))
    img, st = inference.predict_boxes(model, pool, idx, mat, *norm_stats, crop_size=96, return_stats=True,
                                      calibration=cal)
    ok = torch.ones(idx.numel(), dtype=torch.bool, device='cuda')
    ok[2] = False
    p = st['p_correct']
    assert p.shape == st['peak'].shape and torch.isnan(p[2]).all().item() and torch.isfinite(p[ok]).all().item()
    spread = stat_score(st, 'spread')
    assert spread.dtype == torch.float32 and torch.isnan(spread[2]).all().item()
    want = score_ref.lookup(spread.cpu().numpy(), edges, values, 0)
    assert _same(p[ok].cpu().numpy(), want[ok.cpu().numpy()]) and (want[2] == np.float32(0.05)).all()
    cov = st['cov_image'].cpu().numpy()
    # one fp64 add, one fp64 square root, one rounding to fp32: two fp32 ulps cover a square root that is not exact
    ref = np.sqrt(cov[..., 0, 0] + cov[..., 1, 1])
    assert (np.abs(spread.cpu().numpy()[ok.cpu().numpy()] - ref[ok.cpu().numpy()]) <= 2.0 ** -22 * ref[ok.cpu().numpy()]).all()
