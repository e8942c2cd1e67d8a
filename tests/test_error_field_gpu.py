"""The misprediction field (`error_field_kernel`, csrc/pckh.hip, through `dsnt_error_field`) and
`dsnt.evaluator.ErrorField` against the numpy restatement of tests/error_field_ref.py.

All five planes must equal the restatement exactly, the fp64 sums included: one lane owns each cell and adds its samples
in ascending `n`, which is the restatement's loop.  The only expression that may round differently on the device is the
distance inside `pckh_distance` (FMA contraction), so every case first checks on the CPU that no counted joint lies
within 1e-9 relative of the threshold; the offsets `(double)p - (double)t` and their sums are single fp64 operations.

Shapes are chosen around DSNT_ERROR_FIELD_BLOCK = 256 (include/dsnt_hip.h): the samples of a joint are walked in chunks
of 256, and a lane owns the cells `l, l + 256, ...`, more than one from 17 x 17 cells on.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import error_field_ref as ref
from dsnt import _lib
from dsnt._lib import call, ptr

pytestmark = pytest.mark.gpu

SENTINEL = -7
THR = 0.5
GENERATORS = {'spread': ref.spread, 'crowded': ref.crowded, 'wide': ref.wide}


def new_tables(J, bins, counts=0, sums=0.0):
    """Device tables pre-filled with `counts` and `sums`, each with 8 sentinel guard cells behind it."""
    cells = J * bins * bins
    c = torch.full((3 * cells + 8,), SENTINEL, dtype=torch.int64, device='cuda')
    s = torch.full((2 * cells + 8,), float(SENTINEL), dtype=torch.float64, device='cuda')
    c[:3 * cells] = counts
    s[:2 * cells] = sums
    return c, s


def launch(args, bins, tables, thr=THR):
    """One `dsnt_error_field` call on numpy (pred, target, m, b, mask, head) into `tables`."""
    B, J = args[4].shape
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
    assert dev[0].dtype == dev[1].dtype == dev[4].dtype == torch.float32 and dev[2].dtype == dev[5].dtype == torch.float64
    edges = ref.edges_of(bins)
    call('dsnt_error_field', *[ptr(t) for t in dev], thr, (C.c_double * (bins + 1))(*edges), bins, ptr(tables[0]),
         ptr(tables[1]), B, J)


def read(tables, J, bins):
    """(total, miss, miss_finite, sum_x, sum_y) as numpy [J, bins, bins]; the guard cells must be intact."""
    cells = J * bins * bins
    c, s = tables[0].cpu(), tables[1].cpu()
    assert (c[3 * cells:] == SENTINEL).all().item() and (s[2 * cells:] == SENTINEL).all().item()
    c, s = c[:3 * cells].view(3, J, bins, bins).numpy(), s[:2 * cells].view(2, J, bins, bins).numpy()
    return c[0], c[1], c[2], s[0], s[1]


def field_dev(args, bins, counts=0, sums=0.0):
    tables = new_tables(args[4].shape[1], bins, counts, sums)
    launch(args, bins, tables)
    return read(tables, args[4].shape[1], bins)


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == len(want) == 5


def clear_of_threshold(args, bins, thr=THR):
    """No counted joint within 1e-9 relative of the threshold: contraction inside `pckh_distance` cannot flip a decision."""
    pred, target, m, b, mask, head = args
    d = ref.distance(pred, target, m, b, head)[ref.in_frame(target, mask, ref.edges_of(bins))]
    d = d[np.isfinite(d)]
    return bool((np.abs(d - thr) > 1e-9 * thr).all())


def differing_sums(a, b):
    return int((a[3] != b[3]).sum() + (a[4] != b[4]).sum())


def slices(args, lo, hi):
    return tuple(a[lo:hi] for a in args)


CASES = [(1, 1, 1, 'spread'), (37, 7, 5, 'spread'), (16, 16, 8, 'spread'),
         (257, 3, 8, 'crowded'),                               # one record in the second chunk
         (512, 2, 8, 'crowded'),                               # a full last chunk
         (70, 2, 32, 'spread'),                                # 1024 cells: four per lane
         (40, 17, 8, 'spread'), (257, 3, 8, 'wide')]


@pytest.mark.parametrize('B,J,bins,gen', CASES, ids=['%dx%d-b%d-%s' % c for c in CASES])
def test_tables_match_restatement(B, J, bins, gen):
    args = GENERATORS[gen](B, J)
    edges = ref.edges_of(bins)
    want = ref.restate(*args, THR, edges)
    assert clear_of_threshold(args, bins)
    valid, framed = int((args[4] == 1).sum()), int(ref.in_frame(args[1], args[4], edges).sum())
    print('B=%d J=%d bins=%d %s: %d valid, %d in frame, %d misses, %d of them finite'
          % (B, J, bins, gen, valid, framed, want[1].sum(), want[2].sum()))
    assert want[0].sum() == framed
    if gen == 'spread' and B * J >= 256:                       # misses, non-misses and targets outside the frame
        assert 0 < want[1].sum() < framed < valid
    if gen == 'crowded':
        assert framed == valid and 0 < want[1].sum() < framed and want[0].max() >= 8
    if gen == 'wide':
        # the order of the adds is under test: the same samples in descending order, or as two halves summed afterwards,
        # give other sums (on the other generators fp32 differences add exactly in fp64, and these numbers are 0)
        down = ref.restate(*args, THR, edges, order=range(B - 1, -1, -1))
        halves = [ref.restate(*slices(args, lo, hi), THR, edges) for lo, hi in ((0, B // 2), (B // 2, B))]
        halves = [x + y for x, y in zip(*halves)]
        print('sums that differ: %d descending, %d as two halves' % (differing_sums(want, down), differing_sums(want, halves)))
        assert differing_sums(want, down) >= 5 and differing_sums(want, halves) >= 5
        assert all(np.array_equal(a, b) for a, b in zip(down[:3], want[:3]))      # (the counts do not depend on it)
    got = field_dev(args, bins)
    for name, g, w in zip(('total', 'miss', 'miss_finite', 'sum_x', 'sum_y'), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, B, J, bins, gen)


def test_batches_and_repeats_are_bit_identical():
    """The wide case as batches of 100, 100 and 57 into one pair of tables: the tables of one call with all 257, which two
    runs of that call also agree on."""
    B, J, bins = 257, 3, 8
    args = ref.wide(B, J)
    whole = field_dev(args, bins)
    assert same(field_dev(args, bins), whole)
    tables = new_tables(J, bins)
    for lo, hi in ((0, 100), (100, 200), (200, 257)):
        launch(slices(args, lo, hi), bins, tables)
    assert same(read(tables, J, bins), whole)
    assert same(whole, ref.restate(*args, THR, ref.edges_of(bins)))


def test_kernel_adds_and_never_stores():
    """Tables that hold 7 and 0.5 in every cell come back as the restatement started from those values (for the sums that
    is not the restatement plus 0.5: the first add rounds differently), with one cell per lane and with four."""
    for B, J, bins, gen in ((257, 3, 8, 'wide'), (70, 2, 32, 'spread')):
        args = GENERATORS[gen](B, J)
        assert clear_of_threshold(args, bins)
        start = tuple(np.full((J, bins, bins), v, t) for v, t in ((7, np.int64),) * 3 + ((0.5, np.float64),) * 2)
        want = ref.restate(*args, THR, ref.edges_of(bins), start=start)
        assert (want[0] - 7).sum() > 0 and (want[3] != 0.5).any()
        assert same(field_dev(args, bins, counts=7, sums=0.5), want)


def _identity(B):
    return np.tile(np.eye(2), (B, 1, 1)), np.zeros((B, 2))


def _through_class(rows, bins=8):
    """rows of (target xy, pred xy, mask, head), one joint, identity transform -> the five planes [bins, bins], after they
    were checked against the restatement."""
    from dsnt.evaluator import ErrorField
    B = len(rows)
    target = np.array([r[0] for r in rows], np.float32).reshape(B, 1, 2)
    pred = np.array([r[1] for r in rows], np.float32).reshape(B, 1, 2)
    mask = np.array([r[2] for r in rows], np.float32).reshape(B, 1)
    head = np.array([r[3] for r in rows], np.float64)
    m, b = _identity(B)
    ev = ErrorField(bins=bins, n_joints=1)
    ev.add_normalized(*[torch.from_numpy(a).cuda() for a in (pred, target, mask, head, m, b)])
    counts, sums = ev.tables()
    got = tuple(x.numpy() for x in (counts[0], counts[1], counts[2], sums[0], sums[1]))
    assert same(got, ref.restate(pred, target, m, b, mask, head, THR, ev.edges))
    assert np.array_equal(ev.totals(0), got[0][0]) and np.array_equal(ev.misses(), got[1][0])
    return tuple(g[0] for g in got)


def test_edge_values_through_the_class():
    nan, inf = float('nan'), float('inf')
    bins, edges = 8, ref.edges_of(8)
    f32 = np.float32
    # a target on every edge (x with y = 0.1, then y with x = 0.1), predicted exactly: e_k opens cell k, the last edge is closed
    on_x = _through_class([((e, 0.1), (e, 0.1), 1, 1.0) for e in edges])
    on_y = _through_class([((0.1, e), (0.1, e), 1, 1.0) for e in edges])
    want = np.zeros((bins, bins), np.int64)
    want[4, :] = 1
    want[4, bins - 1] = 2
    assert np.array_equal(on_x[0], want) and np.array_equal(on_y[0], want.T)
    assert not on_x[1].any() and not on_y[1].any() and not on_x[3].any()
    # the four corners and the centre of the frame
    corners = _through_class([((x, y), (x, y), 1, 1.0) for x, y in ((-1, -1), (1, -1), (-1, 1), (1, 1), (0, 0))])
    want[:] = 0
    want[0, 0] = want[0, 7] = want[7, 0] = want[7, 7] = want[4, 4] = 1
    assert np.array_equal(corners[0], want)
    # left out: one fp32 ulp beyond -1 or 1 on either axis, a NaN or inf target, masks other than 1
    below, above = np.nextafter(f32(-1), f32(-2)), np.nextafter(f32(1), f32(2))
    out = _through_class([((below, 0), (0, 0), 1, 1.0), ((above, 0), (0, 0), 1, 1.0), ((0, below), (0, 0), 1, 1.0),
                          ((0, above), (0, 0), 1, 1.0), ((nan, 0), (0, 0), 1, 1.0), ((0, nan), (0, 0), 1, 1.0),
                          ((inf, 0), (0, 0), 1, 1.0), ((0, -inf), (0, 0), 1, 1.0), ((nan, nan), (nan, nan), 1, 1.0),
                          ((0, 0), (5, 5), 0, 1.0), ((0, 0), (5, 5), 0.5, 1.0), ((0, 0), (5, 5), 2, 1.0),
                          ((nan, nan), (nan, nan), 0, 1.0)])
    assert not any(plane.any() for plane in out)
    # one fp32 ulp inside the frame: the outermost cells
    inside = _through_class([((np.nextafter(f32(-1), f32(0)), np.nextafter(f32(1), f32(0))), (0, 0), 1, 100.0)])
    assert inside[0][7, 0] == 1 and inside[0].sum() == 1 and not inside[1].any()
    # NaN and inf predictions: a miss that is counted and kept out of the sums, beside a finite miss in the same cell
    bad = _through_class([((0.1, 0.1), (1.1, 0.35), 1, 1.0), ((0.1, 0.1), (nan, 0.1), 1, 1.0), ((0.1, 0.1), (0.1, inf), 1, 1.0),
                          ((0.1, 0.1), (-inf, nan), 1, 1.0), ((0.1, 0.1), (0.1, 0.1), 1, 1.0)])
    assert bad[0][4, 4] == 5 and bad[1][4, 4] == 4 and bad[2][4, 4] == 1
    assert bad[3][4, 4] == float(f32(1.1)) - float(f32(0.1)) and bad[4][4, 4] == float(f32(0.35)) - float(f32(0.1))
    assert sum(int(p.astype(bool).sum()) for p in bad) == 5      # nothing outside that cell
    # head length 0: inf (or 0 / 0 = NaN where the prediction is exact), a miss either way
    zero = _through_class([((0.25, 0.5), (0.375, 0.5), 1, 0.0), ((0.25, 0.5), (0.25, 0.5), 1, 0.0)])
    assert zero[0][6, 5] == 2 and zero[1][6, 5] == 2 and zero[2][6, 5] == 2 and zero[3][6, 5] == 0.125 and zero[4][6, 5] == 0.0
    # d == threshold exactly is a hit (|0.75 - 0.25| / 1 = 0.5); one ulp less head length and it is a miss
    exact = _through_class([((0.25, 0.5), (0.75, 0.5), 1, 1.0)])
    assert exact[0][6, 5] == 1 and not exact[1].any() and not exact[3].any()
    over = _through_class([((0.25, 0.5), (0.75, 0.5), 1, np.nextafter(1.0, 0.0))])
    assert over[0][6, 5] == 1 and over[1][6, 5] == 1 and over[2][6, 5] == 1 and over[3][6, 5] == 0.5 and over[4][6, 5] == 0.0


def _feed(ev, args):
    pred, target, m, b, mask, head = [torch.from_numpy(a).cuda() for a in args]
    return ev.add_normalized(pred, target, mask, head, m, b)


def _batches(n=3, B=16, J=16, seed=60):
    out = [ref.crowded(B, J, seed=seed + k) for k in range(n)]
    assert all(clear_of_threshold(a, 8) for a in out)
    return out


def test_misses_are_the_joints_pckh_does_not_hit():
    """Three batches with every target in frame into `ErrorField` and `PCKhEvaluator(0.5)`: for every joint and group the
    field holds the meter's count, and its misses are the meter's count less its hits."""
    from dsnt.evaluator import ErrorField, PCKhEvaluator
    field, meter = ErrorField(), PCKhEvaluator(0.5)
    for args in _batches():
        assert ref.in_frame(args[1], args[4], field.edges).sum() == (args[4] == 1).sum()
        _feed(field, args)
        _feed(meter, args)
    for name in PCKhEvaluator.JOINT_NAMES + list(PCKhEvaluator.JOINT_GROUPS):
        count, hits = int(meter.meters[name].count), int(meter.meters[name].hits)
        assert field.totals(name).sum() == count and field.misses(name).sum() == count - hits, name
        assert 0 < hits < count
    for j, name in enumerate(PCKhEvaluator.JOINT_NAMES):
        assert np.array_equal(field.totals(j), field.totals(name))


def test_refusals_launch_nothing():
    """Null pointers, an empty batch, bins outside 1..32 and edges that are not finite or not ascending are refused on the
    host with DSNT_ERR_ARG and the entry's name; the tables keep their sentinels, and then take a call that is in order."""
    fn = _lib.fn('dsnt_error_field')
    B, J, bins = 20, 3, 4
    args = ref.spread(B, J)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
    tables = new_tables(J, bins, SENTINEL, float(SENTINEL))
    stream = _lib.stream_ptr()
    good = list(ref.edges_of(bins))

    def rc(edges=good, nbins=None, ptrs=None, counts=ptr(tables[0]), sums=ptr(tables[1]), B=B, J=J):
        arr = (C.c_double * max(len(edges), 1))(*edges) if edges is not None else None
        nbins = (len(edges) - 1 if edges is not None else bins) if nbins is None else nbins
        got = fn(*(ptrs or [ptr(t) for t in dev]), THR, arr, nbins, counts, sums, B, J, stream)
        assert got == 0 or _lib.fn('dsnt_last_error')().startswith(b'dsnt_error_field: ')
        return got
    nan, inf = float('nan'), float('inf')
    bad = [rc(nbins=0), rc(nbins=-1), rc(list(np.linspace(-1, 1, 34))), rc([1, -1]), rc([-1, 0, 0, 1]), rc([-1, 0.5, 0, 1]),
           rc([-1, nan, 1]), rc([nan, 1]), rc([-1, inf]), rc([-inf, 1]), rc(None), rc(counts=None), rc(sums=None),
           rc(B=0), rc(J=0), rc(B=-4)]
    bad += [rc(ptrs=[None if k == q else ptr(t) for q, t in enumerate(dev)]) for k in range(6)]
    assert bad == [3] * len(bad), bad
    torch.cuda.synchronize()
    assert (tables[0] == SENTINEL).all().item() and (tables[1] == SENTINEL).all().item()
    assert rc() == 0
    assert clear_of_threshold(args, bins)
    start = tuple(np.full((J, bins, bins), SENTINEL, t) for t in (np.int64,) * 3 + (np.float64,) * 2)
    assert same(read(tables, J, bins), ref.restate(*args, THR, ref.edges_of(bins), start=start))


def test_add_without_host_sync():
    """After the first call has allocated the tables, `add_normalized` enqueues and returns."""
    from dsnt.evaluator import ErrorField
    batches = _batches(2)
    dev = [[torch.from_numpy(a).cuda() for a in args] for args in batches]
    ev = ErrorField()

    def step(k):
        pred, target, m, b, mask, head = dev[k]
        assert ev.add_normalized(pred, target, mask, head, m, b) is None
    step(0)                                         # first call: the tables are set up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')         # any synchronising call raises
    try:
        step(1)
        step(1)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    want = ref.restate(*batches[0], THR, ev.edges)
    for _ in range(2):
        want = ref.restate(*batches[1], THR, ev.edges, start=want)
    counts, sums = ev.tables()
    assert same((counts[0].numpy(), counts[1].numpy(), counts[2].numpy(), sums[0].numpy(), sums[1].numpy()), want)


def test_class_behaviour():
    from dsnt.evaluator import ErrorField
    batches = _batches(4)
    edges = ref.edges_of(8)
    want = None
    whole, first, second = ErrorField(), ErrorField(), ErrorField()
    for k, args in enumerate(batches):
        want = ref.restate(*args, THR, edges, start=want)
        _feed(whole, args)
        _feed(first if k < 2 else second, args)
    counts, sums = whole.tables()
    assert counts.dtype == torch.int64 and sums.dtype == torch.float64 and not counts.is_cuda and not sums.is_cuda
    assert np.array_equal(counts.numpy(), np.stack(want[:3])) and np.array_equal(sums.numpy(), np.stack(want[3:]))
    # two halves merged: the counts of the whole, and its sums but for the order of the last add
    first.merge(second)
    assert torch.equal(first.tables()[0], counts)
    assert np.allclose(first.tables()[1].numpy(), sums.numpy(), rtol=1e-12, atol=0.0)
    for name in ('all', 'ubody', 'lwrist', 3):
        assert np.array_equal(first.totals(name), whole.totals(name)) and np.array_equal(first.misses(name), whole.misses(name))
        assert np.array_equal(first.miss_rate(name), whole.miss_rate(name))
        assert np.allclose(first.mean_offset(name), whole.mean_offset(name), rtol=1e-12, atol=0.0, equal_nan=True)
    # the readings, from the restatement
    rate = whole.miss_rate('all')
    with np.errstate(divide='ignore', invalid='ignore'):
        assert np.array_equal(rate, np.nan_to_num(want[1].sum(0) / want[0].sum(0))) and 0 < rate.max() <= 1
    X, Y, U, V, Cc = whole.quiver()
    assert X.shape == (64,) and (np.diff(Cc) >= 0).all() and np.isfinite(U).sum() == (want[2].sum(0) > 0).sum()
    # the state loads into an object that never sees a GPU, and answers the same
    cpu = ErrorField()
    cpu.load_state_dict(whole.state_dict())
    assert np.array_equal(cpu.mean_offset('total_mpii'), whole.mean_offset('total_mpii'), equal_nan=True)
    with pytest.raises(ValueError):
        whole.merge(ErrorField(bins=5))
    with pytest.raises(ValueError):
        _feed(ErrorField(n_joints=7), batches[0])
    # reset zeroes the tables, and the field counts again from there
    whole.reset()
    assert not whole.tables()[0].any().item() and not whole.tables()[1].any().item()
    _feed(whole, batches[0])
    counts, sums = whole.tables()
    again = ref.restate(*batches[0], THR, edges)
    assert np.array_equal(counts.numpy(), np.stack(again[:3])) and np.array_equal(sums.numpy(), np.stack(again[3:]))


def test_seven_unnamed_joints_on_five_bins():
    from dsnt.evaluator import ErrorField
    args = ref.spread(37, 7)
    assert clear_of_threshold(args, 5)
    ev = ErrorField(bins=5, n_joints=7)
    _feed(ev, args)
    want = ref.restate(*args, THR, ref.edges_of(5))
    counts, sums = ev.tables()
    assert np.array_equal(counts.numpy(), np.stack(want[:3])) and np.array_equal(sums.numpy(), np.stack(want[3:]))
    assert np.array_equal(ev.totals(), want[0].sum(0)) and np.array_equal(ev.misses(6), want[1][6]) and want[1].sum() > 0
    assert ev.mean_offset().shape == (5, 5, 2) and len(ev.quiver()[0]) == 25
    with pytest.raises(KeyError):
        ev.totals('total_mpii')
    with pytest.raises(KeyError):
        ev.totals(7)
