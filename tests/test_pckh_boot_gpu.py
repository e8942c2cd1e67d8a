"""`dsnt_pckh_boot` (csrc/pckh.hip) and `dsnt.evaluator.PCKhBootstrap` on the device against tests/boot_ref.py.

The table is integer and must equal the restatement exactly (`np.array_equal`).  The expected column of every joint is
taken from the device's own fp64 distance, the `dist` output of a `dsnt_pckh_hist` call on the same inputs, binned in
numpy: the weights are what is under test here, and no distance has to keep clear of a threshold.  That copy 0 is
`dsnt_pckh_hist`'s table is checked on its own.  The table is pre-filled (the kernel only adds) and carries guard cells.

Shapes sit around the constants of include/dsnt_hip.h: a workgroup owns min(CHUNK, LDS_CELLS // (J * (T + 1))) copies and
walks B * J in spans of SPAN joints; at most MAX_CHUNK_BLOCKS x MAX_SPAN_BLOCKS workgroups stride over chunks and spans;
J * (T + 1) <= LDS_CELLS selects the LDS path.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import boot_ref
import score_ref
from dsnt import evaluator
from dsnt._lib import call, ptr

pytestmark = pytest.mark.gpu

M = boot_ref.header_macros()
LDS_CELLS, CHUNK, SPAN, CHUNK_BLOCKS, SPAN_BLOCKS = (M['LDS_CELLS'], M['CHUNK'], M['SPAN'], M['MAX_CHUNK_BLOCKS'],
                                                     M['MAX_SPAN_BLOCKS'])
SENTINEL, FILL = -7, 5
THR1, THR3 = score_ref.THR1, score_ref.THR3
DEFAULT = score_ref.f32(np.arange(51) / 100)
T64 = score_ref.f32(np.arange(1, 65) / 128)
T63 = T64[1:]
assert 64 * (len(T63) + 1) == LDS_CELLS < 64 * (len(T64) + 1)      # J = 64: the largest LDS table, and the direct path
assert LDS_CELLS // (16 * 2) >= CHUNK and LDS_CELLS // (7 * 52) == 11 and LDS_CELLS // (16 * 52) == 4


def ids_for(B, kind='mixed', seed=0):
    """int64 [B], all different.  'mixed': shuffled and non-contiguous, a third of them above 2^32 and a third negative."""
    if kind == 'range':
        return np.arange(B, dtype=np.int64)
    r = np.random.default_rng(1000 + seed)
    ids = r.permutation(7 * B + 11)[:B].astype(np.int64) * 3 + 1
    ids[1::3] += r.integers(1, 2 ** 30, len(ids[1::3])) << 32
    ids[2::3] = -ids[2::3] - (r.integers(0, 2 ** 31, len(ids[2::3])) << 32)
    assert len(set(ids.tolist())) == B
    return ids


def case(B, J, seed):
    """`score_ref.case` without the score, with a NaN prediction and a zero head length where there is room for them."""
    pred, target, m, b, mask, head, _ = score_ref.case(B, J, seed)
    if B >= 3:
        pred[1, 0, 0], mask[1, 0] = np.nan, 1
        head[2], mask[2, J - 1] = 0.0, 1
    return pred, target, m, b, mask, head


def on_device(args):
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
    assert dev[0].dtype == dev[1].dtype == dev[4].dtype == torch.float32 and dev[2].dtype == dev[5].dtype == torch.float64
    return dev


def hist_dev(dev, thr, B, J):
    """(table [J, T + 1], dist [B, J]) of one `dsnt_pckh_hist` call."""
    T = len(thr)
    table = torch.zeros(J, T + 1, dtype=torch.int64, device='cuda')
    dist = torch.empty(B, J, dtype=torch.float64, device='cuda')
    call('dsnt_pckh_hist', *[ptr(t) for t in dev], (C.c_double * T)(*thr), T, ptr(table), ptr(dist), B, J)
    return table.cpu().numpy(), dist.cpu().numpy()


def boot_dev(dev, ids, thr, R, seed, B, J, fill=FILL):
    """One `dsnt_pckh_boot` call into a table pre-filled with `fill`, with 8 guard cells behind it."""
    T = len(thr)
    cells = (R + 1) * J * (T + 1)
    table = torch.full((cells + 8,), SENTINEL, dtype=torch.int64, device='cuda')
    table[:cells] = fill
    ids_dev = torch.from_numpy(ids).cuda()
    call('dsnt_pckh_boot', *[ptr(t) for t in dev], ptr(ids_dev), (C.c_double * T)(*thr), T, C.c_uint64(seed), R, ptr(table),
         B, J)
    assert (table[cells:] == SENTINEL).all().item()
    return table[:cells].view(R + 1, J, T + 1).cpu().numpy()


def expected(dist, mask, ids, thr, R, seed):
    """The restatement's table from the device's distances (NaN where the mask is not 1, as `dsnt_pckh_hist` writes them)."""
    valid = mask == 1
    assert np.array_equal(np.isnan(dist) & ~valid, ~valid)
    return boot_ref.table(score_ref.column(dist, thr), valid, ids, R, seed, mask.shape[1], len(thr))


# (B, J, thresholds, R): see the module docstring for what each is next to
CASES = [
    (3, 16, THR1, 1),                                  # the smallest: copy 0 and one replicate
    (9, 16, THR1, 4), (9, 16, THR1, 5), (9, 16, THR3, 67),         # whole Philox calls, one word more, a chunk's tail
    (9, 16, THR1, CHUNK - 1), (9, 16, THR1, CHUNK),    # copies 0..R: exactly one chunk, and one past it
    (37, 7, DEFAULT, 25), (16, 16, DEFAULT, 9),        # chunks of 11 and of 4 copies: chunks that do not begin on a Philox call
    (SPAN // 5 + 1, 5, THR3, 6), (SPAN + 1, 1, THR1, 5),           # B * J one past a span; the span cuts an example in two
    (SPAN_BLOCKS * SPAN + 1, 1, THR1, 4),              # one past the span workgroups' stride
    (70, 16, THR3, 40),                                # more than one span, two chunks
    (40, 64, T63, 5), (40, 64, T64, 5),                # one copy per workgroup in LDS; the direct path
    (3, 1, THR1, CHUNK_BLOCKS * CHUNK),                # one chunk past the chunk workgroups' stride
]
assert (SPAN // 5 + 1) * 5 > SPAN and (SPAN // 5 + 1) * 5 % SPAN != 0


@pytest.mark.parametrize('B,J,thr,R', CASES, ids=['%dx%d-T%d-R%d' % (B, J, len(t), R) for B, J, t, R in CASES])
def test_table_equals_restatement(B, J, thr, R):
    args = case(B, J, seed=B * 100 + J)
    ids, seed = ids_for(B, seed=B + R), 0x0123456789ABCDEF ^ R
    dev = on_device(args)
    hist, dist = hist_dev(dev, thr, B, J)
    want = expected(dist, args[4], ids, thr, R, seed)
    got = boot_dev(dev, ids, thr, R, seed, B, J) - FILL
    valid = args[4] == 1
    print('B=%d J=%d T=%d R=%d: %d valid, copy sums %d..%d' % (B, J, len(thr), R, valid.sum(), want.sum((1, 2)).min(),
                                                               want.sum((1, 2)).max()))
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], hist) and got[0].sum() == valid.sum()       # copy 0 is dsnt_pckh_hist's table
    if B >= 3:                                                     # the NaN prediction and the zero head went to column T
        T = len(thr)
        k = score_ref.column(dist, thr)
        assert k[1, 0] == T and k[2, J - 1] == T and got[0, 0, T] >= 1 and got[0, J - 1, T] >= 1
    if B * J >= 256:                                               # the case has hits and misses, and weights beyond 1
        assert 0 < got[0, :, :len(thr)].sum() < valid.sum()
        assert (got[1:].sum((1, 2)) != got[0].sum()).any()


@pytest.mark.parametrize('kind', ['range', 'mixed'])
def test_ids_are_taken_as_their_64_bits(kind):
    """Contiguous ids and shuffled, wide and negative ones; the same examples under other ids give another table."""
    B, J, R, seed = 33, 16, 12, 77
    args = case(B, J, seed=3)
    dev = on_device(args)
    _, dist = hist_dev(dev, THR3, B, J)
    ids = ids_for(B, kind)
    got = boot_dev(dev, ids, THR3, R, seed, B, J, fill=0)
    assert np.array_equal(got, expected(dist, args[4], ids, THR3, R, seed))
    for other in (ids + (1 << 32), -ids - 1):                      # the high word and the sign both count
        moved = boot_dev(dev, other, THR3, R, seed, B, J, fill=0)
        assert np.array_equal(moved, expected(dist, args[4], other, THR3, R, seed))
        assert np.array_equal(moved[0], got[0]) and not np.array_equal(moved[1:], got[1:])
    # another seed: other weights; the high word of the seed counts too
    for other in (seed + 1, seed + (1 << 32)):
        moved = boot_dev(dev, ids, THR3, R, other, B, J, fill=0)
        assert np.array_equal(moved, expected(dist, args[4], ids, THR3, R, other)) and not np.array_equal(moved, got)


# ---------------------------------------------------------------------------------------------------- the accumulator
N, R, SEED = 101, 40, 5


@pytest.fixture(scope='module')
def whole():
    """One set of 101 examples: its arrays, device tensors, ids and the restated table (computed once, never changed)."""
    args = case(N, 16, seed=8)
    dev = on_device(args)
    ids = ids_for(N, seed=2)
    hist, dist = hist_dev(dev, THR3, N, 16)
    want = expected(dist, args[4], ids, THR3, R, SEED)
    want.setflags(write=False)
    return args, dev, torch.from_numpy(ids).cuda(), want


def _fed(dev, ids, batches, **kw):
    """A `PCKhBootstrap` fed the rows of each index array of `batches` as one batch."""
    ev = evaluator.PCKhBootstrap(replicates=R, thresholds=THR3, seed=SEED, **kw)
    pred, target, m, b, mask, head = dev
    for rows in batches:
        rows = torch.as_tensor(rows, device='cuda')
        ev.add_normalized(pred[rows], target[rows], mask[rows], head[rows], m[rows], b[rows], ids[rows.to(ids.device)])
    return ev


def test_batching_and_order_do_not_matter(whole):
    args, dev, ids, want = whole
    everything = np.arange(N)
    one = _fed(dev, ids, [everything])
    assert np.array_equal(one.counts().numpy(), want)
    cuts = [everything[:13], everything[13:64], everything[64:]]
    assert torch.equal(_fed(dev, ids, cuts).counts(), one.counts())                    # batches equal their concatenation
    assert torch.equal(_fed(dev, ids, cuts[::-1]).counts(), one.counts())              # in any order
    shuffled = np.random.default_rng(0).permutation(N)
    assert torch.equal(_fed(dev, ids, [shuffled[:50], shuffled[50:]]).counts(), one.counts())
    assert torch.equal(_fed(dev, ids, [everything, everything]).counts(), 2 * one.counts())    # twice the batch, twice the table
    ids_host = _fed(dev, ids.cpu(), [everything])                   # an index on the host is moved
    assert torch.equal(ids_host.counts(), one.counts())


def test_merge_of_halves_and_pckh_of_the_curve(whole):
    args, dev, ids, want = whole
    everything = np.arange(N)
    a, b = _fed(dev, ids, [everything[:47]]), _fed(dev, ids, [everything[47:]])
    a.merge(b)
    assert np.array_equal(a.counts().numpy(), want)
    curve = evaluator.PCKhCurve(thresholds=THR3)
    curve.add_normalized(dev[0], dev[1], dev[4], dev[5], dev[2], dev[3])
    assert torch.equal(a.counts()[0], curve.counts())
    for name in ('total_mpii', 'all', 'rwrist', 3):
        for thr in (0.1, 0.2, 0.5):
            assert a.pckh(thr, name) == curve.pckh(thr, name)
    rows = a.groups['total_mpii']
    assert np.array_equal(a.replicates(0.5), boot_ref.replicates(want, 2, rows))
    assert a.interval(0.5) == boot_ref.interval(want, 2, rows) and a.stderr(0.5) == boot_ref.stderr(want, 2, rows)
    # `add`: coordinates already in image space go through the identity transform
    img = evaluator.PCKhBootstrap(replicates=R, thresholds=THR3, seed=SEED)
    img.add(dev[0], dev[1], dev[4], dev[5], ids)
    ident = _fed([dev[0], dev[1], torch.eye(2, dtype=torch.float64, device='cuda').repeat(N, 1, 1),
                  torch.zeros(N, 2, dtype=torch.float64, device='cuda'), dev[4], dev[5]], ids, [everything])
    assert torch.equal(img.counts(), ident.counts()) and img.counts()[0].sum() == (args[4] == 1).sum()
    a.reset()
    assert not a.counts().any()


def test_ten_passes_give_identical_bits(whole):
    args, dev, ids, want = whole
    ids_host = ids.cpu().numpy()
    for _ in range(10):
        assert np.array_equal(boot_dev(dev, ids_host, THR3, R, SEED, N, 16, fill=0), want)


def test_fed_from_an_epoch_loader():
    """`sample['index']` of a shuffled `EpochLoader` is the id: two epochs in different orders and batchings, one table."""
    from dsnt.data import DeviceAugment, DeviceDataset, EpochLoader, ImageSpecs
    n, r = 21, np.random.default_rng(6)
    side = r.uniform(150, 500, n)
    mat = np.zeros((n, 3, 3))
    mat[:, 0, 0] = mat[:, 1, 1] = 2 / side
    mat[:, 0, 2], mat[:, 1, 2], mat[:, 2, 2] = -2 * r.uniform(300, 900, n) / side, -2 * r.uniform(200, 600, n) / side, 1
    kp = (r.uniform(-1.2, 1.2, (n, 16, 2)) - mat[:, None, :2, 2]) / mat[:, None, 0:1, 0]
    data = DeviceDataset.from_arrays(r.integers(0, 256, (n, 96, 96, 3), dtype=np.uint8), kp,
                                     (r.random((n, 16)) < 0.8).astype(np.float32), mat, r.uniform(40, 120, n))
    aug = DeviceAugment(ImageSpecs(64, True, True), (0.44, 0.44, 0.40), (0.25, 0.26, 0.27), use_aug=False, train=False)
    noise = torch.from_numpy(r.normal(0, 0.15, (n, 16, 2)).astype(np.float32)).cuda()      # the "model": per example

    def epoch(batch, seed):
        ev = evaluator.PCKhBootstrap(replicates=R, seed=SEED)
        rows, masks = [], []
        for s in EpochLoader(data, batch, aug, seed=seed):
            assert s['index'].dtype == torch.int64 and s['index'].is_cuda
            ev.add_normalized(s['part_coords'] + noise[s['index']], s['part_coords'], s['part_mask'], s['normalize'],
                              s['transform_m'], s['transform_b'], s['index'])
            rows.append(s['index'])
            masks.append(s['part_mask'])
        return ev, torch.cat(rows).cpu().numpy(), torch.cat(masks).cpu().numpy()
    a, order_a, mask_a = epoch(8, seed=1)
    b, order_b, _ = epoch(5, seed=2)
    assert sorted(order_a) == sorted(order_b) == list(range(n)) and not np.array_equal(order_a, order_b)
    assert torch.equal(a.counts(), b.counts()) and 0 < a.pckh() < 1
    # the weighted valid count of every copy: the weight of each example, by its id, over its valid joints
    valid = (mask_a == 1).astype(np.int64)
    assert valid.sum() > 0
    assert np.array_equal(a.counts().numpy().sum(2), np.einsum('nr,nj->rj', boot_ref.weights(order_a, R, SEED), valid))


def test_paired_comparison(whole):
    """Two prediction sets over the same ids, fed in different batchings: `compare` is the numpy reader on the restated
    tables, and refuses when one side misses an example."""
    args, dev, ids, want = whole
    r = np.random.default_rng(12)
    better = (args[1] + r.normal(0, 0.12, args[1].shape)).astype(np.float32)
    better[1, 0, 0] = np.nan
    dev_b = [torch.from_numpy(better).cuda()] + list(dev[1:])
    _, dist_b = hist_dev(dev_b, THR3, N, 16)
    want_b = expected(dist_b, args[4], ids.cpu().numpy(), THR3, R, SEED)
    everything = np.arange(N)
    a = _fed(dev, ids, [everything[:13], everything[13:]])
    b = _fed(dev_b, ids, [everything[70:], everything[:32], everything[32:70]])
    assert np.array_equal(b.counts().numpy(), want_b)
    rows = a.groups['total_mpii']
    for thr, k, level in ((0.5, 2, 0.95), (0.2, 1, 0.9)):
        got = b.compare(a, thr, level=level)
        assert got == boot_ref.compare(want_b, want, k, rows, level)
        print('PCKh@%g: diff %.4f, interval %s, stderr %.4f, p_greater %.3f'
              % (thr, got['diff'], got['interval'], got['stderr'], got['p_greater']))
    assert got['diff'] > 0 and got['p_greater'] > 0.9
    assert b.compare(a, 0.5, 'rwrist') == boot_ref.compare(want_b, want, 2, [10])
    short = _fed(dev, ids, [everything[:-1]])
    with pytest.raises(ValueError, match='same examples'):
        b.compare(short)
    with pytest.raises(ValueError, match='seed'):
        b.compare(evaluator.PCKhBootstrap(replicates=R, thresholds=THR3, seed=SEED + 1))
