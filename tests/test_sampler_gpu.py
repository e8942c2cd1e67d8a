"""The importance sampler's kernels on the MI355X (csrc/sampler.hip) against their numpy restatement
(tests/sampler_ref.py): `dsnt_sample_cdf` bit for bit at every size where the scan takes another path, with guard cells
behind the output and the scratch; `dsnt_sample_indices` exactly, over seeds, epochs and sub-ranges up to position 2^32;
`dsnt_example_scores` to one fp32 ulp, with the table's ordering rules."""
import numpy as np
import pytest
import torch

import sampler_ref

pytestmark = pytest.mark.gpu

TILE = sampler_ref.TILE
GUARD = 8
SENTINEL = 0x5A5A5A5A5A5A5A5A
# the block scan's edges, and 257 tiles: more totals than the one workgroup that scans them has threads
SIZES = (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 257 * TILE + 5)


def _weights(n, seed, kind='mixed'):
    """fp32 weights, log-uniform over 40 binades, with runs of zeros at both ends, NaN, +-inf, negatives and subnormals
    planted where there is room, and the maximum in the last position."""
    r = np.random.default_rng(seed)
    w = np.exp2(r.uniform(-20, 20, n)).astype(np.float32)
    if kind == 'zero':
        w[:] = 0
        if n >= 8:
            w[1], w[2], w[3], w[5] = np.nan, -1, np.inf, -0.0
        return w
    if kind == 'subnormal':                                    # the scale itself comes from a subnormal maximum
        w = r.integers(0, 2 ** 23, n).astype(np.uint32).view(np.float32)
        w[-1] = np.uint32(2 ** 23 - 1).view(np.float32)
        return w
    if n >= 64:
        w[:5] = 0
        w[-7:-1] = 0
        w[7], w[8], w[9], w[10], w[11], w[12] = np.nan, np.inf, -1, 1e-40, -0.0, -np.inf
        w[n // 2] = 1e-45
    w[-1] = np.float32(2 ** 21) * np.float32(1.37)
    return w


def _device_cdf(w):
    """(cdf uint64 numpy [n], the guard cells behind the output and behind the scratch) of one dsnt_sample_cdf call."""
    from dsnt import _lib
    n = len(w)
    words = 1 + (n + TILE - 1) // TILE                          # DSNT_SAMPLE_CDF_SCRATCH_BYTES(n) / 8
    out = torch.full((n + GUARD,), SENTINEL, dtype=torch.int64, device='cuda')
    scratch = torch.full((words + GUARD,), SENTINEL, dtype=torch.int64, device='cuda')
    _lib.call('dsnt_sample_cdf', _lib.ptr(torch.tensor(w).cuda()), n, _lib.ptr(out), _lib.ptr(scratch))
    out, scratch = out.cpu().numpy(), scratch.cpu().numpy()
    return out[:n].view(np.uint64), out[n:], scratch[words:]


CASES = [(n, 'mixed') for n in SIZES] + [(TILE + 1, 'subnormal'), (2 * TILE + 3, 'zero'), (5, 'zero')]
_cache = {}


def _case(n, kind):
    """(weights, the restatement's CDF) of a case: computed once, shared by the tests, never written."""
    if (n, kind) not in _cache:
        w = _weights(n, 100 + n % 97, kind)
        c = sampler_ref.cdf(w)
        w.setflags(write=False)
        c.setflags(write=False)
        _cache[(n, kind)] = (w, c)
    return _cache[(n, kind)]


def test_scratch_macro_is_what_the_tests_allocate():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'dsnt_hip.h')).read()
    body = re.search(r'#define DSNT_SAMPLE_CDF_SCRATCH_BYTES\(n\) (.*)', text).group(1)
    assert ' '.join(body.split()) == '(8 * (1 + ((int64_t)(n) + DSNT_SAMPLE_TILE - 1) / DSNT_SAMPLE_TILE))'


@pytest.mark.parametrize('n,kind', CASES)
def test_device_cdf_equals_restatement_bit_for_bit(n, kind):
    w, want = _case(n, kind)
    got, guard, scratch_guard = _device_cdf(w)
    assert (guard == SENTINEL).all() and (scratch_guard == SENTINEL).all()
    assert np.array_equal(got, want), (n, kind, int(np.flatnonzero(got != want)[0]))
    if kind == 'zero':
        assert not got.any()
    else:
        assert int(got[-1]) < 2 ** 56 and int(got[-1]) - (int(got[-2]) if n > 1 else 0) >= 2 ** 31    # the maximum is last
    again, _, _ = _device_cdf(w)                               # and the same on a second build
    assert np.array_equal(again, got)


def _device_draw(cdf_dev, n, seed, epoch, first, count):
    from dsnt import _lib
    out = torch.full((count + GUARD,), SENTINEL, dtype=torch.int64, device='cuda')
    _lib.call('dsnt_sample_indices', _lib.ptr(cdf_dev), n, seed, epoch, first, count, _lib.ptr(out))
    out = out.cpu().numpy()
    assert (out[count:] == SENTINEL).all()
    return out[:count]


@pytest.mark.parametrize('n,kind', CASES)
def test_device_draw_equals_restatement(n, kind):
    _, c = _case(n, kind)
    cdf_dev = torch.tensor(c.view(np.int64)).cuda()
    full = 1500
    for seed in (0, 0xDEADBEEFCAFEF00D):
        for epoch in (0, 2 ** 33 + 5):
            want = sampler_ref.draw(c, seed, epoch, np.arange(full))
            got = _device_draw(cdf_dev, n, seed, epoch, 0, full)
            assert np.array_equal(got, want), (n, kind, seed, epoch)
            # a sub-range is the matching slice of the full draw, whatever its size
            for first, count in ((0, 1), (257, 700), (full - 1, 1)):
                assert np.array_equal(_device_draw(cdf_dev, n, seed, epoch, first, count), want[first:first + count])
            # the last positions there are: the range ends at 2^32
            first = 2 ** 32 - 100
            assert np.array_equal(_device_draw(cdf_dev, n, seed, epoch, first, 100),
                                  sampler_ref.draw(c, seed, epoch, np.arange(first, 2 ** 32)))
            if kind == 'zero':
                assert (got == -1).all()
            else:
                assert got.min() >= 0 and got.max() < n


def test_draws_from_a_device_built_cdf_never_name_a_row_without_weight():
    w, c = _case(2 * TILE + 3, 'mixed')
    from dsnt import _lib
    n = len(w)
    cdf = torch.empty(n, dtype=torch.int64, device='cuda')
    scratch = torch.empty(1 + (n + TILE - 1) // TILE, dtype=torch.int64, device='cuda')
    _lib.call('dsnt_sample_cdf', _lib.ptr(torch.tensor(w).cuda()), n, _lib.ptr(cdf), _lib.ptr(scratch))
    got = _device_draw(cdf, n, 3, 1, 0, 20000)
    q = sampler_ref.quantise(w)
    assert (q[got] > 0).all() and np.array_equal(got, sampler_ref.draw(c, 3, 1, np.arange(20000)))


# ---------------------------------------------------------------- dsnt_example_scores
def _batch(B, J, seed):
    r = np.random.default_rng(seed)
    pred = r.uniform(-1, 1, (B, J, 2)).astype(np.float32)
    target = (pred + r.normal(0, 0.08, (B, J, 2))).astype(np.float32)
    m = r.uniform(60, 140, (B, 2, 2)) * np.array([[1, 0.1], [-0.1, 1]])
    b = r.uniform(100, 500, (B, 1, 2))
    head = r.uniform(40, 120, B)
    mask = (r.random((B, J)) < 0.7).astype(np.float32)
    mask[:, 0] = 1
    return pred, target, m, b, mask, head


def _device_scores(batch, idx, stamp, table, n_rows, lead):
    """One dsnt_example_scores call on the rows [lead, lead + n_rows) of `table`; returns the fp32 scores (numpy)."""
    from dsnt import _lib
    pred, target, m, b, mask, head = batch
    B, J = mask.shape
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (pred, target, m, b.reshape(B, 2), mask, head)]
    score = torch.full((B + GUARD,), 7.0, device='cuda')
    _lib.call('dsnt_example_scores', *map(_lib.ptr, dev), _lib.ptr(torch.from_numpy(np.asarray(idx, np.int64)).cuda()),
              n_rows, stamp, _lib.ptr(table[lead:lead + n_rows]), _lib.ptr(score), B, J)
    score = score.cpu().numpy()
    assert (score[B:] == 7.0).all()
    return score[:B]


def _ulps(a, b):
    """Distance in fp32 steps between finite non-negative fp32 arrays."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize('J', [16, 3])
def test_example_scores_and_table_against_fp64_restatement(J):
    B, N, lead = 5, 9, 4
    table = torch.full((lead + N + lead,), SENTINEL, dtype=torch.int64, device='cuda')
    table[lead:lead + N] = 0
    want_table = np.zeros(N, dtype=np.uint64)

    def step(batch, idx, stamp):
        nonlocal want_table
        got = _device_scores(batch, idx, stamp, table, N, lead)
        want64 = sampler_ref.example_scores(*batch[:4], batch[4], batch[5])
        want = want64.astype(np.float32)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        # device and numpy hold the fp64 mean to 1e-9 relative, far below half an fp32 ulp: the roundings differ by <= 1
        assert (_ulps(got[ok], want[ok]) <= 1).all(), (got, want)
        want_table = sampler_ref.table_words(want, idx, stamp, N, want_table)
        have = table.cpu().numpy()
        assert (have[:lead] == SENTINEL).all() and (have[lead + N:] == SENTINEL).all()      # rows -1 and N wrote nothing
        have = have[lead:lead + N].view(np.uint64)
        assert np.array_equal(have >> np.uint64(32), want_table >> np.uint64(32)), (have, want_table)
        low = lambda t: (t & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert (np.abs(low(have) - low(want_table)) <= 1).all()
        return got

    a = list(_batch(B, J, seed=J))
    a[1][1] = a[0][1] + (a[1][1] - a[0][1]) * 3                # example 1 misses three times as far as it did
    a[4][2] = 0                                                # example 2 has no valid joint
    a[0][3, 0] = np.nan                                        # example 3 predicts a NaN on a counted joint
    # examples 0 and 1 share row 4; 2 and 3 write nothing; 4 goes to row 7
    got = step(a, [4, 4, 2, 5, 7], stamp=7)
    assert np.isnan(got[2]) and np.isnan(got[3]) and abs(got[1] - got[0]) > 0.01 * max(got[0], got[1])
    have = table.cpu().numpy()[lead:lead + N]
    keep = max(got[0], got[1])
    assert have[4] == (7 << 32) | int(np.float32(keep).view(np.uint32)) and have[2] == 0 and have[5] == 0
    # an older stamp writes rows never seen, and leaves the newer ones alone
    b = _batch(B, J, seed=50 + J)
    step(b, [4, 7, 2, 5, 0], stamp=5)
    have2 = table.cpu().numpy()[lead:lead + N]
    assert have2[4] == have[4] and have2[7] == have[7] and have2[2] >> 32 == 5 and have2[0] >> 32 == 5
    # rows outside the table, and a newer stamp that replaces a larger score with a smaller one
    c = list(_batch(B, J, seed=90 + J))
    c[1][4] = c[0][4]                                          # example 4: a perfect prediction, score 0
    got = step(c, [-1, N, 1, 1, 4], stamp=2 ** 31 - 1)
    have3 = table.cpu().numpy()[lead:lead + N]
    assert got[4] == 0 and have3[4] == (2 ** 31 - 1) << 32 and have3[7] == have[7]


def test_example_scores_class_reads_its_table_back():
    from dsnt.data import ExampleScores
    B, J, N = 5, 16, 9
    batch = _batch(B, J, seed=3)
    pred, target, m, b, mask, head = (torch.from_numpy(a).cuda() for a in batch)
    idx = torch.tensor([8, 0, 3, 3, -1], device='cuda')
    s = ExampleScores(N)
    got = s.add(idx, pred, target, mask, head, m, b, stamp=4)
    want = sampler_ref.example_scores(*batch[:4], batch[4], batch[5]).astype(np.float32)
    assert got.dtype == torch.float32 and (_ulps(got.cpu().numpy(), want) <= 1).all()
    assert s.last_seen().cpu().tolist() == [4, 0, 0, 4, 0, 0, 0, 0, 4]
    sc = s.scores().cpu().numpy()
    assert np.array_equal(np.isnan(sc), [False, True, True, False] + [True] * 4 + [False])
    assert sc[8] == got[0].item() and sc[0] == got[1].item() and sc[3] == max(got[2].item(), got[3].item())
    other = ExampleScores(N)
    other.add(idx.flip(0).contiguous(), pred, target, mask, head, m, b, stamp=3)      # rows -1, 3, 3, 0, 8: older
    other.add(torch.tensor([1, 1, 1, 1, 1], device='cuda'), pred, target, mask, head, m, b, stamp=9)
    before = s.table.clone()
    s.merge(other)
    assert torch.equal(s.table[[0, 3, 8]], before[[0, 3, 8]]) and s.last_seen()[1].item() == 9
    assert s.scores()[1].item() == got.max().item()
    w = ExampleScores.weights_from_table(s.table)
    assert w.is_cuda and torch.allclose(w.cpu(), ExampleScores.weights_from_table(s.table.cpu()), rtol=1e-6, atol=0)
    t = ExampleScores(N)
    t.load_state_dict(s.state_dict())
    assert torch.equal(t.table, s.table)
