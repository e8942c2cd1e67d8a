"""CPU checks of the importance sampler (dsnt.data.ExampleScores, WeightedLoader; csrc/sampler.hip): the entry points are
exported, declared, bound and validate their arguments without a GPU; the numpy restatement (tests/sampler_ref.py) has
the properties the construction promises (q < 2^32, a row with q == 0 is never drawn, draws are a function of the
position alone, frequencies follow q / T); `weights_from_table` and the loader's host-side refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sampler_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dsnt_sample_cdf', 'dsnt_sample_indices', 'dsnt_example_scores')


def test_sampler_symbols_exported_declared_and_bound():
    from dsnt import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, 'include', 'dsnt_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
        assert re.search(r'\bint\s+%s\s*\(' % n, header), n
    assert lib.dsnt_version() >= 130
    macros = dict(re.findall(r'^#define (DSNT_SAMPLE_[A-Z_]+) (\S.*)$', header, flags=re.M))
    assert int(macros['DSNT_SAMPLE_DOMAIN'].rstrip('u'), 16) == sampler_ref.DOMAIN == 0x57534D50
    assert eval(macros['DSNT_SAMPLE_MAX_N']) == sampler_ref.MAX_N == 2 ** 24
    assert int(macros['DSNT_SAMPLE_TILE']) == sampler_ref.TILE
    # a domain of its own: not the augmentation draw's, the epoch order's or the bootstrap's
    boot = int(re.search(r'#define DSNT_PCKH_BOOT_DOMAIN (0x[0-9A-Fa-f]+)u', text).group(1), 16)
    assert sampler_ref.DOMAIN not in {0, 1, 2, boot} | {0x4F524400 + r for r in range(8)}
    assert 'never drawn' in ' '.join(text.split()).lower()          # the resolution limit is part of the contract


def test_sampler_entry_points_validate_arguments_without_gpu():
    from dsnt import _lib
    lib = _lib.load()
    v = C.c_void_p(4096)
    err = lambda: lib.dsnt_last_error().decode()
    # dsnt_sample_cdf(weights, n, cdf, scratch)
    for args in ((None, 8, v, v), (v, 8, None, v), (v, 8, v, None)):
        assert lib.dsnt_sample_cdf(*args, None) == 3 and 'dsnt_sample_cdf: null pointer' in err()
    for n in (0, -1, 2 ** 24 + 1):
        assert lib.dsnt_sample_cdf(v, n, v, v, None) == 1 and 'dsnt_sample_cdf: n=%d outside' % n in err()
    # dsnt_sample_indices(cdf, n, seed, epoch, first, count, out)
    assert lib.dsnt_sample_indices(None, 8, 0, 0, 0, 4, v, None) == 3
    assert lib.dsnt_sample_indices(v, 8, 0, 0, 0, 4, None, None) == 3 and 'dsnt_sample_indices: null pointer' in err()
    for n in (0, 2 ** 24 + 1):
        assert lib.dsnt_sample_indices(v, n, 0, 0, 0, 4, v, None) == 1, n
    for first, count in ((0, 0), (0, -3), (-1, 4), (2 ** 32 - 3, 4), (0, 2 ** 32 + 1), (2 ** 32, 1)):
        assert lib.dsnt_sample_indices(v, 8, 0, 0, first, count, v, None) == 1, (first, count)
        assert 'dsnt_sample_indices: bad range first=%d count=%d' % (first, count) in err()
    # dsnt_example_scores(pred, target, m, b, mask, head, idx, N, stamp, table, score, B, J)
    def scores(ptrs=(v,) * 7, N=10, stamp=1, table=v, score=v, B=4, J=16):
        return lib.dsnt_example_scores(*ptrs, N, stamp, table, score, B, J, None)
    for k in range(7):
        assert scores(ptrs=(v,) * k + (None,) + (v,) * (6 - k)) == 3, k
    assert scores(table=None) == 3 and scores(score=None) == 3
    assert scores(B=0) == 3 and scores(B=-2) == 3 and scores(J=0) == 3 and scores(J=-1) == 3
    assert 'dsnt_example_scores: bad argument' in err()
    assert scores(N=0) == 3
    assert scores(stamp=0) == 3 and 'stamp 0 outside [1, 2^31)' in err()
    assert scores(stamp=2 ** 31) == 3 and scores(stamp=2 ** 32 - 1) == 3
    # valid arguments record a launch without touching a device, so nothing above got as far as one by luck
    h = lib.dsnt_list_create()
    assert lib.dsnt_list_begin(h) == 0
    try:
        assert scores(stamp=2 ** 31 - 1) == 0 and lib.dsnt_list_size(h) == 1
        assert lib.dsnt_sample_indices(v, 8, 0, 0, 2 ** 32 - 4, 4, v, None) == 0 and lib.dsnt_list_size(h) == 2
        assert lib.dsnt_sample_cdf(v, 2 ** 24, v, v, None) == 0 and lib.dsnt_list_size(h) == 7       # five launches
    finally:
        assert lib.dsnt_list_end() == 0
        lib.dsnt_list_destroy(h)


def _weights(n, seed, binades=40):
    r = np.random.default_rng(seed)
    return np.exp2(r.uniform(-binades / 2, binades / 2, n)).astype(np.float32)


def test_quantised_weights_stay_below_two_to_the_32():
    for n, seed in ((1, 0), (2, 1), (1000, 2), (5000, 3)):
        w = _weights(n, seed)
        q = sampler_ref.quantise(w)
        assert q.dtype == np.uint64 and int(q.max()) < 2 ** 32 and int(q[np.argmax(w)]) >= 2 ** 31
        assert np.array_equal(sampler_ref.cdf(w), np.cumsum([int(x) for x in q]).astype(np.uint64))
    w = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 3.0, 1e-45, 2.5, 3.0 * 2.0 ** -33], dtype=np.float32)
    q = sampler_ref.quantise(w)
    assert [int(x) for x in q] == [0, 0, 0, 0, 0, 0, 3 << 30, 0, 5 << 29, 0]
    assert not sampler_ref.quantise(np.array([0.0, np.nan, -2.0], dtype=np.float32)).any()
    # the largest weight alone decides the scale, down to subnormals: 2^-149 and 3 * 2^-149
    tiny = np.array([1e-45, 4e-45], dtype=np.float32)
    assert [int(x) for x in sampler_ref.quantise(tiny)] == [1 << 30, 3 << 30]


def test_a_row_with_zero_quantum_is_never_drawn():
    w = _weights(400, 5)
    w[::7] = 0
    w[3] = np.nan
    w[399] = w.max() * 4                                   # pushes the smallest weights below the resolution
    q = sampler_ref.quantise(w)
    assert (q[w > 0] == 0).any(), 'the case needs positive weights that quantise to 0'
    got = sampler_ref.draw(sampler_ref.cdf(w), 11, 2, np.arange(20000))
    assert got.min() >= 0 and got.max() < 400 and not (q[got] == 0).any()
    assert np.array_equal(sampler_ref.draw(sampler_ref.cdf(np.zeros(9, np.float32)), 1, 0, np.arange(50)), np.full(50, -1))


@pytest.mark.parametrize('at', [0, 18, 36])
def test_a_single_weighted_row_is_drawn_every_time(at):
    w = np.zeros(37, dtype=np.float32)
    w[at] = 0.3
    for seed, epoch in ((0, 0), (0xDEADBEEFCAFEF00D, 2 ** 33 + 5)):
        assert np.array_equal(sampler_ref.draw(sampler_ref.cdf(w), seed, epoch, np.arange(3000)), np.full(3000, at))


def test_sub_ranges_are_slices_of_the_full_draw():
    c = sampler_ref.cdf(_weights(777, 9))
    full = sampler_ref.draw(c, 4, 6, np.arange(5000))
    for first, count in ((0, 1), (1, 31), (1234, 999), (4999, 1)):
        assert np.array_equal(sampler_ref.draw(c, 4, 6, np.arange(first, first + count)), full[first:first + count])
    assert not np.array_equal(full, sampler_ref.draw(c, 4, 7, np.arange(5000)))
    assert not np.array_equal(full, sampler_ref.draw(c, 5, 6, np.arange(5000)))
    # position 2^32 - 1 is the last one; the counter's first word is the position itself
    last = sampler_ref.draw(c, 4, 6, np.array([2 ** 32 - 1]))
    assert 0 <= int(last[0]) < 777


@pytest.mark.parametrize('seed', [0, 5])
def test_frequencies_follow_the_quantised_weights(seed):
    """Fixed inputs, so a condition and not a gamble: every row's count within 4 binomial standard deviations of n q / T."""
    w = np.array([1, 0, 3, 0.5, 0, 2.5, 1e-12, 7], dtype=np.float32)
    n = 200000
    q = sampler_ref.quantise(w).astype(np.float64)
    p = q / q.sum()
    counts = np.bincount(sampler_ref.draw(sampler_ref.cdf(w), seed, 3, np.arange(n)), minlength=8)
    sd = np.sqrt(n * p * (1 - p))
    assert counts.sum() == n and counts[1] == 0 and counts[4] == 0
    for j in range(8):
        assert abs(counts[j] - n * p[j]) <= 4 * sd[j], (j, counts[j], n * p[j], sd[j])


def _table(scores, stamps):
    bits = np.asarray(scores, dtype=np.float32).view(np.uint32).astype(np.int64)
    return torch.from_numpy((np.asarray(stamps, dtype=np.int64) << 32) | np.where(np.asarray(stamps) > 0, bits, 0))


def test_weights_from_table_on_cpu_tensors():
    from dsnt.data import ExampleScores
    wft = ExampleScores.weights_from_table
    t = _table([0.1, 0.0, 0.3, 0.2, 0.0], [3, 0, 1, 2, 0])                  # rows 1 and 4 never seen; mean seen score 0.2
    mean = np.float32(np.float64(np.float32(0.1)) + np.float64(np.float32(0.3)) + np.float64(np.float32(0.2))) / 3
    ratio = np.array([0.1, 0, 0.3, 0.2, 0], dtype=np.float32) / np.float32(mean)
    w = wft(t)
    assert w.dtype == torch.float32 and w.shape == (5,)
    np.testing.assert_allclose(w.numpy()[[0, 2, 3]], 0.1 + ratio[[0, 2, 3]], rtol=1e-6)
    assert w[1] == w[4] == w[2] and w[2] == w.max()                         # unseen = the largest seen weight
    w = wft(t, unseen='mean')
    assert w[1] == 1 and w[4] == 1
    np.testing.assert_allclose(w.numpy()[[0, 2, 3]], 0.1 + ratio[[0, 2, 3]], rtol=1e-6)
    w = wft(t, power=2.0, floor=0.0)
    np.testing.assert_allclose(w.numpy()[[0, 2, 3]], ratio[[0, 2, 3]] ** 2, rtol=1e-6)
    assert w[1] == w[2]
    w = wft(t, power=0.0, floor=0.5)                                        # power 0: every seen row alike
    assert torch.equal(w, torch.full((5,), 1.5))
    for unseen in ('max', 'mean'):                                          # nothing seen: uniform
        assert torch.equal(wft(torch.zeros(6, dtype=torch.int64), unseen=unseen), torch.ones(6))
    w = wft(_table([0.0, 0.0, 0.0], [1, 1, 0]))                             # every seen score 0: nothing to tell rows apart
    assert torch.equal(w, torch.full((3,), 1.1))
    with pytest.raises(RuntimeError, match='dsnt: unseen'):
        wft(t, unseen='min')
    with pytest.raises(RuntimeError, match='dsnt: weights_from_table'):
        wft(t, floor=-0.1)
    with pytest.raises(RuntimeError, match='dsnt: weights_from_table'):
        wft(t, power=float('nan'))
    with pytest.raises(RuntimeError, match='dsnt: a score table'):
        wft(t.float())


def test_example_scores_refuses_bad_arguments():
    from dsnt.data import ExampleScores
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ExampleScores(8, device='cpu')
    with pytest.raises(RuntimeError, match='n >= 1'):
        ExampleScores(0)
    s = ExampleScores.__new__(ExampleScores)                                # a shell around a CPU table: host logic only
    s.table = _table([0.1, 0.0, 0.3], [3, 0, 1])
    assert len(s) == 3
    assert s.last_seen().tolist() == [3, 0, 1]
    sc = s.scores()
    assert sc.dtype == torch.float32 and sc[0] == np.float32(0.1) and torch.isnan(sc[1]) and sc[2] == np.float32(0.3)
    s.merge(_table([0.5, 0.2, 0.9], [2, 1, 1]))                             # older, first sight, same stamp and larger
    assert s.last_seen().tolist() == [3, 1, 1]
    assert s.scores().tolist() == [np.float32(0.1), np.float32(0.2), np.float32(0.9)]
    state = s.state_dict()
    s.table.zero_()
    assert state['table'].tolist() != s.table.tolist()                      # a copy
    s.load_state_dict(state)
    assert s.last_seen().tolist() == [3, 1, 1]
    with pytest.raises(RuntimeError, match='dsnt: merge'):
        s.merge(torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='dsnt: the state'):
        s.load_state_dict({'table': torch.zeros(3)})
    B, J = 2, 16
    args = (torch.zeros(B, J, 2), torch.zeros(B, J, 2), torch.ones(B, J), torch.ones(B), torch.eye(2).expand(B, 2, 2),
            torch.zeros(B, 1, 2))
    idx = torch.zeros(B, dtype=torch.int64)
    for stamp in (0, -1, 2 ** 31):
        with pytest.raises(RuntimeError, match='dsnt: stamp'):
            s.add(idx, *args, stamp=stamp)
    with pytest.raises(RuntimeError, match='dsnt: index'):
        s.add(idx.int(), *args, stamp=1)
    with pytest.raises(RuntimeError, match='dsnt: index'):
        s.add(idx[:1], *args, stamp=1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        s.add(idx, *args, stamp=1)


def _stand_in(N=6, R=8, J=16):
    """A DeviceDataset shell around CPU tensors, as in tests/test_loader_cpu.py: the checks are host logic."""
    from dsnt.data import DeviceDataset
    d = DeviceDataset.__new__(DeviceDataset)
    d.crops, d.keypoints, d.keypoint_mask = (torch.zeros(N, R, R, 3, dtype=torch.uint8),
                                             torch.zeros(N, J, 2, dtype=torch.float64), torch.ones(N, J))
    d.matrix, d.head_lengths = torch.eye(3, dtype=torch.float64).expand(N, 3, 3).contiguous(), torch.ones(N, dtype=torch.float64)
    return d


def test_weighted_loader_refuses_bad_arguments():
    from dsnt.data import DeviceAugment, EpochLoader, ImageSpecs, WeightedLoader
    assert issubclass(WeightedLoader, EpochLoader)
    aug = DeviceAugment(ImageSpecs(4, False, False), (0, 0, 0), (1, 1, 1))
    d = _stand_in(N=6)
    w = torch.ones(6)
    with pytest.raises(RuntimeError, match='dsnt: weights must be a float32 tensor'):
        WeightedLoader(d, 2, aug, w.double())
    with pytest.raises(RuntimeError, match='dsnt: weights must be a float32 tensor'):
        WeightedLoader(d, 2, aug, [1.0] * 6)
    with pytest.raises(RuntimeError, match=r'dsnt: weights must have shape \(6,\)'):
        WeightedLoader(d, 2, aug, torch.ones(5))
    with pytest.raises(RuntimeError, match=r'dsnt: weights must have shape \(6,\)'):
        WeightedLoader(d, 2, aug, torch.ones(6, 1))
    with pytest.raises(RuntimeError, match="dsnt: weights must be on the dataset's device"):
        WeightedLoader(d, 2, aug, torch.ones(6, device='meta'))
    with pytest.raises(RuntimeError, match='no CPU fallback'):             # all host checks passed: the CDF build is next
        WeightedLoader(d, 2, aug, w)
    with pytest.raises(RuntimeError, match='dsnt: samples_per_epoch'):
        WeightedLoader(d, 2, aug, w, samples_per_epoch=0)
    with pytest.raises(RuntimeError, match='dsnt: samples_per_epoch'):
        WeightedLoader(d, 2, aug, w, samples_per_epoch=2 ** 32 + 1)
    # EpochLoader's refusals, with samples_per_epoch in the place of the dataset's length
    with pytest.raises(RuntimeError, match='leaves no batch'):
        WeightedLoader(d, 4, aug, w, samples_per_epoch=3, drop_last=True)
    with pytest.raises(RuntimeError, match='leaves no batch'):
        WeightedLoader(d, 4, aug, w, drop_last=True, world_size=2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):             # 30 positions hold 3 x 2 batches of 4
        WeightedLoader(d, 4, aug, w, samples_per_epoch=30, drop_last=True, world_size=2, rank=1)
    with pytest.raises(RuntimeError, match='drop_last'):
        WeightedLoader(d, 2, aug, w, world_size=2)
    with pytest.raises(RuntimeError, match='rank'):
        WeightedLoader(d, 2, aug, w, rank=1)
    with pytest.raises(RuntimeError, match='batch_size'):
        WeightedLoader(d, 0, aug, w)
    with pytest.raises(RuntimeError, match='DeviceDataset'):
        WeightedLoader(object(), 2, aug, w)
    with pytest.raises(RuntimeError, match='DeviceAugment'):
        WeightedLoader(d, 2, object(), w)
    with pytest.raises(RuntimeError, match='HFLIP_INDICES'):
        WeightedLoader(_stand_in(J=15), 2, aug, w)
