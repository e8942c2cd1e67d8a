"""`dsnt.data.WeightedLoader` and `ExampleScores` on the MI355X: batches are `DeviceAugment` on the rows the numpy
restatement of the weighted draw names (tests/sampler_ref.py), bit for bit; ranks split an epoch's positions; epoch
lengths of their own; a re-weighting takes effect at the next batch; a resumed loader repeats the uninterrupted batches;
nothing crop-sized is allocated per batch; and a closed loop (loader, model, scores, weights, loader) runs without a host
synchronisation."""
import numpy as np
import pytest
import torch

import sampler_ref

pytestmark = pytest.mark.gpu

N, R, S, J = 12, 48, 32, 16
KEYS = ('input', 'part_coords', 'part_mask', 'transform_m', 'transform_b', 'normalize', 'hflip')


def _arrays(n=N, r_side=R, seed=0):
    """A synthetic training set as host arrays (crops, keypoints, keypoint_mask, matrix, head_lengths)."""
    r = np.random.default_rng(seed)
    side = r.uniform(150, 500, n)
    m = np.zeros((n, 3, 3))
    m[:, 0, 0] = m[:, 1, 1] = 2 / side
    m[:, 0, 2], m[:, 1, 2], m[:, 2, 2] = -2 * r.uniform(300, 900, n) / side, -2 * r.uniform(200, 600, n) / side, 1
    kp = (r.uniform(-1.2, 1.2, (n, J, 2)) - m[:, None, :2, 2]) / m[:, None, 0:1, 0]
    return (r.integers(0, 256, (n, r_side, r_side, 3), dtype=np.uint8), kp, (r.random((n, J)) < 0.8).astype(np.float32),
            m, r.uniform(40, 120, n))


@pytest.fixture(scope='module')
def pool():
    from dsnt.data import DeviceDataset
    return DeviceDataset.from_arrays(*_arrays())


def _augment(size=S, use_aug=True, train=True, seed=17):
    from dsnt.data import DeviceAugment, ImageSpecs
    return DeviceAugment(ImageSpecs(size, True, True), (0.44, 0.44, 0.40), (0.25, 0.26, 0.27), use_aug=use_aug,
                         train=train, seed=seed)


def _w(seed=0, n=N):
    """Row weights (numpy fp32) over two decades with two rows of no weight."""
    w = np.exp2(np.random.default_rng(seed).uniform(-3, 3, n)).astype(np.float32)
    w[[3, 8]] = 0
    return w


def _dev(w):
    return torch.tensor(w, dtype=torch.float32, device='cuda')


def _rows(d, idx):
    return d.crops[idx], d.keypoints[idx], d.keypoint_mask[idx], d.matrix[idx], d.head_lengths[idx]


def _assert_same(a, b, keys=KEYS):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert torch.equal(a[k], b[k]), (k, (a[k].double() - b[k].double()).abs().max().item())
    for k in ('scale', 'rot', 'hflip', 'gain'):
        assert torch.equal(a['params'][k], b['params'][k]), k


def _index(batches):
    return torch.cat([s['index'] for s in batches]).cpu().numpy()


@pytest.mark.parametrize('flip_pair', [False, True])
def test_batches_equal_device_augment_on_the_rows_the_restatement_names(pool, flip_pair):
    from dsnt.data import WeightedLoader
    aug = _augment()
    w = _w(1)
    ld = WeightedLoader(pool, 5, aug, _dev(w), seed=5, flip_pair=flip_pair)
    ld.set_epoch(2)
    want_rows = sampler_ref.draw(sampler_ref.cdf(w), 5, 2, np.arange(N))
    assert np.array_equal(ld.indices().cpu().numpy(), want_rows) and np.array_equal(ld.indices(2).cpu().numpy(), want_rows)
    sizes = []
    for s, got in enumerate(ld):
        assert got['index'].dtype == torch.int64
        assert np.array_equal(got['index'].cpu().numpy(), want_rows[5 * s:5 * s + 5])
        want = aug(*_rows(pool, got['index']), step=2 * len(ld) + s, flip_pair=flip_pair)
        _assert_same(got, want, KEYS + (('input_pair',) if flip_pair else ()))
        sizes.append(len(got['index']))
    assert sizes == [5, 5, 2] and ld.state_dict()['epoch'] == 3
    assert not set(want_rows.tolist()) & {3, 8}                  # rows of no weight
    assert len(set(want_rows.tolist())) < N                      # with replacement: some row came twice
    assert not np.array_equal(ld.indices(3).cpu().numpy(), want_rows)


def test_one_hot_weights_name_one_row_and_no_weight_names_none(pool):
    from dsnt.data import WeightedLoader
    w = np.zeros(N, dtype=np.float32)
    w[7] = 1e-3
    ld = WeightedLoader(pool, 4, _augment(), _dev(w), seed=1)
    for got in ld:
        assert (got['index'] == 7).all().item()
    ld.set_weights(torch.zeros(N, device='cuda'))
    got = next(iter(ld))
    assert (got['index'] == -1).all().item()                     # nothing to draw: NaN samples with mask 0, no fault
    assert torch.isnan(got['input']).all().item() and (got['part_mask'] == 0).all().item()


def test_two_ranks_take_disjoint_positions_of_one_epoch(pool):
    from dsnt.data import WeightedLoader
    aug, w, B = _augment(), _dev(_w(2)), 3
    r0 = list(WeightedLoader(pool, B, aug, w, seed=8, drop_last=True, rank=0, world_size=2))
    r1 = list(WeightedLoader(pool, B, aug, w, seed=8, drop_last=True, rank=1, world_size=2))
    assert len(r0) == len(r1) == N // (2 * B) == 2
    single = list(WeightedLoader(pool, B, aug, w, seed=8, drop_last=True))
    assert len(single) == 4
    union = np.concatenate([np.concatenate([x['index'].cpu().numpy(), y['index'].cpu().numpy()]) for x, y in zip(r0, r1)])
    assert np.array_equal(union, _index(single))
    assert np.array_equal(union, sampler_ref.draw(sampler_ref.cdf(_w(2)), 8, 0, np.arange(N)))
    # rank r draws its augmentation with sample words r*B .. r*B + B-1 at its own step s, as EpochLoader's ranks do
    for s, (x, y) in enumerate(zip(r0, r1)):
        both = aug(*_rows(pool, torch.cat([x['index'], y['index']])), step=s)
        for k in ('scale', 'rot', 'hflip', 'gain'):
            assert torch.equal(both['params'][k][:B], x['params'][k]) and torch.equal(both['params'][k][B:], y['params'][k])
        assert torch.equal(both['input'][B:], y['input'])


def test_samples_per_epoch_sets_the_epoch_length(pool):
    from dsnt.data import WeightedLoader
    aug, w = _augment(), _dev(_w(3))
    want = sampler_ref.draw(sampler_ref.cdf(_w(3)), 2, 0, np.arange(30))
    keep = WeightedLoader(pool, 4, aug, w, seed=2, samples_per_epoch=30)
    batches = list(keep)
    assert len(keep) == 8 and [len(s['index']) for s in batches] == [4] * 7 + [2]
    assert np.array_equal(_index(batches), want) and np.array_equal(keep.indices(0).cpu().numpy(), want)
    drop = WeightedLoader(pool, 4, aug, w, seed=2, samples_per_epoch=30, drop_last=True)
    batches = list(drop)
    assert len(drop) == 7 and [len(s['index']) for s in batches] == [4] * 7
    assert np.array_equal(_index(batches), want[:28])
    # the augmentation's step counts this loader's batches: batch 1 of epoch 1 is step 7 + 1 of `aug`
    second = list(drop)
    assert drop.state_dict()['epoch'] == 2
    _assert_same(second[1], aug(*_rows(pool, second[1]['index']), step=8))


def test_set_weights_mid_epoch_changes_the_next_batch_only(pool):
    from dsnt.data import WeightedLoader
    aug, wa, wb = _augment(), _w(4), _w(5)
    first = sampler_ref.draw(sampler_ref.cdf(wa), 9, 0, np.arange(36))
    then = sampler_ref.draw(sampler_ref.cdf(wb), 9, 0, np.arange(36))
    assert not np.array_equal(first[12:], then[12:])
    ld = WeightedLoader(pool, 6, aug, _dev(wa), seed=9, samples_per_epoch=36)
    it = iter(ld)
    got = [next(it), next(it)]
    before = [s['index'].clone() for s in got]
    ld.set_weights(_dev(wb))
    got += list(it)
    assert np.array_equal(_index(got), np.concatenate([first[:12], then[12:]]))
    assert all(torch.equal(a, s['index']) for a, s in zip(before, got))      # batches already out are not touched
    # and the batches after the change are those of a loader that had the new weights all along
    other = list(WeightedLoader(pool, 6, aug, _dev(wb), seed=9, samples_per_epoch=36))
    for a, b in zip(got[2:], other[2:]):
        _assert_same(a, b, KEYS + ('index',))


def test_state_dict_round_trip_reproduces_the_remaining_batches(pool):
    from dsnt.data import WeightedLoader
    aug = _augment()
    ref = WeightedLoader(pool, 5, aug, _dev(_w(6)), seed=4)
    run = list(ref)                                              # epoch 0: 3 batches
    ref.set_weights(_dev(_w(7)))
    run += list(ref) + list(ref)                                 # epochs 1 and 2 on the new weights
    first = WeightedLoader(pool, 5, aug, _dev(_w(6)), seed=4)
    list(first)
    first.set_weights(_dev(_w(7)))
    it = iter(first)
    next(it)                                                     # interrupted after batch 0 of epoch 1
    state = first.state_dict()
    assert {k: v for k, v in state.items() if k != 'cdf'} == {'epoch': 1, 'batch': 1, 'seed': 4}
    assert state['cdf'].dtype == torch.int64 and state['cdf'].shape == (N,)
    assert np.array_equal(state['cdf'].cpu().numpy().view(np.uint64), sampler_ref.cdf(_w(7)))
    first.set_weights(_dev(_w(8)))                               # the state holds a copy
    assert np.array_equal(state['cdf'].cpu().numpy().view(np.uint64), sampler_ref.cdf(_w(7)))
    ld = WeightedLoader(pool, 5, aug, torch.ones(N, device='cuda'), seed=0)
    ld.load_state_dict({k: (v.cpu() if k == 'cdf' else v) for k, v in state.items()})      # as a checkpoint comes back
    resumed = list(ld) + list(ld)
    assert len(resumed) == len(run[4:]) == 5
    for a, b in zip(resumed, run[4:]):
        _assert_same(a, b, KEYS + ('index',))


def test_no_crop_sized_allocation_per_batch(pool):
    from dsnt.data import WeightedLoader
    ld = WeightedLoader(pool, 4, _augment(), _dev(_w(9)), samples_per_epoch=100)
    it = iter(ld)
    sample = next(it)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    for _ in range(20):
        sample = next(it)
    del sample
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() - base < R * R * 3, torch.cuda.memory_allocated() - base


def test_closed_loop_runs_without_host_sync(pool):
    """loader -> model -> ExampleScores.add -> weights_from_table -> set_weights, three steps of hg1 at 64 x 64."""
    from dsnt import inference, synthetic
    from dsnt.data import ExampleScores, WeightedLoader
    from dsnt.model import build_mpii_pose_model
    model = build_mpii_pose_model(base='hg1', output_strat='dsnt', reg='js')
    synthetic.fill_state_dict(model, seed=0)
    model.cuda().eval()
    aug = _augment(size=64, use_aug=False, train=False)
    ld = WeightedLoader(pool, 4, aug, torch.ones(N, device='cuda'), seed=3, samples_per_epoch=16, flip_pair=True)
    scores = ExampleScores(N)
    seen, weights = [], []

    def step(s, stamp):
        _, norm = inference.predict(model, s['input_pair'], s['transform_m'], s['transform_b'], paired=True,
                                    return_normalized=True)
        sc = scores.add(s['index'], norm, s['part_coords'], s['part_mask'], s['normalize'], s['transform_m'],
                        s['transform_b'], stamp)
        w = ExampleScores.weights_from_table(scores.table)
        ld.set_weights(w)
        seen.append(s['index'])
        weights.append(w)
        return sc

    it = iter(ld)
    with torch.no_grad():
        step(next(it), 1)                           # first pass: constants and the model's launch lists
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')     # any synchronising call inside the steps raises
        try:
            for stamp in (2, 3, 4):
                sc = step(next(it), stamp)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    assert sc.shape == (4,) and torch.isfinite(sc).all().item()
    rows = sorted(set(torch.cat(seen).cpu().tolist()))
    last = scores.last_seen().cpu().numpy()
    assert np.flatnonzero(last).tolist() == rows and 0 < len(rows) <= N
    # every re-weighting was used: the draws of step k + 1 are the restatement's on the weights of step k
    idx = [s.cpu().numpy() for s in seen]
    assert np.array_equal(idx[0], sampler_ref.draw(sampler_ref.cdf(np.ones(N, np.float32)), 3, 0, np.arange(4)))
    for k in range(1, 4):
        c = sampler_ref.cdf(weights[k - 1].cpu().numpy())
        assert np.array_equal(idx[k], sampler_ref.draw(c, 3, 0, np.arange(4 * k, 4 * k + 4))), k
    assert not torch.equal(weights[0], torch.ones(N, device='cuda'))
