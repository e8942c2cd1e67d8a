"""The device-resident training set on the MI355X (dsnt.data.DeviceDataset, EpochLoader; csrc/augment.hip): the device
epoch order equals its numpy restatement (tests/loader_ref.py), the gather kernels equal DeviceAugment on the gathered
batch bit for bit, an epoch visits every row once and ranks shard it disjointly, a resumed loader repeats the
uninterrupted batches, and a training step and a validation pass run from it without a host synchronisation."""
import numpy as np
import pytest
import torch

import golden_util
import loader_ref

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 7, 64, 65, 1000, 4097, 25000)
KEYS = ('input', 'part_coords', 'part_mask', 'transform_m', 'transform_b', 'normalize', 'hflip')


def _device_order(n, seed, epoch, first, count, shuffle=True):
    from dsnt import _lib
    out = torch.empty(count, dtype=torch.int64, device='cuda')
    _lib.call('dsnt_epoch_indices', n, seed, epoch, first, count, int(shuffle), _lib.ptr(out))
    return out.cpu().numpy()


def _arrays(N, R=96, J=16, seed=0):
    """A synthetic training set as host arrays (crops, keypoints, keypoint_mask, matrix, head_lengths)."""
    r = np.random.default_rng(seed)
    side = r.uniform(150, 500, N)
    m = np.zeros((N, 3, 3))
    m[:, 0, 0] = m[:, 1, 1] = 2 / side
    m[:, 0, 2], m[:, 1, 2], m[:, 2, 2] = -2 * r.uniform(300, 900, N) / side, -2 * r.uniform(200, 600, N) / side, 1
    kp = (r.uniform(-1.2, 1.2, (N, J, 2)) - m[:, None, :2, 2]) / m[:, None, 0:1, 0]
    return (r.integers(0, 256, (N, R, R, 3), dtype=np.uint8), kp, (r.random((N, J)) < 0.8).astype(np.float32), m,
            r.uniform(40, 120, N))


def _dataset(N, R=96, seed=0):
    from dsnt.data import DeviceDataset
    return DeviceDataset.from_arrays(*_arrays(N, R, seed=seed), chunk_bytes=1 << 20)     # several chunks


def _augment(use_aug=True, train=True, S=64, seed=17):
    from dsnt.data import DeviceAugment, ImageSpecs
    return DeviceAugment(ImageSpecs(S, True, True), (0.44, 0.44, 0.40), (0.25, 0.26, 0.27), use_aug=use_aug,
                         train=train, seed=seed)


def _rows(d, idx):
    i = torch.as_tensor(idx, device='cuda')
    return d.crops[i], d.keypoints[i], d.keypoint_mask[i], d.matrix[i], d.head_lengths[i]


def _assert_same(a, b, keys=KEYS):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert torch.equal(a[k], b[k]), (k, (a[k].double() - b[k].double()).abs().max().item())
    for k in ('scale', 'rot', 'hflip', 'gain'):
        assert torch.equal(a['params'][k], b['params'][k]), k


@pytest.mark.parametrize('n', SIZES)
def test_device_order_equals_numpy_restatement(n):
    for seed, epoch in ((0, 0), (7, 3), (0xDEADBEEFCAFEF00D, 2 ** 33 + 1)):
        want = loader_ref.order(n, seed, epoch)
        assert np.array_equal(_device_order(n, seed, epoch, 0, n), want), (n, seed, epoch)
        first = n // 3
        count = max(1, min(n - first, 1000))
        assert np.array_equal(_device_order(n, seed, epoch, first, count), want[first:first + count]), (n, first)
        assert np.array_equal(_device_order(n, seed, epoch, 0, n, shuffle=False), np.arange(n))


@pytest.mark.parametrize('flip_pair', [False, True])
@pytest.mark.parametrize('train', [True, False])
def test_loader_batches_equal_device_augment_on_gathered_rows(flip_pair, train):
    """Drawn parameters: each EpochLoader batch is DeviceAugment on crops[index] at the global step, bit for bit."""
    from dsnt.data import EpochLoader
    d = _dataset(37)
    aug = _augment(train=train)
    ld = EpochLoader(d, 8, aug, seed=5, flip_pair=flip_pair)
    ld.set_epoch(2)
    n_batches = 0
    for s, got in enumerate(ld):
        want = aug(*_rows(d, got['index']), step=2 * len(ld) + s, flip_pair=flip_pair)
        _assert_same(got, want, KEYS + (('input_pair',) if flip_pair else ()))
        assert got['index'].dtype == torch.int64
        n_batches += 1
    assert n_batches == 5 and ld.state_dict()['epoch'] == 3


def _gather_pinned(d, aug, idx, params, step, flip_pair):
    """The gather entry points with pinned parameters (draw = 0), called directly."""
    from dsnt import _lib
    B = idx.numel()
    S = aug.image_specs.size
    mean, std, flip = aug._consts(d.device)
    p = [params[k].clone() for k in ('scale', 'rot', 'hflip', 'gain')]
    pair = torch.empty(2 * B if flip_pair else B, 3, S, S, device='cuda')
    name = 'dsnt_augment_fwd_pair_gather' if flip_pair else 'dsnt_augment_fwd_gather'
    _lib.call(name, _lib.ptr(d.crops), len(d), _lib.ptr(idx), B, d.crops.shape[1], S, *map(_lib.ptr, p), 0, aug.seed,
              step, 0, _lib.ptr(mean), _lib.ptr(std), _lib.ptr(pair))
    J = d.keypoints.shape[1]
    out = {'input': pair[:B], 'part_coords': torch.empty(B, J, 2, device='cuda'),
           'part_mask': torch.empty(B, J, device='cuda'),
           'transform_m': torch.empty(B, 2, 2, dtype=torch.float64, device='cuda'),
           'transform_b': torch.empty(B, 1, 2, dtype=torch.float64, device='cuda'),
           'normalize': torch.empty(B, dtype=torch.float64, device='cuda')}
    _lib.call('dsnt_augment_keypoints_gather', _lib.ptr(d.matrix), _lib.ptr(d.keypoints), _lib.ptr(d.keypoint_mask),
              _lib.ptr(d.head_lengths), len(d), _lib.ptr(idx), B, J, *map(_lib.ptr, p[:3]), _lib.ptr(flip),
              1 if aug.train else 0, *(_lib.ptr(out[k]) for k in ('part_coords', 'part_mask', 'transform_m',
                                                                  'transform_b', 'normalize')))
    out['hflip'] = p[2].bool()
    out['params'] = dict(zip(('scale', 'rot', 'hflip', 'gain'), p))
    if flip_pair:
        out['input_pair'] = pair
    return out


@pytest.mark.parametrize('flip_pair', [False, True])
@pytest.mark.parametrize('train', [True, False])
def test_pinned_params_gather_equals_device_augment(flip_pair, train):
    d = _dataset(23, seed=1)
    aug = _augment(train=train)
    idx = torch.tensor([22, 0, 5, 5, 17, 3, 9], device='cuda')        # repeats allowed
    params = aug(*_rows(d, idx), step=11)['params']                       # some rotations, flips and scales
    got = _gather_pinned(d, aug, idx, params, 11, flip_pair)
    want = aug(*_rows(d, idx), step=0, params=params, flip_pair=flip_pair)
    _assert_same(got, want, KEYS + (('input_pair',) if flip_pair else ()))


def test_golden_cases_packed_in_shuffled_order():
    """tests/golden/augment.npz's cases (R = 384, pinned parameters, rotated ones included) as a pool in a shuffled
    order: the gather kernels equal DeviceAugment on the contiguous batch, which the augment tests hold to the golden."""
    from dsnt.data import DeviceAugment, DeviceDataset, ImageSpecs
    g = golden_util.load('augment')
    by_s = {}
    for n in g['names']:
        by_s.setdefault(int(g[str(n) + '.S']), []).append(str(n))
    for S, names in by_s.items():
        perm = np.random.default_rng(S).permutation(len(names))
        pooled = [names[i] for i in perm]                                 # row r of the pool = case pooled[r]
        st = lambda k, ns: np.stack([np.asarray(g[n + '.' + k]) for n in ns])
        d = DeviceDataset.from_arrays(st('src', pooled), st('keypoints', pooled), st('keypoint_mask', pooled),
                                      st('matrix', pooled), np.linspace(50, 90, len(pooled)), chunk_bytes=1 << 20)
        idx = torch.from_numpy(np.argsort(perm)).cuda()                  # batch b = case names[b]
        aug = DeviceAugment(ImageSpecs(S, True, True), g['mean'], g['std'])
        params = {k: torch.from_numpy(st(k, names)).cuda() for k in ('scale', 'rot', 'hflip', 'gain')}
        for pair in (False, True):
            got = _gather_pinned(d, aug, idx, params, 0, pair)
            want = aug(*_rows(d, idx), step=0, params=params, flip_pair=pair)
            _assert_same(got, want, KEYS + (('input_pair',) if pair else ()))


def test_epoch_visits_every_row_once():
    from dsnt.data import EpochLoader
    n, B = 37, 8
    d = _dataset(n)
    aug = _augment()
    ld = EpochLoader(d, B, aug, seed=3)
    rows = torch.cat([s['index'] for s in ld]).cpu().numpy()
    assert [len(s['index']) for s in EpochLoader(d, B, aug, seed=3)] == [8, 8, 8, 8, 5]
    assert np.array_equal(np.sort(rows), np.arange(n))
    assert np.array_equal(rows, loader_ref.order(n, 3, 0))
    assert np.array_equal(ld.indices(0).cpu().numpy(), rows)
    second = torch.cat([s['index'] for s in ld]).cpu().numpy()            # the next epoch: another order
    assert np.array_equal(np.sort(second), np.arange(n)) and not np.array_equal(second, rows)
    dl = EpochLoader(d, B, aug, seed=3, drop_last=True)
    kept = torch.cat([s['index'] for s in dl]).cpu().numpy()
    assert len(kept) == (n // B) * B and len(set(kept.tolist())) == (n // B) * B
    plain = torch.cat([s['index'] for s in EpochLoader(d, B, aug, shuffle=False)]).cpu().numpy()
    assert np.array_equal(plain, np.arange(n))


def test_two_ranks_shard_one_epoch():
    from dsnt.data import EpochLoader
    n, B = 41, 5
    d = _dataset(n)
    aug = _augment()
    r0 = list(EpochLoader(d, B, aug, seed=8, drop_last=True, rank=0, world_size=2))
    r1 = list(EpochLoader(d, B, aug, seed=8, drop_last=True, rank=1, world_size=2))
    assert len(r0) == len(r1) == n // (2 * B)
    a = torch.cat([s['index'] for s in r0]).cpu().numpy()
    b = torch.cat([s['index'] for s in r1]).cpu().numpy()
    assert not set(a.tolist()) & set(b.tolist())
    order = loader_ref.order(n, 8, 0)
    union = np.concatenate([np.concatenate([x, y]) for x, y in zip(a.reshape(-1, B), b.reshape(-1, B))])
    assert np.array_equal(union, order[:len(union)])
    for x, y in zip(r0, r1):
        assert not torch.equal(x['params']['scale'], y['params']['scale'])
        assert not torch.equal(x['params']['gain'], y['params']['gain'])
    # rank r draws sample words r*B .. r*B + B-1: the second half of one DeviceAugment batch of 2B at the same step
    for s, (x, y) in enumerate(zip(r0, r1)):
        both = aug(*_rows(d, torch.cat([x['index'], y['index']])), step=s)
        for k in ('scale', 'rot', 'hflip', 'gain'):
            assert torch.equal(both['params'][k][:B], x['params'][k]), k
            assert torch.equal(both['params'][k][B:], y['params'][k]), k
        assert torch.equal(both['input'][B:], y['input'])


def test_resume_reproduces_the_uninterrupted_batches():
    from dsnt.data import EpochLoader
    d = _dataset(29)
    aug = _augment()
    ref = EpochLoader(d, 6, aug, seed=4)
    run = [s for _ in range(3) for s in ref]                             # epochs 0..2, 5 batches each
    first = EpochLoader(d, 6, aug, seed=4)
    list(first)                                                          # epoch 0
    it = iter(first)
    next(it), next(it)                                                   # interrupted after batch 1 of epoch 1
    state = first.state_dict()
    assert state == {'epoch': 1, 'batch': 2, 'seed': 4}
    ld = EpochLoader(d, 6, aug, seed=0)
    ld.load_state_dict(state)
    resumed = list(ld) + list(ld)
    assert len(resumed) == len(run[7:]) == 8
    for a, b in zip(resumed, run[7:]):
        _assert_same(a, b, KEYS + ('index',))


def test_training_step_and_validation_pass_without_host_sync():
    from dsnt import inference, synthetic
    from dsnt.data import DeviceAugment, DeviceDataset, EpochLoader
    from dsnt.evaluator import PCKhEvaluator
    from dsnt.model import build_mpii_pose_model
    model = build_mpii_pose_model(base='hg1', output_strat='dsnt', reg='js')
    synthetic.fill_state_dict(model, seed=0)
    model.cuda().train()
    specs = model.image_specs
    d = DeviceDataset.from_arrays(*_arrays(20, R=384, seed=2))
    train = EpochLoader(d, 8, DeviceAugment(specs, synthetic.IMAGE_MEAN, (1, 1, 1), seed=5), seed=1)
    it = iter(train)
    next(it)                                        # first batch: per-device constants are uploaded once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')         # any synchronising call inside the loader raises
    try:
        sample = next(it)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert sample['input'].shape == (8, 3, specs.size, specs.size)
    out = model(sample['input'])
    loss = model.forward_loss(out, sample['part_coords'], sample['part_mask'])
    loss.backward()
    assert torch.isfinite(loss).item()

    model.eval()
    val = EpochLoader(d, 8, DeviceAugment(specs, synthetic.IMAGE_MEAN, (1, 1, 1), use_aug=False, train=False),
                      shuffle=False, flip_pair=True)
    ev = PCKhEvaluator()

    def step(s):
        img, norm = inference.predict(model, s['input_pair'], s['transform_m'], s['transform_b'], paired=True,
                                      return_normalized=True)
        ev.add_normalized(norm, s['part_coords'], s['part_mask'], s['normalize'], s['transform_m'], s['transform_b'])
        return img
    with torch.no_grad():
        for s in val:                               # first pass: constants and launch lists of both batch sizes
            step(s)
        torch.cuda.synchronize()
        val.set_epoch(0)
        torch.cuda.set_sync_debug_mode('error')
        try:
            for s in val:                           # two full batches and the final partial one (4 samples)
                img = step(s)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    assert img.shape == (4, 16, 2) and torch.isfinite(img).all().item()
    assert torch.equal(s['index'], torch.arange(16, 20, device='cuda'))


def test_no_crop_sized_allocation_per_batch():
    from dsnt.data import EpochLoader
    B, R = 16, 384
    d = _dataset(11 * B, R=R)
    ld = EpochLoader(d, B, _augment(S=256))
    it = iter(ld)
    sample = next(it)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    for _ in range(10):
        sample = next(it)
    del sample
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() - base < B * R * R * 3, torch.cuda.memory_allocated() - base


def test_save_and_load_round_trip(tmp_path):
    from dsnt.data import DeviceDataset
    d = _dataset(11, R=40)
    d.save(str(tmp_path))
    e = DeviceDataset.load(str(tmp_path), chunk_bytes=1 << 12)
    for k in ('crops', 'keypoints', 'keypoint_mask', 'matrix', 'head_lengths'):
        assert torch.equal(getattr(d, k), getattr(e, k)), k
    assert len(e) == 11 and e.nbytes == d.nbytes == 11 * (40 * 40 * 3 + 16 * 2 * 8 + 16 * 4 + 9 * 8 + 8)
    host = _arrays(11, R=40)
    assert np.array_equal(np.load(str(tmp_path / 'crops.npy')), host[0])
