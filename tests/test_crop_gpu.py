"""The device person crop on the MI355X (dsnt_crop_affine; dsnt.data.ImagePool, DeviceDataset.from_pool;
dsnt.inference.predict_boxes): the golden crops of Pillow's affine sampler bit for bit, samples without a crop, the
evaluation chain from full images against its parts, and a training set built from a pool."""
import numpy as np
import pytest
import torch

import golden_util

pytestmark = pytest.mark.gpu


def _pool(g):
    from dsnt.data import ImagePool
    n = sum(1 for k in g.files if k.startswith('img.'))
    return ImagePool.from_images([g['img.%d' % k] for k in range(n)], chunk_bytes=1 << 16)    # several chunks


def _cases(g, R=None):
    names = [str(n) for n in g['names'] if R is None or int(g[str(n) + '.R']) == R]
    idx = torch.tensor([int(g[n + '.image']) for n in names], device='cuda')
    m = torch.from_numpy(np.stack([g[n + '.matrix'] for n in names])).cuda()
    return names, idx, m


def _model():
    from dsnt import synthetic
    from dsnt.model import build_mpii_pose_model
    model = build_mpii_pose_model(base='hg1', output_strat='dsnt', reg='js')
    synthetic.fill_state_dict(model, seed=0)
    return model.cuda().eval()


def _stats():
    from dsnt import synthetic
    return synthetic.IMAGE_MEAN, (0.25, 0.26, 0.27)


def test_golden_crops_bit_exact():
    g = golden_util.load('crop')
    pool = _pool(g)
    assert len(pool) == 4 and pool.hw.tolist() == [list(g['img.%d' % k].shape[:2]) for k in range(4)]
    for R in (384, 96, 37):
        names, idx, m = _cases(g, R)
        crops, valid = pool.crop(idx, m, size=R)
        assert crops.dtype == torch.uint8 and crops.shape == (len(names), R, R, 3)
        assert valid.dtype == torch.bool and valid.all().item()
        for b, n in enumerate(names):
            want = torch.from_numpy(g[n + '.crop'])
            assert torch.equal(crops[b].cpu(), want), (n, (crops[b].cpu().int() - want.int()).abs().max().item())


def test_samples_without_a_crop():
    from dsnt import inference
    g = golden_util.load('crop')
    pool = _pool(g)
    names, idx, m = _cases(g, 96)
    B = len(names)
    bad_idx = idx.clone()
    bad_idx[1], bad_idx[4] = -1, len(pool)                                # outside the pool
    bad_m = m.clone()
    bad_m[2] = 0                                                          # singular
    bad_m[5, 0, 0] = float('nan')                                         # not finite
    out = torch.full((B, 96, 96, 3), 255, dtype=torch.uint8, device='cuda')
    valid = torch.full((B,), 7, dtype=torch.uint8, device='cuda')
    pool._crop_into(bad_idx, bad_m, out, valid)
    want_valid = [b not in (1, 2, 4, 5) for b in range(B)]
    assert valid.cpu().tolist() == [int(v) for v in want_valid]
    for b, n in enumerate(names):
        if want_valid[b]:
            assert torch.equal(out[b].cpu(), torch.from_numpy(g[n + '.crop'])), n
        else:
            assert not out[b].any().item(), b
    img = inference.predict_boxes(_model(), pool, bad_idx, bad_m, *_stats(), crop_size=96)
    ok = torch.tensor(want_valid, device='cuda')
    assert torch.isnan(img[~ok]).all().item() and torch.isfinite(img[ok]).all().item()


@pytest.mark.parametrize('flip', [True, False])
def test_predict_boxes_is_crop_then_augment_then_predict(flip):
    """On hg1 with random weights: predict_boxes equals predict on DeviceAugment of the golden crops, bit for bit, and
    its image coordinates are the fp64 back-projection inverse(M) . [n, 1] of its normalised ones."""
    from dsnt import inference
    from dsnt.data import DeviceAugment
    g = golden_util.load('crop')
    pool, model = _pool(g), _model()
    names, idx, m = _cases(g, 96)
    B = len(names)
    img, norm = inference.predict_boxes(model, pool, idx, m, *_stats(), use_flipped=flip, crop_size=96,
                                        return_normalized=True)
    assert img.dtype == torch.float64 and img.shape == (B, 16, 2) and norm.shape == (B, 16, 2)
    crops = torch.from_numpy(np.stack([g[n + '.crop'] for n in names])).cuda()
    aug = DeviceAugment(model.image_specs, *_stats(), use_aug=False, train=False)
    s = aug(crops, torch.zeros(B, 16, 2, dtype=torch.float64, device='cuda'), torch.zeros(B, 16, device='cuda'), m,
            torch.ones(B, device='cuda'), 0, flip_pair=flip)
    want_img, want_norm = inference.predict(model, s['input_pair'] if flip else s['input'],
                                            s['transform_m'].transpose(1, 2).contiguous(), s['transform_b'],
                                            use_flipped=flip, paired=flip, return_normalized=True)
    assert torch.equal(norm, want_norm)
    assert torch.equal(img, want_img)
    inv = np.linalg.inv(m.cpu().numpy())
    n = norm.double().cpu().numpy()
    back = np.einsum('bij,bkj->bki', inv[:, :2, :2], n) + inv[:, None, :2, 2]
    got = img.cpu().numpy()
    assert np.abs(got - back).max() <= 1e-12 * max(1.0, np.abs(back).max())
    # axis-aligned boxes (symmetric 2 x 2): the reference convention of predict gives the same bits untransposed
    sym = [b for b in range(B) if abs(m[b, 0, 1].item()) < 1e-15 and abs(m[b, 1, 0].item()) < 1e-15]
    assert len(sym) >= 3
    plain = inference.predict(model, s['input_pair'] if flip else s['input'], s['transform_m'], s['transform_b'],
                              use_flipped=flip, paired=flip)
    assert torch.equal(plain[sym], img[sym])


def test_pckh_on_image_pixels_equals_the_normalised_path():
    from dsnt import inference
    from dsnt.data import DeviceAugment, box_matrix
    from dsnt.evaluator import PCKhEvaluator
    g = golden_util.load('crop')
    pool, model = _pool(g), _model()
    r = np.random.default_rng(5)
    B = 12
    idx = torch.from_numpy(r.integers(0, len(pool), B)).cuda()
    hw = pool.hw.cpu().numpy()[idx.cpu().numpy()]
    center = np.stack([r.uniform(0, hw[:, 1]), r.uniform(0, hw[:, 0])], 1)
    side = r.uniform(30, 300, B)
    m = box_matrix(torch.from_numpy(center).cuda(), torch.from_numpy(side).cuda())
    kp = center[:, None, :] + r.uniform(-0.2, 0.2, (B, 16, 2)) * side[:, None, None]
    mask = (r.random((B, 16)) < 0.85).astype(np.float32)
    head = side * r.uniform(0.05, 0.4, B)
    kp_t, mask_t, head_t = (torch.from_numpy(a).cuda() for a in (kp, mask, head))
    img, norm = inference.predict_boxes(model, pool, idx, m, *_stats(), crop_size=96, return_normalized=True)
    a = PCKhEvaluator()
    a.add(img, kp_t, mask_t, head_t)
    crops, _ = pool.crop(idx, m, 96)
    s = DeviceAugment(model.image_specs, *_stats(), use_aug=False, train=False)(crops, kp_t, mask_t, m, head_t, 0)
    b = PCKhEvaluator()
    b.add_normalized(norm, s['part_coords'], mask_t, head_t, s['transform_m'], s['transform_b'])
    for k in a.meters:
        assert int(a.meters[k].count) == int(b.meters[k].count), k
        assert int(a.meters[k].hits) == int(b.meters[k].hits), k
    assert 0 < int(a.meters['all'].hits) < int(a.meters['all'].count)      # some hits, some misses


def test_from_pool_rows_and_loader_batch():
    from dsnt.data import DeviceAugment, DeviceDataset, EpochLoader, ImageSpecs
    g = golden_util.load('crop')
    pool = _pool(g)
    names, idx, m = _cases(g, 96)
    N = len(names)
    r = np.random.default_rng(3)
    mh = m.cpu().numpy()
    kp = np.einsum('bij,bkj->bki', np.linalg.inv(mh)[:, :2, :2], r.uniform(-1.1, 1.1, (N, 16, 2))) + \
        np.linalg.inv(mh)[:, None, :2, 2]
    d = DeviceDataset.from_pool(pool, idx.cpu().numpy(), mh, kp, r.random((N, 16)) < 0.8, r.uniform(40, 90, N),
                                size=96, chunk_bytes=1 << 12)
    assert len(d) == N and d.crops.shape == (N, 96, 96, 3)
    for b, n in enumerate(names):
        assert torch.equal(d.crops[b].cpu(), torch.from_numpy(g[n + '.crop'])), n
    assert torch.equal(d.matrix, m) and torch.equal(d.keypoints.cpu(), torch.from_numpy(kp))
    aug = DeviceAugment(ImageSpecs(64, True, True), *_stats(), seed=9)
    ld = EpochLoader(d, 4, aug, seed=2)
    got = next(iter(ld))
    i = got['index']
    want = aug(d.crops[i], d.keypoints[i], d.keypoint_mask[i], d.matrix[i], d.head_lengths[i], step=0)
    for k in ('input', 'part_coords', 'part_mask', 'transform_m', 'transform_b', 'normalize', 'hflip'):
        assert torch.equal(got[k], want[k]), k
    bad = idx.cpu().numpy().copy()
    bad[0] = 99
    with pytest.raises(RuntimeError, match='1 of %d rows have no crop' % N):
        DeviceDataset.from_pool(pool, bad, mh, kp, np.ones((N, 16)), np.ones(N), size=96)


def test_predict_boxes_does_not_synchronise():
    from dsnt import inference
    g = golden_util.load('crop')
    pool, model = _pool(g), _model()
    names, idx, m = _cases(g, 96)
    with torch.no_grad():
        for flip in (True, False):              # first calls: constants and the launch lists of both batch sizes
            inference.predict_boxes(model, pool, idx, m, *_stats(), use_flipped=flip, crop_size=96)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            img = inference.predict_boxes(model, pool, idx, m, *_stats(), crop_size=96)
            img2 = inference.predict_boxes(model, pool, idx, m, *_stats(), use_flipped=False, crop_size=96)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    assert torch.isfinite(img).all().item() and torch.isfinite(img2).all().item()
