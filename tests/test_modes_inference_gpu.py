"""`predict`, `predict_boxes` and `predict_dataset` with the mode-seeking read-out (`readout='mode'`, `return_modes=True`):
the default read-out keeps its bits, the mode read-out is mode 0 of `nn.heatmap_modes` on the map the prediction comes
from, and on a bimodal map it lands on the dominant bump where the expectation lands between the two."""
import numpy as np
import pytest
import torch

import golden_util
import modes_ref as ref
from dsnt import synthetic

pytestmark = pytest.mark.gpu

SIZE = 128          # 32 x 32 heat-maps


def _model(**kw):
    from dsnt.model import build_mpii_pose_model
    m = build_mpii_pose_model(base='hg1', **kw)
    if kw.get('output_strat') == 'fc':
        m.out_fc = torch.nn.Linear((SIZE // 4) ** 2, 2)       # the constructor sizes it for the canonical crop
    synthetic.fill_state_dict(m, seed=0)
    return m.cuda().eval()


@pytest.fixture(scope='module')
def models():
    return {'dsnt': _model(output_strat='dsnt', reg='js'), 'gauss': _model(),
            'fc': _model(output_strat='fc', preact='sigmoid')}


@pytest.fixture(scope='module')
def batch():
    B = 2
    g = torch.Generator().manual_seed(3)
    x, _, _ = synthetic.batch(B, size=SIZE, seed=21, mask_p=1.0)
    tm = torch.eye(2, dtype=torch.float64) * 140 + 20 * torch.rand(B, 2, 2, generator=g, dtype=torch.float64)
    tb = 200 * torch.rand(B, 1, 2, generator=g, dtype=torch.float64)
    return x.cuda(), tm.cuda(), tb.cuda()


def _same(a, b):
    return torch.equal(a, b) or (torch.equal(torch.isnan(a), torch.isnan(b)) and
                                 torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)]))


def _the_map(m):
    return m.heatmaps_array[-1]


@pytest.mark.parametrize('flip', [True, False])
@pytest.mark.parametrize('name', ['dsnt', 'gauss'])
def test_mean_readout_keeps_its_bits_and_mode_readout_is_mode_zero(models, batch, name, flip):
    import dsnt.nn as dn
    from dsnt import inference
    m = models[name]
    x, tm, tb = batch
    img0, norm0, st0 = inference.predict(m, x, tm, tb, use_flipped=flip, return_normalized=True, return_stats=True)
    hm0 = m.heatmaps.clone()
    img1, norm1, st1 = inference.predict(m, x, tm, tb, use_flipped=flip, return_normalized=True, return_stats=True,
                                         readout='mean', mode_radius=2)
    assert torch.equal(img1, img0) and torch.equal(norm1, norm0) and torch.equal(m.heatmaps, hm0)
    assert set(st1) == set(st0) and all(_same(st1[k], st0[k]) for k in st0)
    assert torch.equal(inference.predict(m, x, tm, tb, use_flipped=flip, readout='mean'), img0)

    for radius in (3, 1):
        img, norm, st = inference.predict(m, x, tm, tb, use_flipped=flip, return_normalized=True, return_stats=True,
                                          readout='mode', mode_radius=radius)
        assert torch.equal(m.heatmaps, hm0)
        want = dn.heatmap_modes(_the_map(m), radius, 1, tm, tb)
        # (bit for bit; a raw 'gauss' map has joints without a positive window, NaN in both)
        assert _same(norm, want['coords'][:, :, 0]) and _same(img, want['image'][:, :, 0])
        assert norm.shape == norm0.shape and img.shape == img0.shape and img.dtype == torch.float64
        assert norm.is_contiguous() and img.is_contiguous()
        # the statistics describe the map, not the read-out: the same keys, the same bits
        assert set(st) == {'peak', 'peak_index', 'mass', 'mean', 'cov', 'cov_image'}
        assert all(_same(st[k], st0[k]) for k in st0)
    if name == 'dsnt':                                        # (a raw 'gauss' map may have no positive window: NaN by definition)
        assert torch.isfinite(img).all().item()
        assert not torch.equal(norm, norm0)                   # another read-out of the same map

    # return_modes: the two dominant modes, after the statistics dict; the same launch serves the read-out
    img2, st2, modes = inference.predict(m, x, tm, tb, use_flipped=flip, return_stats=True, return_modes=True)
    assert torch.equal(img2, img0) and all(_same(st2[k], st0[k]) for k in st0)
    two = dn.heatmap_modes(_the_map(m), 3, 2, tm, tb)
    assert set(modes) == {'coords', 'mass', 'index', 'image'} and all(_same(modes[k], two[k]) for k in two)
    assert modes['coords'].shape == (2, 16, 2, 2) and modes['mass'].shape == (2, 16, 2)
    img3, modes3 = inference.predict(m, x, tm, tb, use_flipped=flip, readout='mode', return_modes=True)
    assert _same(img3, two['image'][:, :, 0]) and all(_same(modes3[k], two[k]) for k in two)
    assert (modes['index'][:, :, 0] >= 0).all().item()


@pytest.mark.parametrize('flip', [True, False])
def test_fc_strategy(models, batch, flip):
    """Its prediction does not come from the map: the mode read-out is refused; the modes of its map can still be returned."""
    import dsnt.nn as dn
    from dsnt import inference
    m = models['fc']
    x, tm, tb = batch
    with pytest.raises(ValueError, match="'fc' strategy"):
        inference.predict(m, x, tm, tb, use_flipped=flip, readout='mode')
    img0 = inference.predict(m, x, tm, tb, use_flipped=flip)
    img, modes = inference.predict(m, x, tm, tb, use_flipped=flip, return_modes=True)
    assert torch.equal(img, img0)
    assert all(_same(v, dn.heatmap_modes(_the_map(m), 3, 2, tm, tb)[k]) for k, v in modes.items())


def test_mode_readout_does_not_synchronise(models, batch):
    from dsnt import inference
    x, tm, tb = batch

    def run():
        return [inference.predict(models[n], x, tm, tb, use_flipped=f, readout='mode', return_modes=True)
                for n in ('dsnt', 'gauss') for f in (True, False)]
    with torch.no_grad():
        run()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')      # any synchronising call raises
        try:
            out = run()
        finally:
            torch.cuda.set_sync_debug_mode('default')
    assert all(torch.isfinite(img).all().item() for img, _ in out[:2])         # the 'dsnt' model's


def test_predict_dataset_passes_the_keywords_through(models, batch):
    from dsnt import inference
    m = models['dsnt']
    x, tm, tb = batch
    data = [{'input': x[i].cpu(), 'transform_m': tm[i].cpu(), 'transform_b': tb[i].cpu()} for i in range(x.size(0))]
    plain = inference.predict_dataset(m, data, batch_size=1)
    assert torch.equal(inference.predict_dataset(m, data, batch_size=1, readout='mean'), plain)
    preds, st, modes = inference.predict_dataset(m, data, batch_size=1, return_stats=True, readout='mode',
                                                 mode_radius=2, return_modes=True)
    assert not preds.is_cuda and preds.shape == plain.shape and set(st) == {'peak', 'peak_index', 'mass', 'mean', 'cov',
                                                                            'cov_image'}
    want = [inference.predict(m, x[i:i + 1], tm[i:i + 1], tb[i:i + 1], readout='mode', mode_radius=2, return_modes=True)
            for i in range(x.size(0))]
    assert torch.equal(preds, torch.cat([w[0] for w in want], 0).cpu())
    for k, v in modes.items():
        assert not v.is_cuda and _same(v, torch.cat([w[1][k] for w in want], 0).cpu()), k
    preds2, modes2 = inference.predict_dataset(m, data, batch_size=1, return_modes=True)
    assert torch.equal(preds2, plain) and set(modes2) == set(modes)
    assert inference.predict_dataset(m, [], return_modes=True)[1] == {}


@pytest.mark.parametrize('flip', [True, False])
def test_predict_boxes_masks_a_sample_without_a_crop(models, flip):
    from dsnt import inference
    from dsnt.data import ImagePool
    g = golden_util.load('crop')
    n = sum(1 for k in g.files if k.startswith('img.'))
    pool = ImagePool.from_images([g['img.%d' % k] for k in range(n)], chunk_bytes=1 << 16)
    names = [str(k) for k in g['names'] if int(g[str(k) + '.R']) == 96]
    idx = torch.tensor([int(g[k + '.image']) for k in names], device='cuda')
    mat = torch.from_numpy(np.stack([g[k + '.matrix'] for k in names])).cuda()
    norm_stats = (synthetic.IMAGE_MEAN, (0.25, 0.26, 0.27))
    m = models['dsnt']
    B = idx.numel()
    img0 = inference.predict_boxes(m, pool, idx, mat, *norm_stats, use_flipped=flip, crop_size=96)
    assert torch.equal(inference.predict_boxes(m, pool, idx, mat, *norm_stats, use_flipped=flip, crop_size=96,
                                               readout='mean'), img0)
    bad = idx.clone()
    bad[2] = len(pool)
    img, norm, st, modes = inference.predict_boxes(m, pool, bad, mat, *norm_stats, use_flipped=flip, crop_size=96,
                                                   return_normalized=True, return_stats=True, readout='mode',
                                                   return_modes=True)
    ok = torch.ones(B, dtype=torch.bool, device='cuda')
    ok[2] = False
    assert torch.isnan(img[2]).all().item() and torch.isfinite(img[ok]).all().item()
    assert torch.isnan(norm[2]).all().item() and torch.isfinite(norm[ok]).all().item()
    assert (st['peak_index'][2] == -1).all().item() and torch.isnan(st['peak'][2]).all().item()
    assert set(modes) == {'coords', 'mass', 'index', 'image'}
    for k, v in modes.items():
        if k == 'index':
            assert (v[2] == -1).all().item() and (v[ok][:, :, 0] >= 0).all().item()
        else:
            assert torch.isnan(v[2]).all().item() and torch.isfinite(v[ok][:, :, 0]).all().item(), k
    # the read-out of the valid samples is mode 0 of the returned modes
    assert torch.equal(img[ok], modes['image'][ok][:, :, 0]) and torch.equal(norm[ok], modes['coords'][ok][:, :, 0])


def test_mode_readout_hits_the_dominant_bump_where_the_mean_lands_between():
    """The bimodal map of DESIGN §22 (two sigma = 1 px bumps, weights 0.6 and 0.4, 24.3 px apart on 64 x 64), as every joint
    of a batch and mirrored, through `nn.heatmap_modes` and `nn.dsnt` on the constructed map."""
    import dsnt.nn as dn
    p = ref.bimodal()
    hm = torch.from_numpy(np.stack([p, p[:, ::-1].copy()])).cuda().view(2, 1, 64, 64)
    modes = dn.heatmap_modes(hm, 3, 2)
    mean = dn.dsnt(hm)
    px = lambda c: ((c.double() + 1) * 64 - 1) / 2            # normalised -> pixels
    centre = torch.tensor([[20.3, 30.7], [63 - 20.3, 30.7]], device='cuda', dtype=torch.float64).view(2, 1, 2)
    runner = torch.tensor([[44.6, 31.2], [63 - 44.6, 31.2]], device='cuda', dtype=torch.float64).view(2, 1, 2)
    d_mode = (px(modes['coords'][:, :, 0]) - centre).norm(dim=-1)
    d_next = (px(modes['coords'][:, :, 1]) - runner).norm(dim=-1)
    d_mean = (px(mean) - centre).norm(dim=-1)
    print('mode 0 off by %.4f px, mode 1 by %.4f px, the mean by %.2f px' % (d_mode.max(), d_next.max(), d_mean.min()))
    assert d_mode.max().item() < 0.05 and d_next.max().item() < 0.05
    assert d_mean.min().item() > 5.0
    assert (modes['mass'][:, :, 0] - 0.5994).abs().max().item() < 1e-4
    assert (modes['mass'][:, :, 1] - 0.3996).abs().max().item() < 1e-4
