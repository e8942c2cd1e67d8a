"""Per-joint heat-map statistics on the device: `dsnt_heatmap_stats` against the numpy fp64 restatement
(tests/stats_ref.py), the fused `dsnt_flip_merge_head_stats` against the launch without statistics and against the
standalone kernel on the heat-maps it stored, and `predict` / `predict_boxes` / `predict_dataset(return_stats=True)`.

The bar for fp32 sums (cov, mass, and a mean summed in another order): per row, err <= max(4 err32, 2e-6 scale), with
err32 the error of an fp32 ATen restatement of the same two-sweep formula against the fp64 reference on the same
input.  For cov, scale = max(vxx + vyy, (2/w)(2/h)) of the reference (a pixel's area is the floor of a spread); for mass
and mean, whose terms are bounded by the pixels themselves, scale = sum |p|."""
import numpy as np
import pytest
import torch

import golden_util
import stats_ref
from dsnt import synthetic

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (7, 7), (14, 14), (66, 66)]        # vector, odd-width scalar, scalar, uncached rows
TEMPS = [0.3, 1.0, 5.0, 30.0]


# ------------------------------------------------------------------ helpers
def _aten32(hm):
    """The two-sweep formula in fp32 ATen: mass, mean [.., 2], cov [.., 3]."""
    h, w = hm.shape[-2:]
    X = ((2 * torch.arange(w, device=hm.device, dtype=torch.float32) - (w - 1)) / w).view(1, w)
    Y = ((2 * torch.arange(h, device=hm.device, dtype=torch.float32) - (h - 1)) / h).view(h, 1)
    mx, my = (X * hm).sum((-2, -1)), (Y * hm).sum((-2, -1))
    dx, dy = X - mx[..., None, None], Y - my[..., None, None]
    cov = torch.stack([(dx * dx * hm).sum((-2, -1)), (dy * dy * hm).sum((-2, -1)), (dx * dy * hm).sum((-2, -1))], -1)
    return hm.sum((-2, -1)), torch.stack([mx, my], -1), cov


def _bars(hm):
    """The reference and, per row, the bars of the module docstring for cov, mass and mean."""
    h, w = hm.shape[-2:]
    ref = stats_ref.stats_ref(hm.cpu().numpy())
    m32, e32, c32 = (t.double().cpu().numpy() for t in _aten32(hm))
    scale_c = np.maximum(ref['cov'][..., 0] + ref['cov'][..., 1], (2.0 / w) * (2.0 / h))
    scale_p = np.abs(hm.double().cpu().numpy()).sum((-2, -1))
    bars = {'cov': np.maximum(4 * np.abs(c32 - ref['cov']).max(-1), 2e-6 * scale_c),
            'mass': np.maximum(4 * np.abs(m32 - ref['mass']), 2e-6 * scale_p),
            'mean': np.maximum(4 * np.abs(e32 - ref['mean']).max(-1), 2e-6 * scale_p)}
    return ref, bars


def _np(t):
    return t.double().cpu().numpy()


def _within(got, want, bar, what, extra=None):
    err = np.abs(_np(got) - want)
    if err.ndim > bar.ndim:
        err = err.max(-1)
    worst = int(np.argmax(err - bar))
    print('%s%s: worst row %d err %.3e bar %.3e' % (what, '' if extra is None else ' %s' % (extra,), worst,
                                                      err.reshape(-1)[worst], bar.reshape(-1)[worst]))
    assert (err <= bar).all(), (what, extra, worst, err.reshape(-1)[worst], bar.reshape(-1)[worst])


def _cov_image_ok(cov_image, cov, tm):
    """Within 1e-12 of the fp64 restatement on the kernel's own f32 cov, relative to the matrix' largest entry (four
    products and three sums of terms no larger than that; an entry that cancels has no relative bound of its own)."""
    want = stats_ref.cov_image(_np(cov), _np(tm)[:, None])
    got = _np(cov_image)
    tol = 1e-12 * np.abs(want).max((-2, -1), keepdims=True)
    assert (np.abs(got - want) <= tol).all(), np.abs(got - want).max()


# ------------------------------------------------------------------ 1. the standalone kernel
def _special_rows(h, w):
    """One-hot rows (corners, an interior pixel), a uniform row, and rows with tied maxima."""
    hw = h * w
    rows = torch.zeros(8, hw)
    for k, i in enumerate([0, hw - 1, w - 1, (h // 2) * w + w // 3]):
        rows[k, i] = 1.0
    rows[4] = 1.0 / hw
    rows[5, [hw // 3, hw // 3 + 1, hw - 2]] = 0.25          # three tied maxima, not in the first thread's share
    rows[5, 0] = 0.125
    rows[6, [hw - 1, hw // 2]] = 0.5
    rows[7] = 0.5 / hw
    rows[7, [5, 4, 3]] = 0.1                                # ties inside one thread's 16-byte group
    return rows.view(8, h, w)


@pytest.mark.parametrize('h,w', SIZES)
@pytest.mark.parametrize('T', TEMPS)
def test_heatmap_stats_matches_reference(h, w, T):
    import dsnt.nn as dn
    g = torch.Generator().manual_seed(int(T * 10) * 10000 + h * 100 + w)
    soft = torch.softmax((torch.randn(512, h * w, generator=g) * T).cuda(), -1).view(512, h, w)
    hm = torch.cat([soft, _special_rows(h, w).cuda()], 0).contiguous()
    st = dn.heatmap_stats(hm)
    assert st['peak'].shape == (520,) and st['mean'].shape == (520, 2) and st['cov'].shape == (520, 3)
    assert st['peak_index'].dtype == torch.int32 and not st['cov'].requires_grad
    peak, index = hm.flatten(-2).max(-1)
    assert torch.equal(st['peak'], peak)
    assert torch.equal(st['peak_index'].long(), index)
    assert torch.equal(st['mean'], dn.dsnt(hm))
    ref, bars = _bars(hm)
    assert np.array_equal(_np(st['peak']), ref['peak']) and np.array_equal(_np(st['peak_index']), ref['peak_index'])
    _within(st['cov'], ref['cov'], bars['cov'], 'cov', (h, w, T))
    _within(st['mass'], ref['mass'], bars['mass'], 'mass', (h, w, T))
    assert (st['cov'][512:516] == 0).all().item()                      # one-hot rows: exactly no spread
    assert (st['mass'][512:516] == 1).all().item()


def test_heatmap_stats_leading_dimensions_and_no_grad():
    import dsnt.nn as dn
    hm = torch.softmax(torch.randn(2, 3, 5, 12 * 12, device='cuda'), -1).view(2, 3, 5, 12, 12).requires_grad_()
    st = dn.heatmap_stats(hm)
    flat = dn.heatmap_stats(hm.detach().view(30, 12, 12))
    for k, v in st.items():
        assert v.shape[:3] == (2, 3, 5) and not v.requires_grad
        assert torch.equal(v.reshape(flat[k].shape), flat[k]), k


# ------------------------------------------------------------------ 2. the fused launch
SHAPES = [(64, 64), (32, 32), (14, 14), (7, 7), (66, 66)]     # tests/test_flipmerge_gpu.py's
HEADS = [('dsnt', 'softmax'), ('dsnt', 'thresholded_softmax'), ('dsnt', 'abs'), ('dsnt', 'relu'), ('dsnt', 'sigmoid'),
         ('gauss', 'softmax')]


@pytest.mark.parametrize('h,w', SHAPES)
@pytest.mark.parametrize('strategy,preact', HEADS)
def test_fused_stats_match_plain_launch_and_standalone_kernel(strategy, preact, h, w):
    import dsnt.nn as dn
    from dsnt import inference
    perm = inference.HFLIP_INDICES.cuda()
    g = torch.Generator().manual_seed(h * 1000 + w)
    for B in (1, 3, 5):
        L = (3 * torch.randn(2 * B, 16, h, w, generator=g)).cuda()
        tm = (torch.eye(2, dtype=torch.float64) * 150 + torch.rand(B, 2, 2, generator=g, dtype=torch.float64)).cuda()
        tb = (200 * torch.rand(B, 1, 2, generator=g, dtype=torch.float64)).cuda()
        img0, coords0, hm0 = inference.flip_merge_head(L, tm, tb, strategy, preact)
        img, coords, hm, st = inference.flip_merge_head(L, tm, tb, strategy, preact, stats=True)
        assert torch.equal(img, img0) and torch.equal(coords, coords0) and torch.equal(hm, hm0), B
        img2, coords2, none, st2 = inference.flip_merge_head(L, tm, tb, strategy, preact, heatmaps=False, stats=True)
        assert none is None and torch.equal(img2, img0) and torch.equal(coords2, coords0)
        for k in st:
            assert torch.equal(st[k], st2[k]) or (torch.isnan(st[k]).all() and torch.isnan(st2[k]).all()), (k, B)
        assert st['cov_image'].shape == (B, 16, 2, 2) and st['cov_image'].dtype == torch.float64
        alone = dn.heatmap_stats(hm)
        assert torch.equal(st['peak'], alone['peak']) and torch.equal(st['peak_index'], alone['peak_index']), B
        if strategy == 'gauss':
            merged = (L[:B] + L[B:].flip(-1).index_select(-3, perm)) / 2
            peak, index = merged.flatten(-2).max(-1)
            assert torch.equal(st['peak'], peak) and torch.equal(st['peak_index'].long(), index)
            # the decode reads the row strided by thread, the standalone kernel in groups of four: the mass to the bar
            ref, bars = _bars(merged)
            _within(st['mass'], ref['mass'], bars['mass'], 'gauss mass', (h, w, B))
            for k in ('mean', 'cov', 'cov_image'):
                assert torch.isnan(st[k]).all().item(), k
            continue
        assert torch.equal(st['mean'], coords), B                      # the dsnt coordinates, bit for bit
        if preact == 'softmax' and w % 4 == 0 and h * w <= 4096:
            # head_fwd_row sums four pixels of a heat-map row at a time for the coordinates, and normalises by a
            # multiplication that the compiler fuses into its sums (p = e / sum is not rounded first there);
            # dsnt_heatmap_stats sums the stored, rounded p in dsnt_expect_fwd's order.  The mass, the mean and the
            # covariance about that mean are held to the bar instead.
            ref, bars = _bars(hm)
            _within(st['mass'], ref['mass'], bars['mass'], 'mass', (preact, h, w, B))
            _within(st['mean'], ref['mean'], bars['mean'], 'mean', (preact, h, w, B))
            _within(st['cov'], ref['cov'], bars['cov'], 'cov', (preact, h, w, B))
        else:
            assert torch.equal(st['mass'], alone['mass']), B
            assert torch.equal(st['mean'], alone['mean']) and torch.equal(st['cov'], alone['cov']), B
        _cov_image_ok(st['cov_image'], st['cov'], tm)


# NaN pairs of one merged row, as flat indices.  Thread t reads t, t + 256, ...; a wave is 64 threads.  70 | h w - 2: two
# waves, the lower index met first by the four-wave merge; 257 | 200: wave 0 (second trip) and wave 3, the merge meets the
# HIGHER index first; 259 | 3: both trips of thread 3; 9 | 5: two lanes of one wave (the shuffle steps decide).
_NAN_PAIRS = {(64, 64): [(64 * 64 - 2, 70), (257, 200), (259, 3), (9, 5)], (12, 20): [(12 * 20 - 2, 70), (200, 130), (9, 5)]}


@pytest.mark.parametrize('h,w', sorted(_NAN_PAIRS))
def test_fused_gauss_stats_take_a_nan_as_the_peak(h, w):
    """gauss: peak and peak_index are the decode's arg-max, which is torch.max's (numpy's in stats_ref): a merged map that
    holds NaNs has peak NaN and peak_index at its FIRST NaN, wherever the two sit among threads, waves and trips, and
    decodes to pixel (0, 0).  The rows beside it keep the values they have without it."""
    from dsnt import inference
    from dsnt_oracle import util as ou
    B = 2
    g = torch.Generator().manual_seed(h * 1000 + w + 3)
    L0 = 3 * torch.randn(2 * B, 16, h, w, generator=g)
    tm = (torch.eye(2, dtype=torch.float64) * 150).expand(B, 2, 2).contiguous().cuda()
    tb = torch.zeros(B, 1, 2, dtype=torch.float64).cuda()
    clean = inference.flip_merge_head(L0.cuda(), tm, tb, 'gauss', 'softmax', stats=True)
    for pair in _NAN_PAIRS[h, w]:
        L = L0.clone()
        L[0, 3].view(-1)[list(pair)] = float('nan')                # merged row (0, 3): NaN at both indices
        L[1, 5, 0, 1] = 100.0                                       # and a plain maximum in another row
        merged = (L[:B] + L[B:].flip(-1).index_select(-3, inference.HFLIP_INDICES)) / 2
        ref = stats_ref.stats_ref(merged.numpy())
        assert np.isnan(ref['peak'][0, 3]) and ref['peak_index'][0, 3] == min(pair) and ref['peak_index'][1, 5] == 1
        for store in (True, False):
            _, coords, _, st = inference.flip_merge_head(L.cuda(), tm, tb, 'gauss', 'softmax', heatmaps=store, stats=True)
            assert np.array_equal(_np(st['peak']), ref['peak'], equal_nan=True), pair
            assert np.array_equal(_np(st['peak_index']), ref['peak_index']), (pair, int(st['peak_index'][0, 3]))
            assert torch.equal(coords.cpu(), ou.decode_heatmaps(merged)), pair
            assert ((coords[0, 3].cpu() + 1) * torch.tensor([w / 2, h / 2]) - 0.5).round().tolist() == [0.0, 0.0]
            keep = torch.ones(B, 16, dtype=torch.bool)
            keep[0, 3] = keep[1, 5] = False
            assert torch.equal(st['peak'].cpu()[keep], clean[3]['peak'].cpu()[keep])
            assert torch.equal(st['peak_index'].cpu()[keep], clean[3]['peak_index'].cpu()[keep])
            assert torch.equal(coords.cpu()[keep], clean[1].cpu()[keep])


def test_sharp_joints_score_higher_and_tighter_than_flat_ones():
    """Logits whose merged map is a sharp bump for some joints and nearly flat for the others: every sharp joint has a
    higher peak and a smaller trace(cov_image) than every flat one."""
    from dsnt import inference
    B, J, h, w = 3, 16, 64, 64
    g = torch.Generator().manual_seed(4)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    sharp = torch.rand(B, J, generator=g) < 0.5
    sharp[0, 0], sharp[0, 1] = True, False
    cy, cx = torch.rand(B, J, generator=g) * (h - 1), torch.rand(B, J, generator=g) * (w - 1)
    bump = -((ys - cy[..., None, None]) ** 2 + (xs - cx[..., None, None]) ** 2) / (2 * 1.5 ** 2)
    flat = 0.05 * torch.randn(B, J, h, w, generator=g)
    want = torch.where(sharp[..., None, None], bump, flat)
    # logits whose flip-merge is `want`: the mirrored half holds the mirrored maps under the joint permutation
    perm = inference.HFLIP_INDICES
    second = torch.empty_like(want)
    second[:, perm] = want.flip(-1)
    L = torch.cat([want, second], 0).cuda()
    tm = (torch.tensor([[120.0, 15.0], [-20.0, 90.0]], dtype=torch.float64).expand(B, 2, 2)).contiguous().cuda()
    tb = torch.zeros(B, 1, 2, dtype=torch.float64).cuda()
    _, _, hm, st = inference.flip_merge_head(L, tm, tb, 'dsnt', 'softmax', stats=True)
    assert torch.allclose(hm, torch.softmax(want.flatten(-2), -1).view_as(want).cuda(), atol=1e-6)
    s = sharp.cuda()
    trace = st['cov_image'][..., 0, 0] + st['cov_image'][..., 1, 1]
    assert st['peak'][s].min().item() > st['peak'][~s].max().item()
    assert trace[s].max().item() < trace[~s].min().item()


# ------------------------------------------------------------------ 3. predict, predict_boxes, predict_dataset
SIZE = 128


def _model(base, **kw):
    from dsnt.model import build_mpii_pose_model
    m = build_mpii_pose_model(base=base, **kw)
    if kw.get('output_strat') == 'fc':
        m.out_fc = torch.nn.Linear((SIZE // 4) ** 2, 2)       # the constructor sizes it for the canonical crop
    synthetic.fill_state_dict(m, seed=0)
    m.cuda().train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.momentum = 1.0
    x, _, _ = synthetic.batch(2, size=SIZE, seed=5, mask_p=1.0)
    with torch.no_grad():
        m(x.cuda())
    return m.eval()


@pytest.fixture(scope='module')
def models():
    return {'hg2_dsnt': _model('hg2', output_strat='dsnt', reg='js'), 'hg2_gauss': _model('hg2'),
            'resnet18_dsnt': _model('resnet18', truncate=1, output_strat='dsnt'),
            'hg1_fc': _model('hg1', output_strat='fc', preact='sigmoid')}


@pytest.fixture(scope='module')
def batch():
    B = 4
    g = torch.Generator().manual_seed(3)
    x, _, _ = synthetic.batch(B, size=SIZE, seed=21, mask_p=1.0)
    tm = torch.eye(2, dtype=torch.float64) * 140 + 20 * torch.rand(B, 2, 2, generator=g, dtype=torch.float64)
    tb = 200 * torch.rand(B, 1, 2, generator=g, dtype=torch.float64)
    return x.cuda(), tm.cuda(), tb.cuda()


def _same(a, b):
    return torch.equal(a, b) or (torch.isnan(a).all().item() and torch.isnan(b).all().item())


@pytest.mark.parametrize('flip', [True, False])
@pytest.mark.parametrize('name', ['hg2_dsnt', 'hg2_gauss', 'resnet18_dsnt', 'hg1_fc'])
def test_predict_return_stats(models, batch, name, flip):
    import dsnt.nn as dn
    from dsnt import inference
    m = models[name]
    x, tm, tb = batch
    B = x.size(0)
    img0, norm0 = inference.predict(m, x, tm, tb, use_flipped=flip, return_normalized=True)
    img, norm, st = inference.predict(m, x, tm, tb, use_flipped=flip, return_normalized=True, return_stats=True)
    assert torch.equal(img, img0) and torch.equal(norm, norm0)
    img1, st1 = inference.predict(m, x, tm, tb, use_flipped=flip, return_stats=True)
    assert torch.equal(img1, img0) and all(_same(st[k], st1[k]) for k in st)
    assert set(st) == {'peak', 'peak_index', 'mass', 'mean', 'cov', 'cov_image'}
    assert st['peak'].shape == (B, 16) and st['mean'].shape == (B, 16, 2) and st['cov'].shape == (B, 16, 3)
    assert st['cov_image'].shape == (B, 16, 2, 2) and st['cov_image'].dtype == torch.float64
    # the statistics describe the map the coordinates come from: the merged one with flip, else the LAST stack's
    hg = name.startswith('hg')
    the_map = m.heatmaps if flip and not name.endswith('fc') else (m.heatmaps_array[-1] if hg else m.heatmaps)
    alone = dn.heatmap_stats(the_map)
    assert torch.equal(st['peak'], alone['peak']) and torch.equal(st['peak_index'], alone['peak_index'])
    if name.endswith('gauss'):
        for k in ('mean', 'cov', 'cov_image'):
            assert torch.isnan(st[k]).all().item(), k
        # the decoded coordinates are the arg-max pixel of the 32 x 32 map (+- a quarter pixel) where the peak is positive
        px, py = (norm[..., 0] + 1) * 16 - 0.5, (norm[..., 1] + 1) * 16 - 0.5
        pos = st['peak'] > 0
        assert ((st['peak_index'] % 32 - px).abs() <= 0.26)[pos].all().item()
        assert ((st['peak_index'] // 32 - py).abs() <= 0.26)[pos].all().item()
        return
    assert torch.isfinite(st['cov_image']).all().item()
    _cov_image_ok(st['cov_image'], st['cov'], tm)
    if name.endswith('fc'):
        assert torch.equal(st['mean'], alone['mean'])       # the map's expectation, not the linear layer's prediction
        return
    if flip:
        assert torch.equal(st['mean'], norm)
    else:
        assert torch.equal(st['mean'], alone['mean']) and torch.equal(st['cov'], alone['cov'])
        assert (st['mean'] - norm).abs().max().item() <= 2e-6
        if name == 'hg2_dsnt':                                # `model.heatmaps` is the FIRST stack's: not the map to describe
            first = dn.heatmap_stats(m.heatmaps)
            assert (first['mean'] - norm).abs().max().item() > 1e-4


def test_predict_dataset_return_stats(models, batch):
    from dsnt import inference
    m = models['hg2_dsnt']
    x, tm, tb = batch
    data = [{'input': x[i].cpu(), 'transform_m': tm[i].cpu(), 'transform_b': tb[i].cpu()} for i in range(x.size(0))]
    plain = inference.predict_dataset(m, data, batch_size=3)
    preds, st = inference.predict_dataset(m, data, batch_size=3, return_stats=True)
    assert torch.equal(preds, plain) and not preds.is_cuda
    for k, v in st.items():
        assert not v.is_cuda and v.shape[:2] == (4, 16), k
    want = torch.cat([inference.predict(m, x[i:i + 3], tm[i:i + 3], tb[i:i + 3], return_stats=True)[1]['cov_image']
                      for i in (0, 3)], 0)
    assert torch.equal(st['cov_image'], want.cpu())
    assert (st['peak'] > 0).all().item() and (st['mass'] - 1).abs().max().item() <= 1e-5


def _pool_and_cases():
    from dsnt.data import ImagePool
    g = golden_util.load('crop')
    n = sum(1 for k in g.files if k.startswith('img.'))
    pool = ImagePool.from_images([g['img.%d' % k] for k in range(n)], chunk_bytes=1 << 16)
    names = [str(k) for k in g['names'] if int(g[str(k) + '.R']) == 96]
    idx = torch.tensor([int(g[k + '.image']) for k in names], device='cuda')
    mat = torch.from_numpy(np.stack([g[k + '.matrix'] for k in names])).cuda()
    return pool, idx, mat


@pytest.mark.parametrize('flip', [True, False])
def test_predict_boxes_return_stats_and_an_invalid_box(flip):
    from dsnt import inference
    from dsnt.model import build_mpii_pose_model
    model = build_mpii_pose_model(base='hg1', output_strat='dsnt', reg='js')
    synthetic.fill_state_dict(model, seed=0)
    model.cuda().eval()
    pool, idx, mat = _pool_and_cases()
    norm_stats = (synthetic.IMAGE_MEAN, (0.25, 0.26, 0.27))
    B = idx.numel()
    img0 = inference.predict_boxes(model, pool, idx, mat, *norm_stats, use_flipped=flip, crop_size=96)
    img, st = inference.predict_boxes(model, pool, idx, mat, *norm_stats, use_flipped=flip, crop_size=96,
                                      return_stats=True)
    assert torch.equal(img, img0)
    assert all(torch.isfinite(v.double()).all().item() for v in st.values())
    # cov_image in the image's pixels for any box matrix: inverse(M)'s 2 x 2 part A maps n to pixels as A n
    A = np.linalg.inv(mat.cpu().numpy())[:, :2, :2]
    want = stats_ref.cov_image(_np(st['cov']), np.swapaxes(A, 1, 2)[:, None])
    assert (np.abs(_np(st['cov_image']) - want) <= 1e-11 * np.abs(want).max((-2, -1), keepdims=True)).all()
    bad = idx.clone()
    bad[2] = len(pool)
    img_b, st_b = inference.predict_boxes(model, pool, bad, mat, *norm_stats, use_flipped=flip, crop_size=96,
                                          return_stats=True)
    ok = torch.ones(B, dtype=torch.bool, device='cuda')
    ok[2] = False
    # NaN in that row only.  (The other rows are not compared with the call above bit for bit: the backbone scales its
    # fp16x3 operands by bounds taken over the whole batch, so another sample's crop moves their last bits.)
    assert torch.isnan(img_b[2]).all().item() and torch.isfinite(img_b[ok]).all().item()
    for k, v in st_b.items():
        if k == 'peak_index':
            assert (v[2] == -1).all().item() and (v[ok] >= 0).all().item()
        else:
            assert torch.isnan(v[2]).all().item() and torch.isfinite(v[ok]).all().item(), k


def test_return_stats_does_not_synchronise(models, batch):
    from dsnt import inference
    m = models['hg2_dsnt']
    x, tm, tb = batch
    pool, idx, mat = _pool_and_cases()
    norm_stats = (synthetic.IMAGE_MEAN, (0.25, 0.26, 0.27))

    def run():
        out = [inference.predict(m, x, tm, tb, use_flipped=f, return_stats=True) for f in (True, False)]
        out += [inference.predict_boxes(m, pool, idx, mat, *norm_stats, use_flipped=f, crop_size=96, return_stats=True)
                for f in (True, False)]
        return out
    with torch.no_grad():
        run()                                        # first calls: constants and launch lists are set up
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')      # any synchronising call raises
        try:
            out = run()
        finally:
            torch.cuda.set_sync_debug_mode('default')
    for img, st in out:
        assert torch.isfinite(img).all().item() and torch.isfinite(st['cov_image']).all().item()
