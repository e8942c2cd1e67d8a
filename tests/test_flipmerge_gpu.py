"""Batched flip-augmented evaluation on the device: the fused `dsnt_flip_merge_head` against the ATen merge and the
model's own head, `inference.predict` at batch B against the reference-shaped batch-1 loop and the oracle, the
mirrored twin of `DeviceAugment(flip_pair=True)`, and the absence of host synchronisation."""
import numpy as np
import pytest
import torch

from dsnt import synthetic

pytestmark = pytest.mark.gpu

SIZE = 128          # hg1 at 128 px: 32x32 heat-maps


def _dataset(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        x, _, _ = synthetic.batch(1, size=size, seed=seed + i, mask_p=1.0)
        m = torch.eye(2, dtype=torch.float64) * (100.0 + 10 * i) + 3.0 * torch.rand(2, 2, generator=g, dtype=torch.float64)
        b = 200.0 * torch.rand(1, 2, generator=g, dtype=torch.float64)
        out.append({'input': x[0], 'transform_m': m, 'transform_b': b})
    return out


def _stack(data):
    return (torch.stack([d['input'] for d in data]).cuda(), torch.stack([d['transform_m'] for d in data]).cuda(),
            torch.stack([d['transform_b'] for d in data]).cuda())


def _bar(data):
    return 2 * 1e-4 * max(float(d['transform_m'].abs().max()) for d in data)     # tests/test_inference_gpu.py's bar


def _model(base, **kw):
    from dsnt.model import build_mpii_pose_model
    m = build_mpii_pose_model(base=base, **kw)
    synthetic.fill_state_dict(m, seed=0)
    # realistic running statistics: one train-mode forward with momentum 1
    m.cuda().train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.momentum = 1.0
    x, _, _ = synthetic.batch(2, size=SIZE, seed=5, mask_p=1.0)
    with torch.no_grad():
        m(x.cuda())
    m.eval()
    return m


@pytest.fixture(scope='module')
def models():
    return {'hg1_dsnt': _model('hg1', output_strat='dsnt', reg='js'), 'hg1_gauss': _model('hg1'),
            'resnet18_dsnt': _model('resnet18', truncate=1, output_strat='dsnt')}


@pytest.fixture(scope='module')
def data5():
    return _dataset(5, SIZE, seed=11)


@pytest.fixture(scope='module')
def batch1(models, data5):
    """generate_predictions(..., batch_size=1) per model, computed once."""
    from dsnt import inference
    return {k: inference.generate_predictions(m, data5, use_flipped=True, batch_size=1) for k, m in models.items()}


# ------------------------------------------------------------------ 1. the kernel against the existing composition
SHAPES = [(64, 64), (32, 32), (14, 14), (7, 7), (66, 66)]     # 14, 7: widths not a multiple of 4; 66x66: uncached rows
HEADS = [('dsnt', 'softmax'), ('dsnt', 'thresholded_softmax'), ('dsnt', 'abs'), ('dsnt', 'relu'), ('dsnt', 'sigmoid'),
         ('gauss', 'softmax')]


@pytest.fixture(scope='module')
def head_model():
    from dsnt.model import build_mpii_pose_model
    return build_mpii_pose_model(base='hg1', output_strat='dsnt')      # only its forward_part2 / compute_coords run


@pytest.mark.parametrize('h,w', SHAPES)
@pytest.mark.parametrize('strategy,preact', HEADS)
def test_kernel_matches_aten_merge_and_model_head(head_model, strategy, preact, h, w):
    from dsnt import inference, util
    head_model.output_strat, head_model.preact = strategy, preact
    perm = inference.HFLIP_INDICES.cuda()
    g = torch.Generator().manual_seed(h * 1000 + w)
    for B in (1, 3, 5):
        L = (3 * torch.randn(2 * B, 16, h, w, generator=g)).cuda()
        tm = (torch.eye(2, dtype=torch.float64) * 150 + torch.rand(B, 2, 2, generator=g, dtype=torch.float64)).cuda()
        tb = (200 * torch.rand(B, 1, 2, generator=g, dtype=torch.float64)).cuda()
        img, coords, hm = inference.flip_merge_head(L, tm, tb, strategy, preact)
        hm1, hm2 = L.split(B)
        merged = (hm1 + hm2.flip(-1).index_select(-3, perm)) / 2
        if strategy == 'dsnt':
            out = head_model.forward_part2([merged])
            want_c = head_model.compute_coords(out)
            want_hm = head_model.heatmaps_array[0]
        else:
            want_c = util.decode_heatmaps(merged).cpu()
            want_hm = merged
        assert torch.equal(coords.cpu(), want_c), (B, (coords.cpu() - want_c).abs().max().item())
        assert torch.equal(hm, want_hm), B
        want_img = torch.baddbmm(tb, want_c.cuda().double(), tm)
        assert ((img - want_img).abs() <= 1e-12 * want_img.abs().clamp_min(1)).all(), B
        _, c2, none = inference.flip_merge_head(L, tm, tb, strategy, preact, heatmaps=False)
        assert none is None and torch.equal(c2, coords)


ORACLE_SHAPES = [(64, 64), (7, 7), (12, 20), (20, 12)]


@pytest.mark.parametrize('h,w', ORACLE_SHAPES)
def test_gauss_decode_matches_the_oracle(h, w):
    """The flip-merged gauss coordinates against the CPU oracle's decode of a merge made on the CPU (the test above takes
    the device's own decode as the expected value).  Both sides form (a + b) / 2 as an fp32 addition and an fp32 division
    by two; the division is exact, so the merged maps are equal bit for bit and so must the coordinates be."""
    from dsnt import inference
    from dsnt_oracle import util as ou
    g = torch.Generator().manual_seed(h * 1000 + w + 7)
    for B in (1, 3):
        L = 3 * torch.randn(2 * B, 16, h, w, generator=g)
        tm = torch.eye(2, dtype=torch.float64) * 150 + torch.rand(B, 2, 2, generator=g, dtype=torch.float64)
        tb = 200 * torch.rand(B, 1, 2, generator=g, dtype=torch.float64)
        hm1, hm2 = L.split(B)
        merged = (hm1 + hm2.flip(-1).index_select(-3, inference.HFLIP_INDICES)) / 2
        want = ou.decode_heatmaps(merged)
        for store in (True, False):
            _, coords, hm = inference.flip_merge_head(L.cuda(), tm.cuda(), tb.cuda(), 'gauss', 'softmax', heatmaps=store)
            assert torch.equal(coords.cpu(), want), (B, store, (coords.cpu() - want).abs().max().item())
            assert (hm is None) if not store else torch.equal(hm.cpu(), merged)


# ------------------------------------------------------------------ 2, 6. batch B against batch 1
@pytest.mark.parametrize('name', ['hg1_dsnt', 'hg1_gauss', 'resnet18_dsnt'])
def test_predict_batch_matches_batch_one(models, data5, batch1, name):
    from dsnt import inference
    m = models[name]
    x, tm, tb = _stack(data5)
    got = inference.predict(m, x, tm, tb).cpu()
    want = batch1[name]
    assert got.dtype == torch.float64 and got.shape == want.shape == (5, 16, 2)
    err = (got - want).abs().amax(-1)
    if m.output_strat == 'gauss':
        # arg-max of nearly equal pixels may move between backbone forms (tests/test_inference_gpu.py's rule)
        assert (err <= _bar(data5)).float().mean().item() >= 0.9
        scale = max(float(d['transform_m'].abs().max()) for d in data5)
        assert err.max().item() <= 2.6 * (2.0 / 32) * scale          # one pixel + quarter-pixel shifts of a 32x32 map
    else:
        assert err.max().item() <= _bar(data5), err.max().item()
    assert m.heatmaps.dim() == 4 and m.heatmaps.shape[:2] == (5, 16)      # the merged heat-maps of the batch


def test_predict_without_flip_matches_generate_predictions(models, data5):
    from dsnt import inference
    m = models['hg1_dsnt']
    x, tm, tb = _stack(data5)
    got = inference.predict(m, x, tm, tb, use_flipped=False).cpu()
    want = inference.generate_predictions(m, data5, use_flipped=False, batch_size=5)
    assert (got - want).abs().max().item() <= 1e-12 * 2 * _bar(data5) / 2e-4


def test_predict_dataset_matches_batch_one(models, data5, batch1):
    from dsnt import inference
    m = models['hg1_dsnt']

    class Meter:
        n, total = 0, 0.0

        def add(self, v):
            self.n += 1
            self.total += v
    meter = Meter()
    got = inference.predict_dataset(m, data5, use_flipped=True, batch_size=4, time_meter=meter)
    want = batch1['hg1_dsnt']
    assert got.dtype == want.dtype and got.shape == want.shape and got.device == want.device
    assert meter.n == 2 and meter.total > 0                      # batches of 4 + 1
    assert (got - want).abs().max().item() <= _bar(data5)


# ------------------------------------------------------------------ 3. one oracle-pinned case
def test_predict_matches_oracle_at_batch_one(models, data5):
    from dsnt import inference
    from dsnt_oracle import model as omodel, inference as oinference
    m = models['hg1_dsnt']
    o = omodel.build_mpii_pose_model(base='hg1', output_strat='dsnt', reg='js')
    o.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    data = data5[:1]
    x, tm, tb = _stack(data)
    got = inference.predict(m, x, tm, tb).cpu()
    want = oinference.generate_predictions(o, data, use_flipped=True, batch_size=1)
    assert (got - want).abs().max().item() <= _bar(data)


# ------------------------------------------------------------------ 4, 5. the paired input
def _augment_inputs(B, R=256, J=16, seed=0):
    r = np.random.default_rng(seed)
    src = torch.from_numpy(r.integers(0, 256, (B, R, R, 3), dtype=np.uint8)).cuda()
    side = r.uniform(150, 500, B)
    m = np.zeros((B, 3, 3))
    m[:, 0, 0] = m[:, 1, 1] = 2 / side
    m[:, 0, 2], m[:, 1, 2], m[:, 2, 2] = -2 * r.uniform(300, 900, B) / side, -2 * r.uniform(200, 600, B) / side, 1
    kp = (r.uniform(-0.9, 0.9, (B, J, 2)) - m[:, None, :2, 2]) / m[:, None, 0:1, 0]
    return (src, torch.from_numpy(kp).cuda(), torch.ones(B, J, device='cuda'), torch.from_numpy(m).cuda(),
            torch.from_numpy(r.uniform(40, 120, B)).cuda())


@pytest.fixture(scope='module')
def paired():
    from dsnt.data import DeviceAugment, ImageSpecs
    aug = DeviceAugment(ImageSpecs(SIZE, True, False), synthetic.IMAGE_MEAN, (1, 1, 1), use_aug=False, train=False)
    args = _augment_inputs(3, seed=2)
    return aug, args, aug(*args, step=0), aug(*args, step=0, flip_pair=True)


def test_paired_input_is_the_mirrored_twin(paired):
    _, _, plain, s = paired
    B = plain['input'].size(0)
    assert s['input_pair'].shape == (2 * B,) + tuple(plain['input'].shape[1:])
    assert torch.equal(s['input'], plain['input'])
    assert s['input'].data_ptr() == s['input_pair'].data_ptr()              # a view of the first half
    assert torch.equal(s['input_pair'][B:], s['input'].flip(-1))
    assert 'input_pair' not in plain
    for k in ('part_coords', 'part_mask', 'transform_m', 'transform_b'):
        assert torch.equal(s[k], plain[k])


def test_predict_paired_is_bit_identical(models, paired):
    from dsnt import inference
    _, _, _, s = paired
    for name in ('hg1_dsnt', 'hg1_gauss'):
        m = models[name]
        a = inference.predict(m, s['input_pair'], s['transform_m'], s['transform_b'], paired=True)
        b = inference.predict(m, s['input'], s['transform_m'], s['transform_b'], paired=False)
        assert torch.equal(a, b), name


def test_predict_and_pckh_without_host_sync(models, paired):
    from dsnt import inference
    from dsnt.evaluator import PCKhEvaluator
    aug, args, _, _ = paired
    m = models['hg1_dsnt']
    ev = PCKhEvaluator()

    def step(k):
        s = aug(*args, step=k, flip_pair=True)
        img, norm = inference.predict(m, s['input_pair'], s['transform_m'], s['transform_b'], paired=True,
                                      return_normalized=True)
        ev.add_normalized(norm, s['part_coords'], s['part_mask'], s['normalize'], s['transform_m'], s['transform_b'])
        return img, norm, s
    step(0)                                         # first call: per-device constants and launch lists are set up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')         # any synchronising call raises
    try:
        img, norm, s = step(1)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    want = torch.baddbmm(s['transform_b'], norm.double(), s['transform_m'])
    assert ((img - want).abs() <= 1e-12 * want.abs().clamp_min(1)).all()
    assert torch.isfinite(img).all().item()
