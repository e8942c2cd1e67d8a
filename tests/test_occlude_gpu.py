"""`dsnt.data.Occlude` (`dsnt_occlude`, csrc/occlude.hip) on the MI355X against the numpy restatement
(tests/occlude_ref.py), bit for bit: `input` as int32 bit patterns, `rects`, `donor`, `occluded` and `part_mask` exactly.
Shapes are the smallest at which the kernel can go wrong: S = 5 (the scalar path), S = 8 with rectangle edges off the
multiples of 4 (vector groups part inside, part outside), S = 8 on a tensor that is not 16-byte aligned (the scalar path
again), S = 64 with B = 3 (a sample spans several workgroups), B = 1 and 2 for the paste fill, K = 1 and 8, J = 0, 16, 17."""
import numpy as np
import pytest
import torch

import occlude_ref as ref

pytestmark = pytest.mark.gpu

MEAN, STD, VALUE = (0.44, 0.44, 0.40), (0.25, 0.26, 0.27), (0.5, -1.25, 3.0)
SPECIAL = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001],
                   np.uint32).view(np.int32)      # NaNs with payloads, a signalling NaN, +-inf, -0, a subnormal


def _host(B, S, J, seed, special=False):
    r = np.random.default_rng(seed)
    x = r.standard_normal((B, 3, S, S)).astype(np.float32)
    if special:
        bits = x.view(np.int32)
        at = r.random(x.shape) < 0.3
        bits[at] = SPECIAL[r.integers(0, len(SPECIAL), int(at.sum()))]
    return x, r.uniform(-1.2, 1.2, (B, J, 2)).astype(np.float32), (r.random((B, J)) < 0.7).astype(np.float32)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _dev(a, unaligned=False):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not unaligned:
        return t.cuda()
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')       # the same values 4 bytes off a 16-byte boundary
    out = base[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def _sample(x, coords, mask, unaligned=False):
    B = x.shape[0]
    return {'input': _dev(x, unaligned), 'part_coords': _dev(coords), 'part_mask': _dev(mask),
            'normalize': torch.ones(B, dtype=torch.float64, device='cuda'), 'params': {'scale': torch.ones(B, device='cuda')}}


def _occ(**kw):
    from dsnt.data import Occlude
    return Occlude(**dict(dict(p=0.75, fill_value=VALUE, mean=MEAN, std=STD, seed=23), **kw))


def _run(occ, x, coords, mask, step, draw_offset=0, rects=None, donor=None, unaligned=False):
    """One call held against the restatement; also: the sample passed in is left as it was.  Returns (out, used rects)."""
    B, S = x.shape[0], x.shape[2]
    sample = _sample(x, coords, mask, unaligned)
    before = {k: v.clone() for k, v in sample.items() if isinstance(v, torch.Tensor)}
    kept = dict(sample)
    given = {}
    if rects is not None:
        given['rects'] = torch.from_numpy(np.asarray(rects, np.int32)).cuda()
        if donor is not None:
            given['donor'] = torch.from_numpy(np.asarray(donor, np.int32)).cuda()
    out = occ(sample, step, draw_offset=draw_offset, **given)
    lo, hi = occ.sides(S)
    ref_donor = donor if donor is not None or rects is None else (np.arange(1, B + 1) % B)
    bits, rr, dd, oc = ref.occlude(x, coords, mask, step, K=occ.max_rects, side_min=lo, side_max=hi, p24=ref.p24_of(occ.p),
                                   fill=occ.fill, centre=occ.centre, seed=occ.seed, draw_offset=draw_offset,
                                   fill_value=occ.fill_value, mean=occ.mean, std=occ.std, rects=rects, donor=ref_donor)
    got = _bits(out['input'])
    assert got.shape == bits.shape and out['input'].dtype == torch.float32
    assert np.array_equal(got, bits), np.argwhere(got != bits)[:5]
    pr, pd = out['params']['occ_rects'], out['params']['occ_donor']
    assert pr.dtype == torch.int32 and tuple(pr.shape) == (B, occ.max_rects, 4) and pd.dtype == torch.int32
    if rects is None:
        assert np.array_equal(pr.cpu().numpy(), rr) and np.array_equal(pd.cpu().numpy(), dd)
    else:                                                   # given values are inputs: handed back as they came
        assert np.array_equal(pr.cpu().numpy(), np.asarray(rects, np.int32)) and np.array_equal(pd.cpu().numpy(), ref_donor)
    assert out['occluded'].dtype == torch.uint8 and tuple(out['occluded'].shape) == oc.shape
    assert np.array_equal(out['occluded'].cpu().numpy(), oc)
    if occ.mask_covered:
        assert np.array_equal(out['part_mask'].cpu().numpy(), mask * (1 - oc.astype(np.float32)))
    else:
        assert out['part_mask'] is sample['part_mask']
    # the sample passed in: same keys, same tensor objects, same contents
    assert sample.keys() == kept.keys() and all(sample[k] is kept[k] for k in kept)
    assert 'occluded' not in sample and 'occ_rects' not in sample['params'] and out['params']['scale'] is sample['params']['scale']
    for k, v in before.items():
        assert np.array_equal(_bits(sample[k]) if v.dtype == torch.float32 else sample[k].cpu().numpy(),
                              _bits(v) if v.dtype == torch.float32 else v.cpu().numpy()), k
    assert out['input'].data_ptr() != sample['input'].data_ptr() and out['normalize'] is sample['normalize']
    return out, rr


#         B, S, K, J, side, unaligned
SHAPES = [(3, 64, 8, 16, (0.1, 0.4), False),        # several workgroups per sample
          (2, 5, 1, 17, (0.2, 0.6), False),         # S % 4 != 0: the scalar path
          (2, 8, 2, 17, (0.2, 0.6), False),         # sides 2..5: edges off the multiples of 4
          (1, 8, 8, 0, (0.2, 0.6), False),          # a batch of one, no joints
          (2, 8, 2, 16, (0.2, 0.6), True)]          # S % 4 == 0 but not 16-byte aligned: the scalar path


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'B%d-S%d-K%d-J%d%s' % (s[:4] + ('-unaligned' if s[5] else '',)))
@pytest.mark.parametrize('centre', ['uniform', 'joint'])
@pytest.mark.parametrize('fill', ['value', 'noise', 'paste'])
def test_drawn_occlusion_matches_the_restatement(fill, centre, shape):
    B, S, K, J, side, unaligned = shape
    x, coords, mask = _host(B, S, J, seed=B * 100 + S)
    occ = _occ(fill=fill, centre=centre, max_rects=K, side=side, mask_covered=(K == 2))
    hit = 0
    for step in (0, 3):
        _, rr = _run(occ, x, coords, mask, step, unaligned=unaligned)
        hit += int(rr.any())
    assert hit, 'the case needs at least one occluded sample'


@pytest.mark.parametrize('fill', ['noise', 'paste'])
def test_draw_offset_and_a_step_above_two_to_the_32(fill):
    x, coords, mask = _host(3, 8, 16, seed=7)
    occ = _occ(fill=fill, centre='joint', max_rects=3, side=(0.2, 0.6), p=1.0)
    step = 2 ** 32 + 5
    a, ra = _run(occ, x, coords, mask, step, draw_offset=2 ** 32 - 2)       # the sample word wraps at 2^32
    b, rb = _run(occ, x, coords, mask, step)
    c, rc = _run(occ, x, coords, mask, 5)
    assert not np.array_equal(ra, rb) and not np.array_equal(rb, rc)      # the offset and the step's high word count
    wide = ref.draw(6, 8, 3, *occ.sides(8), 1 << 24, occ.seed, step, 0, 'uniform')[0]
    narrow = ref.draw(3, 8, 3, *occ.sides(8), 1 << 24, occ.seed, step, 3, 'uniform')[0]
    assert np.array_equal(wide[3:], narrow)


def test_same_key_same_bits_another_step_another_draw():
    x, coords, mask = _host(3, 64, 16, seed=9)
    occ = _occ(fill='noise', max_rects=4, p=1.0)
    sample = _sample(x, coords, mask)
    a, b, c = occ(sample, 11), occ(sample, 11), occ(sample, 12)
    assert a['input'].data_ptr() != b['input'].data_ptr()
    assert np.array_equal(_bits(a['input']), _bits(b['input']))
    assert torch.equal(a['params']['occ_rects'], b['params']['occ_rects']) and torch.equal(a['occluded'], b['occluded'])
    assert not torch.equal(a['params']['occ_rects'], c['params']['occ_rects'])
    assert not np.array_equal(_bits(a['input']), _bits(c['input']))
    other = _occ(fill='noise', max_rects=4, p=1.0, seed=24)(sample, 11)
    assert not torch.equal(a['params']['occ_rects'], other['params']['occ_rects'])


def test_probability_zero_copies_every_bit():
    for S, unaligned in ((8, False), (8, True), (5, False), (64, False)):
        x, coords, mask = _host(2, S, 16, seed=S, special=True)
        out, rr = _run(_occ(p=0.0, fill='noise'), x, coords, mask, 1, unaligned=unaligned)
        assert not rr.any() and not out['occluded'].any()
        assert np.array_equal(_bits(out['input']), x.view(np.int32))


def _given(S):
    """rects int32 [4, 4, 4] and donors for a batch of four: the whole image; one pixel and two empty ones; overlapping ones
    with coordinates below 0 and above S; ones that clamp to nothing and a full column."""
    rects = np.array([[[0, 0, S, S], [0, 0, 0, 0], [2, 2, 2, 2], [0, 0, 0, 0]],
                      [[3, 2, 4, 3], [4, 4, 4, S + 1], [4, 1, 2, 4], [0, 0, 0, 0]],
                      [[1, 1, S - 2, S - 2], [3, 3, S, S - 1], [-5, -3, 2, 2], [S - 2, S - 2, S + 10, S + 7]],
                      [[-10, -10, -1, -1], [S + 1, 0, S + 5, S], [2, -100, 3, 100], [0, 0, 0, 0]]], np.int32)
    return rects, np.array([-3, 9, 0, 2], np.int32)


@pytest.mark.parametrize('S,unaligned', [(5, False), (8, False), (8, True), (64, False)])
@pytest.mark.parametrize('fill', ['value', 'noise', 'paste'])
def test_given_rectangles_special_values_and_clamping(fill, S, unaligned):
    x, coords, mask = _host(4, S, 17, seed=S + 1, special=True)
    rects, donor = _given(S)
    occ = _occ(fill=fill, max_rects=4, centre='joint')
    out, rr = _run(occ, x, coords, mask, 2, rects=rects, donor=donor, unaligned=unaligned)
    assert rr.min() == 0 and rr.max() == S                       # the restatement clamped as the kernel does
    got, inside = _bits(out['input']), ref.cover(rr, S)
    assert inside[0].all() and inside[1].sum() == 1 and inside[3].sum() == S
    for b in range(4):                                          # outside the rectangles NaN, +-inf and -0 come through untouched
        assert np.array_equal(got[b][:, ~inside[b]], x.view(np.int32)[b][:, ~inside[b]])
    if fill == 'paste':                                         # donors -3 and 9 clamp to 0 and 3: sample 0 pastes itself
        assert np.array_equal(got[0], x.view(np.int32)[0])
        assert np.array_equal(got[1][:, inside[1]], x.view(np.int32)[3][:, inside[1]])
    _run(occ, x, coords, mask, 2, rects=rects, unaligned=unaligned)          # no donor given: the next sample


def test_joints_on_a_rectangle_edge_at_nan_and_outside_the_image():
    S, B = 8, 2
    on = lambda px: np.float32(-1 + 2 * (px + 0.5) / S)          # the centre of pixel px
    c = np.array([[on(2), on(2)], [on(5), on(5)], [on(6), on(5)], [on(1), on(2)], [-0.5, -0.5], [0.5, 0.0], [on(5), 0.5],
                  [np.nan, 0.0], [0.0, np.nan], [1.0, 0.0], [-1.0, -1.0], [1.5, 0.0], [0.0, -1.5], [np.inf, 0.0],
                  [np.float32(1) - np.float32(2 ** -24), 0.0], [on(3), on(3)], [on(0), on(0)]], np.float32)
    coords = np.stack([c, c])
    mask = np.stack([np.ones(17, np.float32), np.array([0, 0.5, 1] * 5 + [0, 1], np.float32)])
    rects = np.array([[[2, 2, 6, 6], [0, 0, 0, 0]], [[2, 2, 6, 6], [0, 0, 1, 1]]], np.int32)
    want0 = [1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0]
    want1 = want0[:10] + [1] + want0[11:16] + [1]                 # sample 1 also hides pixel (0, 0)
    x = _host(B, S, 17, seed=4)[0]
    for covered in (False, True):
        out, _ = _run(_occ(max_rects=2, mask_covered=covered), x, coords, mask, 0, rects=rects)
        assert out['occluded'].cpu().tolist() == [want0, want1]
        if covered:
            assert out['part_mask'].cpu().tolist() == [[m * (1 - o) for m, o in zip(mask[b].tolist(), w)]
                                                       for b, w in enumerate((want0, want1))]
    # drawn on joints: only joints with a pixel and a non-zero mask centre a rectangle
    out, rr = _run(_occ(max_rects=8, centre='joint', p=1.0, side=(0.1, 0.2)), x, coords, mask, 3)
    px, py = ref.joint_pixels(coords, S)
    for b in range(B):
        ok = {(px[b, j], py[b, j]) for j in range(17) if px[b, j] >= 0 and mask[b, j] != 0}
        for x0, y0, x1, y1 in rr[b]:
            assert x1 == x0 or any(x0 <= u < x1 and y0 <= v < y1 for u, v in ok)


# ---- loaders

N, R, LS, J = 12, 24, 16, 16
KEYS = ('input', 'part_coords', 'part_mask', 'transform_m', 'transform_b', 'normalize', 'hflip', 'index')


@pytest.fixture(scope='module')
def pool():
    from dsnt.data import DeviceDataset
    r = np.random.default_rng(0)
    side = r.uniform(150, 500, N)
    m = np.zeros((N, 3, 3))
    m[:, 0, 0] = m[:, 1, 1] = 2 / side
    m[:, 0, 2], m[:, 1, 2], m[:, 2, 2] = -2 * r.uniform(300, 900, N) / side, -2 * r.uniform(200, 600, N) / side, 1
    kp = (r.uniform(-1.2, 1.2, (N, J, 2)) - m[:, None, :2, 2]) / m[:, None, 0:1, 0]
    return DeviceDataset.from_arrays(r.integers(0, 256, (N, R, R, 3), dtype=np.uint8), kp,
                                     (r.random((N, J)) < 0.8).astype(np.float32), m, r.uniform(40, 120, N))


def _augment():
    from dsnt.data import DeviceAugment, ImageSpecs
    return DeviceAugment(ImageSpecs(LS, True, True), MEAN, STD, seed=17)


def _same(a, b, keys=KEYS):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(_bits(a[k]) if a[k].dtype == torch.float32 else a[k].cpu().numpy(),
                              _bits(b[k]) if b[k].dtype == torch.float32 else b[k].cpu().numpy()), k
    assert a['params'].keys() == b['params'].keys()
    for k in a['params']:
        assert torch.equal(a['params'][k], b['params'][k]), k


def _loader_occ(aug, **kw):
    from dsnt.data import Occlude
    return Occlude.like(aug, **dict(dict(p=0.8, max_rects=3, side=(0.2, 0.5), fill='paste', centre='joint', mask_covered=True), **kw))


def test_loader_without_occlude_is_the_loader_of_today(pool):
    from dsnt.data import EpochLoader
    aug = _augment()
    a, b = list(EpochLoader(pool, 5, aug, seed=5, occlude=None)), list(EpochLoader(pool, 5, aug, seed=5))
    assert len(a) == len(b) == 3
    for x, y in zip(a, b):
        assert x.keys() == y.keys() and 'occluded' not in x and 'occ_rects' not in x['params']
        _same(x, y)


@pytest.mark.parametrize('weighted', [False, True], ids=['epoch', 'weighted'])
@pytest.mark.parametrize('fill', ['paste', 'noise'])
def test_loader_batches_are_occlude_of_the_plain_batches(pool, weighted, fill):
    from dsnt.data import EpochLoader, WeightedLoader
    aug = _augment()
    occ = _loader_occ(aug, fill=fill)
    assert occ.seed == 17 and occ.mean == aug.mean and occ.std == aug.std

    def make(occlude, **kw):
        if weighted:
            w = torch.tensor(np.exp2(np.random.default_rng(1).uniform(-3, 3, N)), dtype=torch.float32, device='cuda')
            return WeightedLoader(pool, 5, aug, w, seed=5, occlude=occlude, **kw)
        return EpochLoader(pool, 5, aug, seed=5, occlude=occlude, **kw)

    ld, plain = make(occ), make(None)
    for epoch in (0, 1):
        got, base = list(ld), list(plain)
        assert len(got) == len(base) == 3 and got[2]['input'].shape[0] == 2          # a partial last batch
        hit = 0
        for s, (g, p) in enumerate(zip(got, base)):
            want = occ(p, epoch * 3 + s, draw_offset=0)
            _same(g, want, KEYS + ('occluded',))
            assert torch.equal(g['part_mask'], p['part_mask'] * (1 - g['occluded'].float()))        # mask_covered
            hit += int(g['params']['occ_rects'].any())
        assert hit, 'the case needs an occluded batch'
    # resumed mid-epoch: the next batch is the uninterrupted one
    state = {'epoch': 1, 'batch': 1, 'seed': 5}
    if weighted:
        state = dict(ld.state_dict(), **state)
    again, plain2 = make(occ), make(None)
    again.load_state_dict(state)
    plain2.load_state_dict(state)
    g, p = next(iter(again)), next(iter(plain2))
    _same(g, occ(p, 1 * 3 + 1), KEYS + ('occluded',))
    _same(g, got[1], KEYS + ('occluded',))
    # rank 1 of 2 draws with offset rank * B
    r1, p1 = make(occ, drop_last=True, rank=1, world_size=2), make(None, drop_last=True, rank=1, world_size=2)
    assert len(r1) == 1
    g, p = next(iter(r1)), next(iter(p1))
    _same(g, occ(p, 0, draw_offset=5), KEYS + ('occluded',))
    assert not torch.equal(g['params']['occ_rects'], occ(p, 0, draw_offset=0)['params']['occ_rects'])


def test_refusals():
    from dsnt.data import DeviceAugment, ImageSpecs
    x, coords, mask = _host(2, 8, 16, seed=1)
    occ = _occ(max_rects=2)
    sample = _sample(x, coords, mask)
    with pytest.raises(RuntimeError, match='input_pair'):
        occ(dict(sample, input_pair=torch.zeros(4, 3, 8, 8, device='cuda')), 0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        occ(dict(sample, input=sample['input'].cpu()), 0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        occ(dict(sample, part_coords=sample['part_coords'].cpu()), 0)
    with pytest.raises(RuntimeError, match='contiguous'):
        occ(dict(sample, input=sample['input'].transpose(2, 3)), 0)
    with pytest.raises(RuntimeError, match='input must be torch.float32'):
        occ(dict(sample, input=sample['input'].double()), 0)
    with pytest.raises(RuntimeError, match='part_mask must have shape'):
        occ(dict(sample, part_mask=sample['part_mask'][:, :15].contiguous()), 0)
    with pytest.raises(RuntimeError, match='part_coords must be torch.float32'):
        occ(dict(sample, part_coords=sample['part_coords'].double()), 0)
    rects = torch.zeros(2, 2, 4, dtype=torch.int32, device='cuda')
    with pytest.raises(RuntimeError, match='rects must be torch.int32'):
        occ(sample, 0, rects=rects.long())
    with pytest.raises(RuntimeError, match='rects must have shape'):
        occ(sample, 0, rects=torch.zeros(2, 3, 4, dtype=torch.int32, device='cuda'))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        occ(sample, 0, rects=rects.cpu())
    with pytest.raises(RuntimeError, match='donor must have shape'):
        occ(sample, 0, rects=rects, donor=torch.zeros(3, dtype=torch.int32, device='cuda'))
    with pytest.raises(RuntimeError, match='donor must be torch.int32'):
        occ(sample, 0, rects=rects, donor=torch.zeros(2, dtype=torch.int64, device='cuda'))
    with pytest.raises(RuntimeError, match='donor needs given rects'):
        occ(sample, 0, donor=torch.zeros(2, dtype=torch.int32, device='cuda'))
    # a flip_pair batch of DeviceAugment is refused, and so is a flip_pair loader with an Occlude
    aug = DeviceAugment(ImageSpecs(8, True, True), MEAN, STD, use_aug=False, seed=1)
    pair = aug(torch.zeros(2, 12, 12, 3, dtype=torch.uint8, device='cuda'), torch.zeros(2, 16, 2, dtype=torch.float64, device='cuda'),
               torch.ones(2, 16, device='cuda'), torch.eye(3, dtype=torch.float64, device='cuda').expand(2, 3, 3).contiguous(),
               torch.ones(2, dtype=torch.float64, device='cuda'), 0, flip_pair=True)
    with pytest.raises(RuntimeError, match='input_pair'):
        occ(pair, 0)
    plain = aug(torch.zeros(2, 12, 12, 3, dtype=torch.uint8, device='cuda'), torch.zeros(2, 16, 2, dtype=torch.float64, device='cuda'),
                torch.ones(2, 16, device='cuda'), torch.eye(3, dtype=torch.float64, device='cuda').expand(2, 3, 3).contiguous(),
                torch.ones(2, dtype=torch.float64, device='cuda'), 0)
    out = occ(plain, 0)                                        # and a DeviceAugment sample goes straight in
    assert out['input'].shape == plain['input'].shape and out['hflip'] is plain['hflip']
    # the entry point itself refuses in == out on the device too
    from dsnt import _lib
    t = sample['input']
    with pytest.raises(RuntimeError, match='in and out overlap'):
        _lib.call('dsnt_occlude', _lib.ptr(t), _lib.ptr(t), 2, 8, 2, 1, 4, 0, 0, 0, _lib.ptr(occ._consts(t.device)[0]),
                  _lib.ptr(occ._consts(t.device)[1]), _lib.ptr(occ._consts(t.device)[2]), None, None, 0,
                  _lib.ptr(rects), _lib.ptr(torch.zeros(2, dtype=torch.int32, device='cuda')), None, 1, 0, 0, 0)
