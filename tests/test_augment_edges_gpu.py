"""The augmentation kernels of csrc/augment.hip off the 384-pixel goldens, against tests/augment_ref.py (which
tests/test_augment_cpu.py pins to Pillow bit for bit): small, odd and upsampling image shapes on noise sources, right
angles, whole turns, -0.0 and a tiny angle, a crop of one pixel and the kernel's clamp of an out-of-range scale; the
flip pair and the gather variants at an odd shape, with indices outside the pool; the parameter draw sample by sample
against the restated Philox stream; the keypoints kernel across workgroups, at J != 16 and on the `|coord| < 1` edge;
ImageSpecs.convert when it upsamples and when the element count is no multiple of the workgroup.

Measured on MI355X at the first run: every image batch matched the restatement bit for bit, rotated samples included
(max |diff| = 0 at (R, S) = (5, 4), (9, 16), (41, 64), (40, 17), (33, 33), (97, 32), on the 24 one-pixel and clamp samples
at (5, 4) and on the (41, 64) pool); the pair, gather and out-of-pool comparisons are exact by construction and held; of
the 8192 drawn scale and rot values of each of the nine (seed, step) pairs and the three gather offsets, 0 were not
bit-identical to the restatement (max 0 ulp), and hflip, the unrotated set and the gains were equal; keypoints, masks,
matrices and convert passed the bars below.  No kernel change was needed.

The bars are the project's existing ones (tests/test_augment_gpu.py), kept as the contract and not tightened to what
was measured: unrotated images 1e-6; rotated ones >= 99.9 % of elements within 1/255 before normalisation and none
beyond 2/255 (device and host fp64 cos / sin may differ in the last bit before the truncation to uint8); f32 keypoints
1e-6 and f64 matrices 1e-12, relative to max(1, |value|); drawn hflip, the set of unrotated samples and the gains
exact (integer arithmetic and exactly rounded fp64 operations), drawn scale and non-zero rot within 1 fp32 ulp (they go
through log, cos and exp2: two correct fp64 values a few ulps apart can straddle an fp32 rounding boundary)."""
import itertools

import numpy as np
import pytest
import torch

import augment_ref

pytestmark = pytest.mark.gpu

MEAN = (0.44, 0.44, 0.40)
STD = (0.26, 0.25, 0.27)
f32 = lambda v: float(np.float32(v))
SCALES = (f32(2 ** -0.5), 0.75, 1.0, f32(1.3), f32(2 ** 0.5))
ROTS = (0.0, -0.0, 7.5, -60.0, 90.0, 180.0, 359.0, 360.0, f32(1e-6))
# (R, S): smallest useful; c < S, even upsampling; c < S, odd R; S*S = 289 = 256 + 33 (a mostly dead second workgroup);
# c == S at scale 1; odd R with ragged windows
SHAPES = ((5, 4), (9, 16), (41, 64), (40, 17), (33, 33), (97, 32))
ONES = (1.0, 1.0, 1.0)
CLAMP_GAIN = (f32(0.6), f32(1.4), 5.0)            # gain 5: most of the blue channel clamps at 1
PARAM_KEYS = ('scale', 'rot', 'hflip', 'gain')
SAMPLE_KEYS = ('input', 'part_coords', 'part_mask', 'transform_m', 'transform_b', 'normalize', 'hflip')


def _cross():
    """The issue's parameter cross, (scale, rot, hflip, gain) per sample; the rotated scale-1 sample carries the gains."""
    cases = [(s, r, h, ONES) for s, r, h in itertools.product(SCALES, ROTS, (0, 1))]
    i = cases.index((1.0, 7.5, 0, ONES))
    cases[i] = (1.0, 7.5, 0, CLAMP_GAIN)
    return cases


def _augment(S, train=True, seed=0, normalise=True):
    from dsnt.data import DeviceAugment, ImageSpecs
    return DeviceAugment(ImageSpecs(S, normalise, normalise), MEAN, STD, use_aug=True, train=train, seed=seed)


def _params(cases):
    col = lambda i, dt: torch.tensor([c[i] for c in cases], dtype=dt).cuda()
    return {'scale': col(0, torch.float32), 'rot': col(1, torch.float32), 'hflip': col(2, torch.uint8),
            'gain': col(3, torch.float32)}


def _still(B, J=16):
    """Keypoint inputs that play no part: zero keypoints, identity box matrices."""
    return (torch.zeros(B, J, 2, dtype=torch.float64, device='cuda'), torch.ones(B, J, device='cuda'),
            torch.eye(3, dtype=torch.float64, device='cuda').expand(B, 3, 3).contiguous(),
            torch.ones(B, dtype=torch.float64, device='cuda'))


def _device_images(src, cases, S):
    out = _augment(S)(torch.from_numpy(src).cuda(), *_still(len(cases)), step=0, params=_params(cases))
    torch.cuda.synchronize()
    return out['input'].cpu().numpy()


def _expected_images(src, cases, S):
    return np.stack([augment_ref.to_input(augment_ref.crop(src[i], s, r, h), g, S, MEAN, STD)
                     for i, (s, r, h, g) in enumerate(cases)])


def _hold_images(got, want, cases, label):
    """The bars of tests/test_augment_gpu.py on every sample; prints the batch's maximum and whether it was bit-exact."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    std = np.asarray(STD, np.float64).reshape(3, 1, 1)
    d = np.abs(got.astype(np.float64) - want)
    print('%s: %d samples, max |diff| %.3g, bit-exact %s' % (label, len(cases), np.nanmax(d), np.array_equal(got, want)))
    assert not np.isnan(got).any(), label
    for i, c in enumerate(cases):
        if c[1] % 360.0 == 0:
            assert d[i].max() <= 1e-6, (label, c, d[i].max())
        else:
            pre = d[i] * std                                   # the difference before normalisation
            frac = float((pre <= 1 / 255 + 1e-6).mean())
            assert frac >= 0.999 and pre.max() <= 2 / 255 + 1e-6, (label, c, frac, pre.max())


@pytest.mark.parametrize('R,S', SHAPES)
def test_images_match_restatement_on_noise(R, S):
    cases = _cross()
    assert len(cases) == 90
    src = np.random.default_rng([R, S]).integers(0, 256, (len(cases), R, R, 3), dtype=np.uint8)
    _hold_images(_device_images(src, cases, S), _expected_images(src, cases, S), cases, 'R=%d S=%d' % (R, S))


def test_one_pixel_crop_and_the_clamp_of_out_of_range_scales():
    """R = 5: scale .3 gives c == 1; R * scale below 1 or NaN is clamped to c = 1 and above 8R to c = 8R = 40, whose
    offset round(-17.5) = -18 leaves the image in a wide zero border."""
    R, S = 5, 4
    cases = [(s, r, h, ONES) for s, r, h in
             itertools.product((f32(0.3), 0.0, 100.0, float('nan')), (0.0, 7.5, 90.0), (0, 1))]
    assert [augment_ref.crop_side(R, s) for s in (f32(0.3), 0.0, 100.0, float('nan'))] == [1, 1, 40, 1]
    src = np.random.default_rng(54).integers(0, 256, (len(cases), R, R, 3), dtype=np.uint8)
    _hold_images(_device_images(src, cases, S), _expected_images(src, cases, S), cases, 'R=5 S=4 clamp')


def _pool(N, R, J=16, seed=0):
    """A synthetic pool on the device: (crops, keypoints, keypoint_mask, matrix, head_lengths)."""
    r = np.random.default_rng(seed)
    side = r.uniform(150, 500, N)
    m = np.zeros((N, 3, 3))
    m[:, 0, 0] = m[:, 1, 1] = 2 / side
    m[:, 0, 2], m[:, 1, 2], m[:, 2, 2] = -2 * r.uniform(300, 900, N) / side, -2 * r.uniform(200, 600, N) / side, 1
    kp = (r.uniform(-1.3, 1.3, (N, J, 2)) - m[:, None, :2, 2]) / m[:, None, 0:1, 0]
    host = (r.integers(0, 256, (N, R, R, 3), dtype=np.uint8), kp, (r.random((N, J)) < 0.8).astype(np.float32), m,
            r.uniform(40, 120, N))
    return tuple(torch.from_numpy(a).cuda() for a in host)


def _rows(pool, idx):
    return tuple(t[idx].contiguous() for t in pool)


def _fwd_gather(aug, crops, idx, p, pair=False, draw=0, step=0, draw_offset=0):
    """dsnt_augment_fwd_gather / _pair_gather through the C ABI; `p` = [scale, rot, hflip, gain] (read, or written when
    draw).  Returns the [B or 2B, 3, S, S] output."""
    from dsnt import _lib
    B, S = idx.numel(), aug.image_specs.size
    mean, std, _ = aug._consts(crops.device)
    out = torch.empty(2 * B if pair else B, 3, S, S, device='cuda')
    _lib.call('dsnt_augment_fwd_pair_gather' if pair else 'dsnt_augment_fwd_gather', _lib.ptr(crops), crops.shape[0],
              _lib.ptr(idx), B, crops.shape[1], S, *map(_lib.ptr, p), draw, aug.seed & (2 ** 64 - 1), step, draw_offset,
              _lib.ptr(mean), _lib.ptr(std), _lib.ptr(out))
    return out


def _gather(aug, pool, idx, params, pair):
    """The sample dict of the gather entry points with given parameters, as EpochLoader assembles it."""
    from dsnt import _lib
    crops, kp, km, m, hl = pool
    B, J = idx.numel(), kp.shape[1]
    p = [params[k].clone() for k in PARAM_KEYS]
    both = _fwd_gather(aug, crops, idx, p, pair)
    out = {'input': both[:B], 'part_coords': torch.empty(B, J, 2, device='cuda'),
           'part_mask': torch.empty(B, J, device='cuda'),
           'transform_m': torch.empty(B, 2, 2, dtype=torch.float64, device='cuda'),
           'transform_b': torch.empty(B, 1, 2, dtype=torch.float64, device='cuda'),
           'normalize': torch.empty(B, dtype=torch.float64, device='cuda')}
    _lib.call('dsnt_augment_keypoints_gather', _lib.ptr(m), _lib.ptr(kp), _lib.ptr(km), _lib.ptr(hl), crops.shape[0],
              _lib.ptr(idx), B, J, *map(_lib.ptr, p[:3]), _lib.ptr(aug._consts(crops.device)[2]), 1 if aug.train else 0,
              *(_lib.ptr(out[k]) for k in ('part_coords', 'part_mask', 'transform_m', 'transform_b', 'normalize')))
    out['hflip'] = p[2].bool()
    if pair:
        out['input_pair'] = both
    torch.cuda.synchronize()
    return out


ODD = (41, 64)
MIXED = [(f32(2 ** -0.5), 7.5, 1, ONES), (1.0, 0.0, 0, ONES), (f32(1.3), -60.0, 0, CLAMP_GAIN), (0.75, 90.0, 1, ONES),
         (f32(2 ** 0.5), 0.0, 1, ONES), (1.0, 359.0, 0, ONES)]


def test_pair_is_the_plain_launch_and_its_mirror():
    R, S = ODD
    pool = _pool(len(MIXED), R, seed=1)
    aug, params = _augment(S), _params(MIXED)
    plain = aug(*pool, step=0, params=params)
    pair = aug(*pool, step=0, params=params, flip_pair=True)
    B = len(MIXED)
    assert pair['input_pair'].shape == (2 * B, 3, S, S)
    assert torch.equal(pair['input_pair'][:B], plain['input']) and torch.equal(pair['input'], plain['input'])
    assert torch.equal(pair['input_pair'][B:], pair['input_pair'][:B].flip(-1))
    for k in SAMPLE_KEYS[1:]:
        assert torch.equal(pair[k], plain[k]), k
    # and the plain launch is the restatement's image here too
    src = pool[0].cpu().numpy()
    _hold_images(plain['input'].cpu().numpy(), _expected_images(src, MIXED, S), MIXED, 'R=41 S=64 pool')


@pytest.mark.parametrize('pair', [False, True])
def test_gather_equals_the_plain_launch_on_the_gathered_rows(pair):
    R, S = ODD
    pool = _pool(7, R, seed=2)
    idx = torch.tensor([4, 0, 6, 2, 2, 5], device='cuda')                 # a repeat allowed
    aug, params = _augment(S), _params(MIXED)
    got = _gather(aug, pool, idx, params, pair)
    want = aug(*_rows(pool, idx), step=0, params=params, flip_pair=pair)
    for k in SAMPLE_KEYS + (('input_pair',) if pair else ()):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize('pair', [False, True])
def test_an_index_outside_the_pool_reads_nothing_and_marks_the_sample(pair):
    """-1 and N: a NaN image (both halves of a pair), part_mask 0, NaN coordinates, matrices and normalize; the samples
    beside them equal the plain launch."""
    R, S = ODD
    N = 7
    pool = _pool(N, R, seed=3)
    idx = torch.tensor([3, -1, 1, N, 5], device='cuda')
    good, bad = [0, 2, 4], [1, 3]
    cases = MIXED[:5]
    B = len(cases)
    aug = _augment(S)
    got = _gather(aug, pool, idx, _params(cases), pair)
    want = aug(*_rows(pool, idx[good]), step=0, params=_params([cases[i] for i in good]), flip_pair=pair)
    for k in SAMPLE_KEYS:
        assert torch.equal(got[k][good], want[k]), k
    halves = (got['input'], got['input_pair'][B:]) if pair else (got['input'],)
    for h in halves:
        assert torch.isnan(h[bad]).all().item() and not torch.isnan(h[good]).any().item()
    if pair:
        assert torch.equal(got['input_pair'][B:][good], want['input_pair'][len(good):])
    assert (got['part_mask'][bad] == 0).all().item()
    for k in ('part_coords', 'transform_m', 'transform_b', 'normalize'):
        assert torch.isnan(got[k][bad]).all().item(), k


DRAW_B = 4096


def _ulps(a, b):
    """Distance in fp32 steps between two float32 arrays (finite values, either sign)."""
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(2 ** 31) - i, i)
    return np.abs(ordered(a) - ordered(b))


def _hold_draw(got, want, label):
    """got / want = (scale, rot, hflip, gain) of every sample of a batch.  Returns the count of values not bit-identical."""
    gs, gr, gh, gg = got
    ws, wr, wh, wg = want
    assert gs.dtype == gr.dtype == gg.dtype == np.float32 and gs.shape == ws.shape and gg.shape == wg.shape, label
    assert np.array_equal(gh, wh), (label, 'hflip', int((gh != wh).sum()))
    assert np.array_equal(gr == 0, wr == 0), (label, 'rotated set', int(((gr == 0) != (wr == 0)).sum()))
    assert np.array_equal(gg, wg), (label, 'gain', int((gg != wg).sum()))
    us, ur = _ulps(gs, ws), _ulps(gr, wr)
    differ = int((us != 0).sum() + (ur != 0).sum())
    print('%s: %d of %d scale and rot values not bit-identical (max %d ulp)'
          % (label, differ, 2 * gs.size, max(us.max(), ur.max())))
    assert us.max() <= 1, (label, 'scale', int(us.max()), int(us.argmax()))
    assert ur.max() <= 1, (label, 'rot', int(ur.max()), int(ur.argmax()))
    return differ


def _host(p):
    return tuple(p[k].cpu().numpy() for k in PARAM_KEYS)


@pytest.mark.parametrize('step', [0, 3, 2 ** 32 + 7])
@pytest.mark.parametrize('seed', [0, 99, 2 ** 63 + 5])
def test_draw_equals_the_restated_stream_sample_by_sample(seed, step):
    B = DRAW_B
    aug = _augment(4, seed=seed, normalise=False)
    src = torch.zeros(B, 8, 8, 3, dtype=torch.uint8, device='cuda')
    out = aug(src, *_still(B), step=step)
    torch.cuda.synchronize()
    _hold_draw(_host(out['params']), augment_ref.draw(seed, step, np.arange(B)), 'seed %d step %d' % (seed, step))


@pytest.mark.parametrize('draw_offset', [0, 1000, 2 ** 32 - DRAW_B])
def test_gather_draws_with_sample_word_b_plus_offset(draw_offset):
    B, seed, step = DRAW_B, 2 ** 63 + 5, 2 ** 32 + 7
    aug = _augment(4, seed=seed, normalise=False)
    crops = torch.zeros(3, 8, 8, 3, dtype=torch.uint8, device='cuda')
    idx = (torch.arange(B, device='cuda') % 3).contiguous()
    p = [torch.empty(B, device='cuda'), torch.empty(B, device='cuda'),
         torch.empty(B, dtype=torch.uint8, device='cuda'), torch.empty(B, 3, device='cuda')]
    _fwd_gather(aug, crops, idx, p, draw=1, step=step, draw_offset=draw_offset)
    torch.cuda.synchronize()
    got = tuple(t.cpu().numpy() for t in p)
    _hold_draw(got, augment_ref.draw(seed, step, np.arange(B) + draw_offset), 'gather offset %d' % draw_offset)


def _device_keypoints(m, kp, km, scale, rot, hflip, flip_idx, train):
    """dsnt_augment_keypoints through the C ABI (DeviceAugment takes given parameters only with the 16 MPII joints)."""
    from dsnt import _lib
    B, J = kp.shape[:2]
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    ins = (dev(m, torch.float64), dev(kp, torch.float64), dev(km, torch.float32))
    par = (dev(scale, torch.float32), dev(rot, torch.float32), dev(hflip, torch.uint8), dev(flip_idx, torch.int64))
    # sentinels: every element must be written
    outs = (torch.full((B, J, 2), -7.0, device='cuda'), torch.full((B, J), -7.0, device='cuda'),
            torch.full((B, 2, 2), -7.0, dtype=torch.float64, device='cuda'),
            torch.full((B, 1, 2), -7.0, dtype=torch.float64, device='cuda'))
    _lib.call('dsnt_augment_keypoints', *map(_lib.ptr, ins), B, J, *map(_lib.ptr, par), train, *map(_lib.ptr, outs))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in outs)


def _close(got, want, tol):
    return bool((np.abs(got - want) <= tol * np.maximum(1.0, np.abs(want))).all())


@pytest.mark.parametrize('train', [0, 1])
@pytest.mark.parametrize('B,J,flips', [(3, 1, False), (5, 17, False), (2, 300, False), (40, 16, True)])
def test_keypoints_match_restatement_across_workgroups(B, J, flips, train):
    """(2, 300) and (40, 16) exceed one 256-thread workgroup (600 = 2 * 256 + 88 elements, 640 = 2 * 256 + 128); flips only
    with the 16 MPII joints, whose table is the only one there is."""
    r = np.random.default_rng([B, J])
    side = r.uniform(150, 500, B)
    m = np.zeros((B, 3, 3))
    m[:, 0, 0] = m[:, 1, 1] = 2 / side
    m[:, 0, 2], m[:, 1, 2], m[:, 2, 2] = -2 * r.uniform(300, 900, B) / side, -2 * r.uniform(200, 600, B) / side, 1
    kp = (r.uniform(-1.3, 1.3, (B, J, 2)) - m[:, None, :2, 2]) / m[:, None, 0:1, 0]
    km = (r.random((B, J)) < 0.8).astype(np.float32)
    scale = r.uniform(2 ** -0.5, 2 ** 0.5, B).astype(np.float32)
    rot = r.uniform(-60, 60, B).astype(np.float32)
    hflip = (np.arange(B) % 2 if flips else np.zeros(B)).astype(np.uint8)
    if flips:
        from dsnt.inference import HFLIP_INDICES
        flip_idx = HFLIP_INDICES.numpy()
        assert J == len(flip_idx)
    else:
        flip_idx = np.arange(J)
    pc, pm, tm, tb = _device_keypoints(m, kp, km, scale, rot, hflip, flip_idx, train)
    masked = 0
    for b in range(B):
        wc, wm, wtm, wtb = augment_ref.keypoints(kp[b], m[b], km[b], float(scale[b]), float(rot[b]), int(hflip[b]),
                                                 flip_idx, bool(train))
        assert _close(pc[b], wc, 1e-6), (b, np.abs(pc[b] - wc).max())
        assert np.array_equal(pm[b], wm.astype(np.float32)), b
        assert _close(tm[b], wtm, 1e-12) and _close(tb[b], wtb, 1e-12), b
        masked += int(km[b].sum() - wm.sum())
    if B * J >= 85:
        assert (masked > 0) == bool(train)                    # train mode masks the joints that left the box


def test_keypoint_mask_edge_is_strict_and_decided_in_fp64():
    """scale 1, rot 0, identity box matrix: the coordinate is the keypoint exactly.  |coord| < 1 is strict, NaN fails it,
    the largest double below 1 (which rounds to 1.f) passes it; eval mode masks nothing."""
    below = np.nextafter(1.0, 0.0)
    nan = float('nan')
    kp = np.array([[[1.0, 0.3], [-1.0, 0.0], [0.5, 1.0], [0.5, -1.0], [nan, 0.0], [0.0, nan], [below, -below],
                    [0.5, 0.5]]])
    J = kp.shape[1]
    args = (np.eye(3)[None], kp, np.ones((1, J), np.float32), np.ones(1), np.zeros(1), np.zeros(1), np.arange(J))
    for train, want in ((1, [0, 0, 0, 0, 0, 0, 1, 1]), (0, [1] * J)):
        pc, pm, tm, tb = _device_keypoints(*args, train)
        assert pm[0].tolist() == want, (train, pm[0])
        ref = augment_ref.keypoints(kp[0], np.eye(3), np.ones(J), 1.0, 0.0, 0, None, bool(train))
        assert np.array_equal(pc[0], ref[0].astype(np.float32), equal_nan=True), train      # a NaN takes its whole joint
        finite = np.isfinite(kp[0]).all(-1)
        assert np.array_equal(pc[0][finite], kp[0][finite].astype(np.float32)) and np.isnan(pc[0][~finite]).all()
        assert np.array_equal(pm[0], ref[1].astype(np.float32)), train
        assert np.array_equal(tm[0], np.eye(2)) and np.array_equal(tb[0], np.zeros((1, 2))), train


class _Stats:
    MEAN, STDDEV = list(MEAN), list(STD)


@pytest.mark.parametrize('N,H,W,S', [(2, 5, 7, 16), (1, 23, 19, 17)])
def test_convert_upsampling_and_on_a_ragged_grid(N, H, W, S):
    """(5, 7) -> 16: windows of one or two source pixels that repeat.  N = 1, S = 17: 3 * 289 = 867 elements, a last
    workgroup with 99 live threads.  Bit-equal to adaptive_avg_pool2d + Normalize on the CPU."""
    from dsnt.data import ImageSpecs
    x = torch.from_numpy(np.random.default_rng([H, W, S]).random((N, 3, H, W), dtype=np.float32))
    want = torch.nn.functional.adaptive_avg_pool2d(x, S)
    for ch in range(3):
        want[:, ch].sub_(_Stats.MEAN[ch]).div_(_Stats.STDDEV[ch])
    specs = ImageSpecs(S, True, True)
    got = specs.convert(x.cuda(), _Stats).cpu()
    assert got.shape == (N, 3, S, S)
    assert torch.equal(got, want), (got - want).abs().max()
    assert torch.equal(specs.convert(x[0].cuda(), _Stats).cpu(), want[0])
