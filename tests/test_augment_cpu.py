"""CPU checks of the training augmentation (dsnt.data.DeviceAugment, csrc/augment.hip): the golden file regenerates
bit for bit, its keypoint maths agrees with the reference's torch formulation, the restatement the GPU tests compare
with (tests/augment_ref.py) reproduces Pillow's flip, rotation and centre crop exactly and draws what the kernel's
header states, and the new entry points are exported and validate their arguments."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import augment_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, 'tests', 'golden', 'make_augment_golden.py')


def _gen():
    spec = importlib.util.spec_from_file_location('make_augment_golden', GEN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'augment.npz'))


def test_golden_regenerates_exactly():
    fresh = _gen().make()
    g = _golden()
    assert sorted(fresh) == sorted(g.files)
    for k in g.files:
        a, b = np.asarray(fresh[k]), g[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(a, b), k


def _reference_keypoints(kp, matrix, kmask, scale, rot, hflip, train=True):
    """data.py:125-196 restated with the reference's torch operations (mm with the transpose, scatter_, torch.inverse)."""
    from dsnt.inference import HFLIP_INDICES
    pc = torch.from_numpy(np.concatenate([kp, np.ones((len(kp), 1))], 1) @ matrix.transpose())[:, :2].contiguous()
    pm = torch.from_numpy(kmask.astype(np.float64))
    t = torch.eye(3).double()
    if hflip:
        t = torch.mm(t.new([[-1, 0, 0], [0, 1, 0], [0, 0, 1]]), t)
    r = math.radians(rot)
    t = torch.mm(t.new([[math.cos(r) / scale, math.sin(r) / scale, 0], [-math.sin(r) / scale, math.cos(r) / scale, 0],
                        [0, 0, 1]]), t)
    coords = torch.DoubleTensor(pc.size(0), 3)
    coords[:, 0:2].copy_(pc)
    coords[:, 2].fill_(1)
    pc.copy_(torch.mm(coords, t.transpose(0, 1))[:, 0:2])
    if hflip:
        idx2 = HFLIP_INDICES.view(-1, 1).expand_as(pc)
        pc.scatter_(0, idx2, pc.clone())
        pm.scatter_(0, HFLIP_INDICES, pm.clone())
    if train:
        within, _ = pc.abs().lt(1).min(-1, keepdim=False)
        pm.mul_(within.double())
    s = torch.mm(torch.from_numpy(np.linalg.inv(matrix)), torch.inverse(t))
    return pc.numpy(), pm.numpy(), s[0:2, 0:2].numpy(), s[0:2, 2].contiguous().view(1, 2).numpy()


def test_golden_keypoints_match_the_reference_formulation():
    g = _golden()
    for n in g['names']:
        p = str(n) + '.'
        pc, pm, tm, tb = _reference_keypoints(g[p + 'keypoints'], g[p + 'matrix'], g[p + 'keypoint_mask'],
                                              float(g[p + 'scale']), float(g[p + 'rot']), int(g[p + 'hflip']))
        for got, want in ((pc, g[p + 'part_coords_f64']), (tm, g[p + 'trans_m']), (tb, g[p + 'trans_b'])):
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), n
        assert np.array_equal(pm.astype(np.float32), g[p + 'part_mask']), n
        assert np.array_equal(pc.astype(np.float32), g[p + 'part_coords']), n


def test_golden_covers_the_issue_cases():
    g = _golden()
    names = [str(n) for n in g['names']]
    assert len(names) >= 12
    sides = {int(g[n + '.S']) for n in names}
    assert sides == {128, 256}
    cs = [int(384 * float(g[n + '.scale'])) for n in names]
    assert any(c % 2 and c < 384 for c in cs) and any(c % 2 and c > 384 for c in cs)     # half-to-even offsets
    rots = {float(g[n + '.rot']) for n in names}
    assert {7.5, -7.5, 30.0, -30.0, 60.0} <= rots
    assert any(int(g[n + '.hflip']) and float(g[n + '.rot']) != 0 and float(g[n + '.scale']) != 1 for n in names)
    assert any(float(g[n + '.gain'].max()) * 255 > 255 * 1.5 for n in names)


@pytest.mark.parametrize('R', [40, 41, 384])
def test_kernel_sampling_rule_is_pillows_rotation(R):
    from PIL import Image
    r = np.random.default_rng(R)
    img = r.integers(0, 256, (R, R, 3), dtype=np.uint8)
    for rot in (7.5, -7.5, 30.0, -30.0, 60.0, -59.9, 0.3, 359.0):
        want = np.asarray(Image.fromarray(img).rotate(rot, Image.Resampling.BILINEAR))
        assert np.array_equal(augment_ref.rotate(img, rot), want), (R, rot)

GRID_R = (5, 8, 9, 33, 40, 41, 97)
GRID_ROT = (90.0, 180.0, 270.0, -90.0, 360.0, 720.5, 1e-6, -1e-6, 60.0, -60.0, 45.0, 0.3, 359.0,
            float(np.float32(-59.9)), float(np.float32(12.345)), -0.0)
GRID_SCALE = (2 ** -0.5, 0.75, 1.0, 1.3, 2 ** 0.5)


@pytest.mark.parametrize('R', GRID_R)
def test_restated_crop_is_pillows_flip_rotate_crop(R):
    """augment_ref.crop against Image.transpose / rotate(BILINEAR) / crop on noise (every pixel differs from its
    neighbours), bit for bit: right angles (Pillow's transpose shortcut), whole turns, -0.0, tiny angles, odd and even
    R, c < R and c > R.  R = 5 adds c == 1."""
    pil_crop = _gen().pil_crop
    r = np.random.default_rng(1000 + R)
    src = r.integers(0, 256, (R, R, 3), dtype=np.uint8)
    scales = GRID_SCALE + ((0.3,) if R == 5 else ())
    for hflip in (0, 1):
        for rot in GRID_ROT:
            for scale in scales:
                scale = float(np.float32(scale))              # the kernel's parameters are fp32
                got, want = augment_ref.crop(src, scale, rot, hflip), pil_crop(src, scale, rot, hflip)
                assert got.shape == want.shape and np.array_equal(got, want), (R, rot, scale, hflip)
    if R == 5:
        assert augment_ref.crop(src, float(np.float32(0.3)), 7.5, 1).shape == (1, 1, 3)


def test_restated_crop_clamps_like_the_kernel():
    src = np.random.default_rng(5).integers(0, 256, (5, 5, 3), dtype=np.uint8)
    for scale in (0.0, -1.0, 0.19, float('nan')):
        assert np.array_equal(augment_ref.crop(src, scale, 0.0, 0), src[2:3, 2:3]), scale      # c = 1, offset 2
    for scale in (100.0, 8.01, float('inf')):
        big = augment_ref.crop(src, scale, 0.0, 0)
        assert big.shape == (40, 40, 3) and np.array_equal(big[18:23, 18:23], src)              # offset round(-17.5) = -18
        assert int(big.sum()) == int(src.sum())
    assert augment_ref.crop(src, 8.0, 0.0, 0).shape == (40, 40, 3) and augment_ref.crop(src, 0.2, 0.0, 0).shape == (1, 1, 3)


def test_restated_keypoints_match_the_reference_formulation():
    from dsnt.inference import HFLIP_INDICES
    g = _golden()
    for n in g['names']:
        p = str(n) + '.'
        for train in (True, False):
            args = (g[p + 'keypoints'], g[p + 'matrix'], g[p + 'keypoint_mask'], float(g[p + 'scale']),
                    float(g[p + 'rot']), int(g[p + 'hflip']))
            want = _reference_keypoints(*args, train=train)
            got = augment_ref.keypoints(*args, HFLIP_INDICES.numpy(), train)
            for a, w in zip(got, want):
                assert a.shape == w.shape, (n, train)
            for a, w in ((got[0], want[0]), (got[2], want[2]), (got[3], want[3])):
                assert np.abs(a - w).max() <= 1e-12 * max(1.0, np.abs(w).max()), (n, train)
            assert np.array_equal(got[1], want[1]), (n, train)


def _draws_differ(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


def test_restated_draw_is_a_function_of_every_counter_and_key_word():
    sample = np.arange(64)
    seed, step = 0x0123456789ABCDEF, 0x00000003_00000007
    base = augment_ref.draw(seed, step, sample)
    again = augment_ref.draw(seed, step, sample)
    assert [x.dtype for x in base] == [np.float32, np.float32, np.uint8, np.float32]
    assert [x.shape for x in base] == [(64,), (64,), (64,), (64, 3)]
    assert all(np.array_equal(x, y) for x, y in zip(base, again))
    one = augment_ref.draw(seed, step, 5)                              # a scalar sample word: that row of the batch
    assert all(np.array_equal(np.asarray(x), y[5]) for x, y in zip(one, base))
    assert _draws_differ(base, augment_ref.draw(seed, step, sample + 64))
    assert _draws_differ(base, augment_ref.draw(seed, step ^ 1, sample))                  # step, low word
    assert _draws_differ(base, augment_ref.draw(seed, step ^ (1 << 32), sample))          # step, high word
    assert _draws_differ(base, augment_ref.draw(seed ^ 1, step, sample))                  # seed, low word
    assert _draws_differ(base, augment_ref.draw(seed ^ (1 << 63), step, sample))          # seed, high word
    # the sample word is 32 bits wide, as the kernel's is
    assert all(np.array_equal(x, y) for x, y in zip(base, augment_ref.draw(seed, step, sample + 2 ** 32)))
    # the three gains are three words of one Philox output, not one word reused
    assert not np.array_equal(base[3][:, 0], base[3][:, 1]) and not np.array_equal(base[3][:, 1], base[3][:, 2])


def test_restated_draw_respects_the_clip_bounds_exactly():
    scale, rot, hflip, gain = augment_ref.draw(99, 3, np.arange(1 << 16))
    lo, hi = np.float32(2 ** -0.5), np.float32(2 ** 0.5)
    assert scale.min() == lo and scale.max() == hi                     # 4.6 % of the samples sit on each pair of bounds
    assert 0.03 < (scale == lo).mean() + (scale == hi).mean() < 0.06
    assert rot.min() == -60 and rot.max() == 60
    assert 0.3 < (rot != 0).mean() < 0.5 and 0.4 < hflip.mean() < 0.6 and set(np.unique(hflip)) == {0, 1}
    assert gain.astype(np.float64).min() > 0.6 and gain.max() <= np.float32(1.4)
    # the ends of the word range: unit() is (0, 1], so the rotation threshold .4 and the flip threshold .5 are inclusive
    w = lambda *v: [np.array([x], np.uint64) for x in v]
    u = lambda t: int(t * 16777216 - 1) << 8                            # the smallest word with unit(word) == t
    assert augment_ref.unit(0) == 2.0 ** -24 and augment_ref.unit(0xFFFFFFFF) == 1.0
    assert augment_ref.unit(u(0.5)) == 0.5 and augment_ref.unit(u(0.5) + 256) > 0.5
    s, r, h, gn = augment_ref.draw_from_words(w(0, 0, 0, u(0.5)), w(0, 0xFFFFFFFF, 0, 0), w(0, 0xFFFFFFFF, 0x80000000, 0))
    assert s[0] == hi and r[0] == 60 and h[0] == 1                      # sqrt(-2 ln 2^-24) cos(2 pi 2^-24) = 5.77: clipped
    assert gn[0, 0] == np.float32(0.6 + 0.8 * 2.0 ** -24) and gn[0, 1] == np.float32(1.4) and float(gn[0, 0]) > 0.6
    s, r, h, gn = augment_ref.draw_from_words(w(0xFFFFFFFF, 0, 0xFFFFFFFF, u(0.5) + 256), w(0, 0, 0, 0), w(0, 0, 0, 0))
    assert s[0] == 1 and r[0] == 0 and h[0] == 0                        # ln 1 = 0: scale 2^0; unit 1 > .4: no rotation
    t4 = (int(0.4 * 16777216) - 1) << 8                                 # the largest word with unit(word) <= .4
    assert augment_ref.unit(t4) <= 0.4 < augment_ref.unit(t4 + 256)
    assert augment_ref.draw_from_words(w(0, 0, t4, 0), w(0, 0, 0, 0), w(0, 0, 0, 0))[1][0] == 60
    assert augment_ref.draw_from_words(w(0, 0, t4 + 256, 0), w(0, 0, 0, 0), w(0, 0, 0, 0))[1][0] == 0


def test_augment_symbols_exported_and_validated_without_gpu():
    from dsnt import _lib
    lib = _lib.load()
    for n in ('dsnt_augment_fwd', 'dsnt_augment_keypoints', 'dsnt_pool_normalize'):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.dsnt_version() >= 115
    v = C.c_void_p(4096)
    assert lib.dsnt_augment_fwd(None, 2, 384, 256, v, v, v, v, 1, 0, 0, v, v, v, None) == 3
    assert lib.dsnt_augment_fwd(v, 2, 384, 0, v, v, v, v, 1, 0, 0, v, v, v, None) == 1
    assert lib.dsnt_augment_fwd(v, 70000, 384, 256, v, v, v, v, 1, 0, 0, v, v, v, None) == 1
    assert lib.dsnt_augment_keypoints(v, v, v, 2, 16, v, v, v, None, 1, v, v, v, v, None) == 3
    assert lib.dsnt_augment_keypoints(v, v, v, 0, 16, v, v, v, v, 1, v, v, v, v, None) == 1
    assert lib.dsnt_pool_normalize(v, 1, 3, 8, 8, 0, v, v, v, None) == 1
    assert lib.dsnt_pool_normalize(None, 1, 3, 8, 8, 4, v, v, v, None) == 3


def test_device_augment_refuses_cpu_and_bad_inputs():
    from dsnt.data import DeviceAugment, ImageSpecs
    specs = ImageSpecs(64, True, True)
    aug = DeviceAugment(specs, (0.4, 0.4, 0.4), (0.25, 0.25, 0.25))
    src = torch.zeros(2, 96, 96, 3, dtype=torch.uint8)
    kp = torch.zeros(2, 16, 2, dtype=torch.float64)
    km = torch.ones(2, 16)
    m = torch.eye(3, dtype=torch.float64).expand(2, 3, 3).contiguous()
    hl = torch.ones(2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        aug(src, kp, km, m, hl, 0)
    with pytest.raises(RuntimeError, match='uint8'):
        aug(src.float(), kp, km, m, hl, 0)
    with pytest.raises(RuntimeError, match=r'\[B, R, R, 3\]'):
        aug(src[:, :, :80], kp, km, m, hl, 0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        specs.convert(torch.zeros(3, 96, 96), type('Stats', (), {'MEAN': [0] * 3, 'STDDEV': [1] * 3}))
