"""CPU checks of the training augmentation (dsnt.data.DeviceAugment, csrc/augment.hip): the golden file regenerates
bit for bit, its keypoint maths agrees with the reference's torch formulation, the sampling rule the kernel implements
reproduces Pillow's rotation exactly, and the new entry points are exported and validate their arguments."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

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


def _kernel_rotate(img, rot):
    """The sampling rule csrc/augment.hip implements (step 2 of its header), restated in numpy."""
    R = img.shape[0]
    deg = rot % 360.0
    ang = -math.radians(deg)
    a, b = round(math.cos(ang), 15), round(math.sin(ang), 15)
    c = a * -(R / 2) + b * -(R / 2) + 0.0 + R / 2
    f = -b * -(R / 2) + a * -(R / 2) + 0.0 + R / 2
    ys, xs = np.mgrid[0:R, 0:R].astype(np.float64)
    xin = a * (xs + 0.5) + b * (ys + 0.5) + c
    yin = -b * (xs + 0.5) + a * (ys + 0.5) + f
    inside = (xin >= 0) & (xin < R) & (yin >= 0) & (yin < R)
    xin, yin = xin - 0.5, yin - 0.5
    x0, y0 = np.floor(xin), np.floor(yin)
    dx, dy = (xin - x0)[..., None], (yin - y0)[..., None]
    x0, y0 = x0.astype(int), y0.astype(int)
    cl = lambda v: np.clip(v, 0, R - 1)
    im = img.astype(np.float64)
    v1 = im[cl(y0), cl(x0)] + (im[cl(y0), cl(x0 + 1)] - im[cl(y0), cl(x0)]) * dx
    has2 = ((y0 + 1 >= 0) & (y0 + 1 < R))[..., None]
    v2 = np.where(has2, im[cl(y0 + 1), cl(x0)] + (im[cl(y0 + 1), cl(x0 + 1)] - im[cl(y0 + 1), cl(x0)]) * dx, v1)
    v = (v1 + (v2 - v1) * dy).astype(np.int64)            # truncation
    return np.where(inside[..., None], v, 0).astype(np.uint8)


@pytest.mark.parametrize('R', [40, 41, 384])
def test_kernel_sampling_rule_is_pillows_rotation(R):
    from PIL import Image
    r = np.random.default_rng(R)
    img = r.integers(0, 256, (R, R, 3), dtype=np.uint8)
    for rot in (7.5, -7.5, 30.0, -30.0, 60.0, -59.9, 0.3, 359.0):
        want = np.asarray(Image.fromarray(img).rotate(rot, Image.Resampling.BILINEAR))
        assert np.array_equal(_kernel_rotate(img, rot), want), (R, rot)


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
