"""CPU checks of the device person crop (dsnt_crop_affine, dsnt.data.ImagePool / box_matrix): the export and its
argument validation, the golden file regenerates bit for bit, the numpy restatement (tests/crop_ref.py) is Pillow's
affine sampler on fresh random cases, and the Python surface refuses bad input before touching a device."""
import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import crop_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, 'tests', 'golden', 'make_crop_golden.py')


def _golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'crop.npz'))


def test_crop_exported_declared_and_versioned():
    from dsnt import _lib
    lib = _lib.load()
    assert hasattr(lib, 'dsnt_crop_affine') and 'dsnt_crop_affine' in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['dsnt_crop_affine']) == 12
    assert lib.dsnt_version() >= 119
    text = open(os.path.join(ROOT, 'include', 'dsnt_hip.h')).read()
    assert re.search(r'int dsnt_crop_affine\(const uint8_t\* pool, int64_t pool_bytes, const int64_t\* offset, '
                     r'const int32_t\* hw, int64_t N,\s+const int64_t\* idx, const double\* matrix, int B, int R, '
                     r'uint8_t\* out, uint8_t\* valid, void\* stream\);', text)


def test_crop_arguments_refused_before_launch():
    from dsnt import _lib
    lib = _lib.load()
    v = C.c_void_p(4096)
    ok = (v, 1 << 20, v, v, 4, v, v, 8, 96, v, v, None)

    def call(**kw):
        names = ('pool', 'pool_bytes', 'offset', 'hw', 'N', 'idx', 'matrix', 'B', 'R', 'out', 'valid', 'stream')
        args = dict(zip(names, ok))
        args.update(kw)
        return lib.dsnt_crop_affine(*(args[n] for n in names))
    for name in ('pool', 'offset', 'hw', 'idx', 'matrix', 'out', 'valid'):
        assert call(**{name: None}) == 3, name
        assert b'null pointer' in lib.dsnt_last_error()
    for kw in ({'B': 0}, {'B': 65536}, {'R': 0}, {'R': 8193}, {'N': 0}, {'pool_bytes': 0}):
        assert call(**kw) == 1, kw
        assert b'bad shape' in lib.dsnt_last_error()


def test_golden_regenerates_exactly():
    spec = importlib.util.spec_from_file_location('make_crop_golden', GEN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fresh = mod.make()
    g = _golden()
    assert sorted(fresh) == sorted(g.files)
    for k in g.files:
        a, b = np.asarray(fresh[k]), g[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(a, b), k


def test_golden_covers_the_issue_cases():
    g = _golden()
    names = [str(n) for n in g['names']]
    assert len(names) >= 12
    assert {int(g[n + '.R']) for n in names} == {384, 96, 37}
    assert sum(int(g[n + '.R']) == 384 for n in names) <= 2
    imgs = [int(g[n + '.image']) for n in names]
    assert len(set(imgs)) >= 3 and max(imgs.count(i) for i in set(imgs)) >= 2
    crops = {n: g[n + '.crop'] for n in names}
    assert any(not c.any() for c in crops.values())                                       # wholly off the image
    assert any(c.any() and (c.reshape(-1, 3).max(1) == 0).mean() > 0.2 for c in crops.values())   # partly off
    rotated = [n for n in names if abs(g[n + '.matrix'][0, 1]) > 1e-6]
    assert len(rotated) >= 3
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'crop.npz')) < 512 * 1024


def test_golden_coefficients_follow_the_rule():
    g = _golden()
    for n in g['names']:
        p = str(n) + '.'
        R = int(g[p + 'R'])
        coef = crop_ref.coefficients(g[p + 'matrix'], R)
        assert np.array_equal(np.array(coef), g[p + 'coef']), n
        inv = np.linalg.inv(g[p + 'matrix'])
        want = [2 * inv[0, 0] / R, 2 * inv[0, 1] / R, inv[0, 2] - inv[0, 0] - inv[0, 1],
                2 * inv[1, 0] / R, 2 * inv[1, 1] / R, inv[1, 2] - inv[1, 0] - inv[1, 1]]
        assert np.allclose(coef, want, rtol=1e-12, atol=1e-9), n
        img = g['img.%d' % int(g[p + 'image'])]
        crop, valid = crop_ref.crop(img, g[p + 'matrix'], R)
        assert valid and np.array_equal(crop, g[p + 'crop']), n


def test_restatement_is_pillows_affine_transform():
    """crop_ref.sample equals Image.transform(AFFINE, BILINEAR) on random images, rotations, scales and boxes."""
    from PIL import Image
    r = np.random.default_rng(119)
    for t in range(24):
        H, W = (int(v) for v in r.integers(3, 240, 2))
        img = r.integers(0, 256, (H, W, 3), dtype=np.uint8)
        ang, sx, sy = r.uniform(-1, 1), r.uniform(0.5, 5), r.uniform(0.5, 5)
        side = r.uniform(4, 300)
        cx, cy = r.uniform(-0.3 * W, 1.3 * W), r.uniform(-0.3 * H, 1.3 * H)
        c, s = math.cos(ang), math.sin(ang)
        m = np.array([[sx * c * 2 / side, sx * s * 2 / side, 0], [-sy * s * 2 / side, sy * c * 2 / side, 0], [0, 0, 1]])
        m[:2, 2] = -(m[:2, :2] @ [cx, cy])
        R = int(r.choice([1, 2, 5, 37, 64]))
        coef = crop_ref.coefficients(m, R)
        want = np.asarray(Image.fromarray(img).transform((R, R), Image.Transform.AFFINE, coef,
                                                         Image.Resampling.BILINEAR))
        assert np.array_equal(crop_ref.sample(img, coef, R), want), t


def test_singular_and_nonfinite_matrices_have_no_crop():
    img = np.full((8, 8, 3), 200, np.uint8)
    for m in (np.zeros((3, 3)), np.array([[1.0, 2, 0], [2, 4, 0], [0, 0, 1]]), np.full((3, 3), np.nan),
              np.array([[np.inf, 0, 0], [0, 1, 0], [0, 0, 1]])):
        crop, valid = crop_ref.crop(img, m, 5)
        assert not valid and not crop.any()


def test_box_matrix_arithmetic():
    from dsnt.data import box_matrix
    center = torch.tensor([[320.0, 240.5], [-10.25, 3.0]], dtype=torch.float64)
    side = torch.tensor([200.0, 33.3], dtype=torch.float64)
    m = box_matrix(center, side)
    assert m.dtype == torch.float64 and m.shape == (2, 3, 3) and m.device == center.device
    for b in range(2):
        cx, cy, s = float(center[b, 0]), float(center[b, 1]), float(side[b])
        want = np.array([[2 / s, 0, -2 * cx / s], [0, 2 / s, -2 * cy / s], [0, 0, 1]])
        assert np.array_equal(m[b].numpy(), want)
        for x, y in ((cx, cy), (cx - s / 2, cy + s / 2)):                  # centre -> 0, corner -> (-1, 1)
            n = m[b].numpy() @ [x, y, 1]
            assert np.allclose(n[:2], [(x - cx) * 2 / s, (y - cy) * 2 / s], atol=1e-12)
    from_numpy = box_matrix(np.array([[5.0, 6.0]]), np.array([10.0]))
    assert np.array_equal(from_numpy[0].numpy(), [[0.2, 0, -1.0], [0, 0.2, -1.2], [0, 0, 1]])
    with pytest.raises(RuntimeError, match=r'center \[B, 2\] and side \[B\]'):
        box_matrix(torch.zeros(3, 3), torch.ones(3))
    with pytest.raises(RuntimeError, match=r'center \[B, 2\] and side \[B\]'):
        box_matrix(torch.zeros(3, 2), torch.ones(2))


def test_image_pool_refuses_wrong_images():
    from dsnt.data import ImagePool
    good = np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(RuntimeError, match=r"convert\('RGB'\)"):
        ImagePool.from_images([good, np.zeros((4, 5, 3), np.float32)])
    with pytest.raises(RuntimeError, match=r"image 0 must be H x W x 3 uint8.*convert\('RGB'\)"):
        ImagePool.from_images([np.zeros((4, 5), np.uint8)])                # greyscale
    with pytest.raises(RuntimeError, match=r'got shape \(4, 5, 4\)'):
        ImagePool.from_images([np.zeros((4, 5, 4), np.uint8)])             # RGBA
    with pytest.raises(RuntimeError, match='image 1 must be H x W x 3 uint8'):
        ImagePool.from_images([good, torch.zeros(3, 4, 5, dtype=torch.uint8)])   # CHW tensor
    with pytest.raises(RuntimeError, match='numpy array or tensor'):
        ImagePool.from_images([good, [[1, 2, 3]]])
    with pytest.raises(RuntimeError, match=r'sides must lie in \[1, 16384\]'):
        ImagePool.from_images([np.zeros((0, 5, 3), np.uint8)])
    with pytest.raises(RuntimeError, match='at least one image'):
        ImagePool.from_images([])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ImagePool.from_images([good], device='cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):           # a pool of host tensors
        ImagePool(torch.zeros(60, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64),
                  torch.tensor([[4, 5]], dtype=torch.int32))
    with pytest.raises(RuntimeError, match='ImagePool.hw must be a torch.int32 tensor'):
        ImagePool(torch.zeros(60, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), torch.tensor([[4, 5]]))
