"""Golden vectors of the device person crop (dsnt_crop_affine, dsnt.data.ImagePool.crop).

    python tests/golden/make_crop_golden.py        # writes tests/golden/crop.npz

A crop is defined by a bounding-box matrix M (original-image pixels -> [-1, 1]^2 box coordinates, the `matrix` of
DeviceAugment) and Pillow's affine sampler:

    Image.fromarray(img).transform((R, R), Image.AFFINE, (a, b, c, d, e, f), Image.BILINEAR)

with inv = inverse(M) by the adjugate (tests/crop_ref.py restates the kernel's order of operations) and, in fp64,
a = 2*inv[0]/R, b = 2*inv[1]/R, c = inv[2] - inv[0] - inv[1], d = 2*inv[3]/R, e = 2*inv[4]/R, f = inv[5] - inv[3] - inv[4].
The crops below are Pillow's (12.2 here); nothing else is imported.

Sources are blocky PCG64 images (8 x 8 blocks of uniform uint8 noise plus a 6-column stripe of a 1-pixel 0/255
checker) of odd sizes, so the file stays small while block edges and the stripe exercise the taps and the truncation.
Cases: pure downscale (x3), upscale (x0.5), rotated and sheared matrices, a mirrored one, a box partly off the image and
one wholly off it, two samples from one image, and R in {384, 96, 37}.
"""
import math
import os
import sys
import zlib

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]

import crop_ref  # noqa: E402

SIZES = [(97, 131), (360, 480), (33, 1000), (250, 187)]       # (H, W)


def _rng(name):
    return np.random.Generator(np.random.PCG64([23, zlib.crc32(name.encode())]))


def source(k):
    H, W = SIZES[k]
    r = _rng('img.%d' % k)
    base = r.integers(0, 256, ((H + 7) // 8, (W + 7) // 8, 3), dtype=np.uint8)
    img = np.repeat(np.repeat(base, 8, 0), 8, 1)[:H, :W]
    x0 = W // 3
    img[:, x0:x0 + 6] = np.where((np.arange(H)[:, None, None] + np.arange(6)[None, :, None]) % 2, 255, 0)
    return np.ascontiguousarray(img)


def box(cx, cy, side, rot=0.0, sx=1.0, sy=1.0, shear=0.0):
    """M = S . Rot(rot) . T(-cx, -cy): image px -> box coordinates, `side` px across (scaled by sx, sy; sheared)."""
    c, s = math.cos(math.radians(rot)), math.sin(math.radians(rot))
    a = np.array([[sx * 2 / side, shear * 2 / side, 0], [0, sy * 2 / side, 0], [0, 0, 1]]) @ \
        np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]])
    a[:2, 2] = -(a[:2, :2] @ np.array([cx, cy]))
    return a


# name, image, R, M
CASES = [
    ('down3_96', 1, 96, box(240.0, 180.0, 288.0)),                     # 3 image px per crop px
    ('up2_96', 0, 96, box(65.5, 48.5, 48.0)),                          # 0.5 image px per crop px
    ('r384', 1, 384, box(231.3, 171.9, 301.7)),
    ('rot30_96', 1, 96, box(250.0, 170.0, 220.0, rot=30.0)),
    ('rot_m70_aniso_37', 3, 37, box(93.0, 125.0, 160.0, rot=-70.0, sx=1.3, sy=0.8)),
    ('shear_37', 0, 37, box(60.0, 40.0, 70.0, rot=11.0, shear=0.35)),
    ('mirror_96', 3, 96, box(90.0, 120.0, 140.0, sx=-1.0)),
    ('partial_left_96', 2, 96, box(20.0, 16.0, 90.0, rot=5.0)),        # much of the box is off the image
    ('off_37', 2, 37, box(1400.0, -300.0, 100.0)),                     # wholly off: black, but valid
    ('pair_a_96', 3, 96, box(60.0, 80.0, 100.0)),                      # two people in one image
    ('pair_b_96', 3, 96, box(140.0, 170.0, 120.0, rot=-15.0)),
    ('strip_37', 2, 37, box(500.0, 16.5, 40.0, rot=3.0)),             # taller than the 33-row image
]


def make():
    out = {'names': np.array([c[0] for c in CASES])}
    for k in range(len(SIZES)):
        out['img.%d' % k] = source(k)
    for name, k, R, m in CASES:
        coef = crop_ref.coefficients(m, R)
        crop = np.asarray(Image.fromarray(out['img.%d' % k]).transform((R, R), Image.Transform.AFFINE, coef,
                                                                       Image.Resampling.BILINEAR))
        p = name + '.'
        out.update({p + 'image': np.int64(k), p + 'R': np.int64(R), p + 'matrix': m,
                    p + 'coef': np.array(coef, np.float64), p + 'crop': crop.copy()})
    return out


if __name__ == '__main__':
    path = os.path.join(HERE, 'crop.npz')
    np.savez_compressed(path, **make())
    print(path, os.path.getsize(path))
