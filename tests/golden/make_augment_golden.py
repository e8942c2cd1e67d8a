"""Golden vectors of the MPII training-sample transform (reference `src/dsnt/data.py:118-226`).

    python tests/golden/make_augment_golden.py        # writes tests/golden/augment.npz

The transform is restated here from its documented semantics and computed with Pillow and torch's CPU
ops; nothing is imported from the reference (its `torchdata` and torchvision 0.2.0 are absent).  Per sample:

  1. `Image.transpose(FLIP_LEFT_RIGHT)` when hflip;
  2. `Image.rotate(rot, BILINEAR)` when rot != 0 (about (w/2, h/2), expand=False, black outside);
  3. torchvision 0.2.0 `CenterCrop(R * scale)`: side c = int(R * scale), offset round((R - c) / 2) with Python's
     half-to-even round, `Image.crop` zero-filling outside the image;
  4. `ToTensor` (x / 255 in fp32), channel gain, clamp(0, 1);
  5. `adaptive_avg_pool2d` to S x S, then `Normalize(mean, std)` ((x - m) / s per channel, fp32).

The keypoints follow `data.py:150-196` in fp64: `transform_keypoints(kp, matrix)` (homogeneous [x, y, 1] @ matrix^T),
then `@ t^T` with t = R(rot)/scale . F(hflip); left/right joints swapped under hflip; train mode masks joints
with |coord| >= 1; the back-projection is inv(matrix) . inv(t).

Pillow version: generated with Pillow 12.2; the reference pins Pillow 4.2.1.  Both rotate about
(w / 2, h / 2) with sample centres at +0.5 and coefficients rounded to 15 decimals, and both truncate the
bilinear value to uint8; the goldens follow 12.2 (the only version here).

The expected image is stored as the uint8 crop Pillow produces (steps 1-3, exact); `to_input` turns it into the
expected model input (steps 4-5, torch CPU ops), which keeps the file small.  `to_input` and the keypoint maths live in
tests/augment_ref.py, the restatement the tests share; only the Pillow side (`pil_crop`) is kept here.

Sources are blocky PCG64 images (32 x 32 blocks of uniform uint8 noise plus an 8-column stripe of a 1-pixel 0/255
checker), so the file stays small while the block edges and the stripe exercise the bilinear taps and the truncation.
"""
import os
import sys
import zlib

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, 'dsnt-pose2d_amd'), os.path.join(ROOT, 'tests')]

import augment_ref  # noqa: E402
from augment_ref import to_input  # noqa: E402,F401  (steps 4-6; tests/test_augment_gpu.py takes it from here)
from dsnt.inference import HFLIP_INDICES  # noqa: E402  (no HIP needed to import it)

R = 384
J = 16
MEAN = (0.44, 0.44, 0.40)
STD = (0.26, 0.25, 0.27)

# name, S, scale, rot (deg), hflip, gains
CASES = [
    ('identity', 256, 1.0, 0.0, 0, (1.0, 1.0, 1.0)),
    ('flip', 128, 1.0, 0.0, 1, (1.0, 1.0, 1.0)),
    ('scale_down_odd', 128, 0.7475, 0.0, 0, (1.0, 1.0, 1.0)),       # c = int(287.04) = 287 (odd): offset round(48.5) = 48
    ('scale_up_odd', 128, 1.3, 0.0, 0, (1.0, 1.0, 1.0)),          # c = 499: offset round(-57.5) = -58, zero border
    ('scale_min', 128, 0.7071067811865476, 0.0, 1, (1.0, 1.0, 1.0)),
    ('scale_max', 128, 1.4142135623730951, 0.0, 0, (0.8, 1.1, 1.25)),
    ('rot_p7.5', 128, 1.0, 7.5, 0, (1.0, 1.0, 1.0)),
    ('rot_m7.5', 128, 1.0, -7.5, 0, (1.0, 1.0, 1.0)),
    ('rot_p30', 128, 1.0, 30.0, 0, (1.0, 1.0, 1.0)),
    ('rot_m30', 128, 1.0, -30.0, 1, (1.0, 1.0, 1.0)),
    ('rot_60_gain_clamp', 128, 0.9, 60.0, 0, (0.6, 1.4, 5.0)),     # gain 5: most of the blue channel clamps at 1
    ('full', 256, 1.1893, -23.25, 1, (1.37, 0.61, 1.02)),
]


def _rng(name):
    return np.random.Generator(np.random.PCG64([11, zlib.crc32(name.encode())]))


def source(name):
    r = _rng('src.' + name)
    base = r.integers(0, 256, (R // 32, R // 32, 3), dtype=np.uint8)
    img = np.repeat(np.repeat(base, 32, 0), 32, 1)
    img[:, 100:108] = np.where((np.arange(R)[:, None, None] + np.arange(8)[None, :, None]) % 2, 255, 0)
    return np.ascontiguousarray(img)


def bb_matrix(name):
    """A bounding-box transform of the `get_bb_transform` kind: original-image pixels -> [-1, 1] box coordinates."""
    r = _rng('bb.' + name)
    cx, cy, side = r.uniform(300, 900), r.uniform(200, 600), r.uniform(150, 500)
    return np.array([[2 / side, 0, -2 * cx / side], [0, 2 / side, -2 * cy / side], [0, 0, 1]], np.float64)


def keypoints(name, m):
    r = _rng('kp.' + name)
    inv = np.linalg.inv(m)
    box = r.uniform(-1.3, 1.3, (J, 2))                 # some joints land outside the box
    kp = np.concatenate([box, np.ones((J, 1))], 1) @ inv.T
    mask = (r.random(J) < 0.85).astype(np.uint8)
    return kp[:, :2].copy(), mask


def pil_crop(src, scale, rot, hflip):
    """Steps 1-3 with Pillow: the uint8 crop [c, c, 3] the reference's ToTensor receives."""
    R = src.shape[0]
    img = Image.fromarray(src)
    if hflip:
        img = img.transpose(Image.Transpose.FLIP_LEFT_RIGHT)
    if rot != 0:
        img = img.rotate(rot, Image.Resampling.BILINEAR)
    c = int(R * scale)
    off = int(round((R - c) / 2.0))
    return np.asarray(img.crop((off, off, off + c, off + c))).copy()


def transform_image(src, scale, rot, hflip, gain, S, mean=MEAN, std=STD):
    """Steps 1-5: the model input [3, S, S] f32."""
    return augment_ref.to_input(pil_crop(src, scale, rot, hflip), gain, S, mean, std)


def transform_keypoints(kp, matrix, kmask, scale, rot, hflip, train=True):
    """data.py:150-196 in fp64 with the MPII flip table: (part_coords f64 [J,2], part_mask [J], trans_m, trans_b)."""
    return augment_ref.keypoints(kp, matrix, kmask, scale, rot, hflip, HFLIP_INDICES.numpy(), train)


def make():
    out = {'mean': np.array(MEAN, np.float32), 'std': np.array(STD, np.float32), 'R': np.int64(R),
           'names': np.array([c[0] for c in CASES])}
    for name, S, scale, rot, hflip, gain in CASES:
        scale, rot = float(np.float32(scale)), float(np.float32(rot))      # the kernel's parameters are fp32
        gain = tuple(float(g) for g in np.float32(gain))
        src = source(name)
        crop = pil_crop(src, scale, rot, hflip)
        m = bb_matrix(name)
        kp, km = keypoints(name, m)
        pc, pm, tm, tb = transform_keypoints(kp, m, km, scale, rot, hflip)
        p = name + '.'
        out.update({p + 'src': src, p + 'S': np.int64(S), p + 'scale': np.float32(scale), p + 'rot': np.float32(rot),
                    p + 'hflip': np.uint8(hflip), p + 'gain': np.array(gain, np.float32),
                    p + 'matrix': m, p + 'keypoints': kp, p + 'keypoint_mask': km,
                    p + 'crop': crop, p + 'part_coords': pc.astype(np.float32),
                    p + 'part_coords_f64': pc, p + 'part_mask': pm.astype(np.float32), p + 'trans_m': tm,
                    p + 'trans_b': tb})
    return out


if __name__ == '__main__':
    path = os.path.join(HERE, 'augment.npz')
    np.savez_compressed(path, **make())
    print(path, os.path.getsize(path))
