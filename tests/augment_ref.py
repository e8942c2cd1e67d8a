"""Restatement of the training augmentation (csrc/augment.hip, reference `src/dsnt/data.py:118-226`): numpy, plus torch
CPU ops where the reference step itself is an ATen op.  It imports neither Pillow nor the library, so it loads
anywhere.  tests/test_augment_cpu.py pins `crop` to Pillow bit for bit and `keypoints` to the reference's torch
formulation; tests/golden/make_augment_golden.py and the GPU tests use it as the expected side.

The steps are numbered as in the header of csrc/augment.hip: 1 flip, 2 rotate, 3 centre crop (`crop`); 4 ToTensor, gain,
clamp, 5 adaptive pool, 6 normalise (`to_input`); the keypoint maths (`keypoints`); the parameter draw (`draw`)."""
import math

import numpy as np
import torch
import torch.nn.functional as Fn

import loader_ref


def rotate(img, rot):
    """Step 2, Pillow's `Image.rotate(rot, BILINEAR)` of a square uint8 [R, R, 3] image as the kernel samples it."""
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


def crop_side(R, scale):
    """c = int(R * scale), with the kernel's clamp: R * scale below 1 or NaN gives 1, above 8R gives 8R."""
    cd = float(R) * float(scale)
    if 1.0 <= cd <= 8.0 * R:
        return int(cd)
    return 8 * R if cd > 1.0 else 1


def crop(src, scale, rot, hflip):
    """Steps 1-3 on a uint8 [R, R, 3] source: the uint8 crop [c, c, 3] the reference's ToTensor receives."""
    R = src.shape[0]
    img = src[:, ::-1] if hflip else src
    if rot % 360.0 != 0:
        img = rotate(img, rot)
    c = crop_side(R, scale)
    off = int(round((R - c) / 2.0))                       # Python 3: half to even
    out = np.zeros((c, c, 3), np.uint8)                   # Image.crop zero-fills outside the image
    lo, hi = max(0, -off), min(c, R - off)
    if hi > lo:
        out[lo:hi, lo:hi] = img[lo + off:hi + off, lo + off:hi + off]
    return out


def to_input(crop, gain, S, mean, std):
    """Steps 4-6 with torch CPU ops on the uint8 crop: the model input [3, S, S] f32."""
    x = torch.from_numpy(np.ascontiguousarray(crop)).permute(2, 0, 1).contiguous().float().div(255)
    for ch in range(3):
        x[ch].mul_(float(gain[ch])).clamp_(0, 1)
    out = Fn.adaptive_avg_pool2d(x, S)
    for ch in range(3):
        out[ch].sub_(float(mean[ch])).div_(float(std[ch]))
    return out.numpy()


def aug_matrix(scale, rot, hflip):
    t = np.eye(3)
    if hflip:
        t = np.array([[-1.0, 0, 0], [0, 1, 0], [0, 0, 1]]) @ t
    a = np.radians(rot)
    return np.array([[np.cos(a) / scale, np.sin(a) / scale, 0], [-np.sin(a) / scale, np.cos(a) / scale, 0],
                     [0, 0, 1]]) @ t


def keypoints(kp, matrix, kmask, scale, rot, hflip, flip_idx, train=True):
    """data.py:150-196 in fp64: (part_coords f64 [J,2], part_mask [J], trans_m [2,2], trans_b [1,2]).  `flip_idx` is the
    joint permutation of a flip (int array [J]); it is read only under hflip, so None serves where nothing flips."""
    t = aug_matrix(scale, rot, hflip)
    pc = (np.concatenate([kp, np.ones((len(kp), 1))], 1) @ matrix.T)[:, :2]
    pc = (np.concatenate([pc, np.ones((len(pc), 1))], 1) @ t.T)[:, :2]
    pm = kmask.astype(np.float64)
    if hflip:
        idx = np.asarray(flip_idx)
        pc2, pm2 = pc.copy(), pm.copy()
        pc2[idx], pm2[idx] = pc, pm            # scatter_(0, idx, src): out[idx[i]] = src[i]
        pc, pm = pc2, pm2
    if train:
        pm = pm * np.all(np.abs(pc) < 1, -1)
    s = np.linalg.inv(matrix) @ np.linalg.inv(t)
    return pc, pm, s[0:2, 0:2].copy(), s[0:2, 2].reshape(1, 2).copy()


def unit(x):
    """(0, 1] from the top 24 bits of a 32-bit word, fp64."""
    return ((np.asarray(x, np.uint64) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * (1.0 / 16777216.0)


def normal(a, b):
    """Box-Muller in fp64, as the kernel writes it."""
    return np.sqrt(-2.0 * np.log(unit(a))) * np.cos(6.283185307179586 * unit(b))


def draw_from_words(r0, r1, r2):
    """The parameters from the three Philox outputs (lists of 4 word arrays): the distributions of data.py:134-140."""
    scale = np.exp2(np.clip(0.25 * normal(r0[0], r0[1]), -0.5, 0.5)).astype(np.float32)
    angle = np.clip(30.0 * normal(r1[0], r1[1]), -60.0, 60.0).astype(np.float32)
    rot = np.where(unit(r0[2]) <= 0.4, angle, np.float32(0))
    hflip = (unit(r0[3]) <= 0.5).astype(np.uint8)
    gain = np.stack([(0.6 + 0.8 * unit(r2[ch])).astype(np.float32) for ch in range(3)], -1)
    return scale, rot, hflip, gain


def draw(seed, step, sample):
    """`draw_params` of csrc/augment.hip: (scale f32, rot f32, hflip u8, gain f32 [.., 3]) of sample word(s) `sample`
    (a 32-bit value or an array of them) at 64-bit `seed` and `step`.  Philox4x32-10 with counter (sample, step lo,
    step hi, k) for k = 0, 1, 2 and key (seed lo, seed hi)."""
    sample = np.asarray(sample, np.uint64) & loader_ref.M32
    lo, hi = step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF
    r0, r1, r2 = (loader_ref.philox4x32_10(sample, lo, hi, k, seed & (2 ** 64 - 1)) for k in range(3))
    return draw_from_words(r0, r1, r2)
