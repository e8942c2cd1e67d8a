"""numpy restatement of dsnt_crop_affine (csrc/augment.hip): the Pillow coefficients of a bounding-box matrix and
Pillow's affine bilinear sampler.  tests/test_crop_cpu.py pins it to Pillow; tests/golden/make_crop_golden.py uses
`coefficients` for the golden crops."""
import numpy as np


def inverse3(m):
    """The kernel's `inverse3`: adjugate over determinant, the same fp64 operations in the same order.
    Returns (inv as 9 Python floats, det)."""
    m = [float(v) for v in np.asarray(m, np.float64).reshape(9)]
    a00, a01, a02 = m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4]
    a10, a11, a12 = m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5]
    a20, a21, a22 = m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]
    det = m[0] * a00 + m[1] * a10 + m[2] * a20
    with np.errstate(all='ignore'):
        inv = [float(np.float64(v) / np.float64(det)) for v in (a00, a01, a02, a10, a11, a12, a20, a21, a22)]
    return inv, det


def coefficients(m, R):
    """Pillow's affine data (a, b, c, d, e, f) of crop size R for matrix m (image px -> [-1, 1]^2), or None when the
    kernel refuses m (determinant 0 or not finite)."""
    inv, det = inverse3(m)
    if det == 0.0 or not np.isfinite(det):
        return None
    return (2 * inv[0] / R, 2 * inv[1] / R, inv[2] - inv[0] - inv[1],
            2 * inv[3] / R, 2 * inv[4] / R, inv[5] - inv[3] - inv[4])


def sample(img, coef, R):
    """Pillow's Image.transform((R, R), AFFINE, coef, BILINEAR) of an H x W x 3 uint8 image, restated: fp64 sample at
    pixel centres, black outside [0, W) x [0, H), taps at floor(v - .5) and +1 clamped (the second row only where it
    exists), lerps a + (b - a) * t along x then y, truncation."""
    H, W = img.shape[:2]
    a, b, c, d, e, f = coef
    ys, xs = np.mgrid[0:R, 0:R].astype(np.float64)
    xo, yo = xs + 0.5, ys + 0.5
    xin = a * xo + b * yo + c
    yin = d * xo + e * yo + f
    inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    xin, yin = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    x0, y0 = np.floor(xin), np.floor(yin)
    dx, dy = (xin - x0)[..., None], (yin - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    cx = lambda v: np.clip(v, 0, W - 1)
    cy = lambda v: np.clip(v, 0, H - 1)
    im = img.astype(np.float64)
    xa, xb = cx(x0), cx(x0 + 1)
    a0, a1 = im[cy(y0), xa], im[cy(y0), xb]
    v1 = a0 + (a1 - a0) * dx
    b0, b1 = im[cy(y0 + 1), xa], im[cy(y0 + 1), xb]
    has2 = ((y0 + 1 >= 0) & (y0 + 1 < H))[..., None]
    v2 = np.where(has2, b0 + (b1 - b0) * dx, v1)
    v = (v1 + (v2 - v1) * dy).astype(np.int64)
    return np.where(inside[..., None], v, 0).astype(np.uint8)


def crop(img, m, R):
    """(crop uint8 [R, R, 3], valid) of image img through matrix m, as dsnt_crop_affine makes it."""
    coef = coefficients(m, R)
    if coef is None:
        return np.zeros((R, R, 3), np.uint8), False
    return sample(img, coef, R), True
