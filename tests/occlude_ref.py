"""numpy restatement of `dsnt_occlude` (construction in include/dsnt_hip.h and csrc/occlude.hip): the integer draw, the
clipping, the three fills and the covered-joint rule.  Shared by tests/test_occlude_cpu.py and tests/test_occlude_gpu.py."""
import numpy as np

import augment_ref
import loader_ref

DOMAIN = 0x4F43434C          # DSNT_OCCLUDE_DOMAIN
MAX_RECTS = 8                # DSNT_OCCLUDE_MAX_RECTS
MAX_JOINTS = 256             # DSNT_OCCLUDE_MAX_JOINTS
FILLS = {'value': 0, 'noise': 1, 'paste': 2}
CENTRES = {'uniform': 0, 'joint': 1}
M32 = 0xFFFFFFFF


def u24(x):
    return np.asarray(x, np.uint64) >> np.uint64(8)


def pick(x, n):
    """(u24(x) * n) >> 24 in 64 bits: a value in [0, n)."""
    return ((u24(x) * np.uint64(n)) >> np.uint64(24)).astype(np.int64)


def words(g, step, k, seed):
    """P(k): Philox4x32-10 with counter (g, step lo, step hi, DOMAIN + k) and key (seed lo, seed hi)."""
    return loader_ref.philox4x32_10(np.asarray(g, np.uint64) & np.uint64(M32), step & M32, (step >> 32) & M32,
                                    (DOMAIN + k) & M32, seed)


def p24_of(p):
    return int(round(p * 2 ** 24))


def joint_pixels(coords, S):
    """(x, y) int64 [.., J] of normalised fp32 coords [.., J, 2]: floorf((c + 1.f) * (0.5f * S)); -1 for a joint without a
    pixel (NaN or outside [0, S) in either coordinate)."""
    c = np.asarray(coords, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        f = np.floor((c + np.float32(1)) * (np.float32(0.5) * np.float32(S)))
        ok = (f[..., 0] >= 0) & (f[..., 0] < S) & (f[..., 1] >= 0) & (f[..., 1] < S)
    px = np.where(ok, np.where(ok, f[..., 0], 0).astype(np.int64), -1)
    py = np.where(ok, np.where(ok, f[..., 1], 0).astype(np.int64), -1)
    return px, py


def draw(B, S, K, side_min, side_max, p24, seed, step, draw_offset=0, centre='uniform', coords=None, mask=None,
         unclipped=False):
    """(rects int32 [B, K, 4], donor int32 [B]) of a batch; with `unclipped` also the sides (w, h) int64 [B, K] before
    clipping (0 in unused rows)."""
    rects = np.zeros((B, K, 4), np.int32)
    donor = np.zeros(B, np.int32)
    sides = np.zeros((B, K, 2), np.int64)
    J = 0 if coords is None else np.asarray(coords).shape[1]
    if J:
        px, py = joint_pixels(coords, S)
    for b in range(B):
        g = (draw_offset + b) & M32
        A = [int(w) for w in words(g, step, 0, seed)]
        count = 1 + int(pick(A[1], K)) if int(u24(A[0])) < p24 else 0
        donor[b] = (b + 1 + int(pick(A[2], B - 1))) % B if B > 1 else b
        valid = []
        if centre == 'joint' and J:
            valid = [j for j in range(J) if px[b, j] >= 0 and np.asarray(mask, np.float32)[b, j] != 0]
        for r in range(count):
            R = [int(w) for w in words(g, step, 1 + r, seed)]
            w = side_min + int(pick(R[0], side_max - side_min + 1))
            h = side_min + int(pick(R[1], side_max - side_min + 1))
            if valid:
                j = valid[int(pick(R[2], len(valid)))]
                cx, cy = int(px[b, j]), int(py[b, j])
            else:
                cx, cy = int(pick(R[2], S)), int(pick(R[3], S))
            rects[b, r] = (max(cx - w // 2, 0), max(cy - h // 2, 0), min(cx - w // 2 + w, S), min(cy - h // 2 + h, S))
            sides[b, r] = (w, h)
    return (rects, donor, sides) if unclipped else (rects, donor)


def clamp_given(rects, donor, B, S):
    """What the kernel makes of given rects / donor: every coordinate into [0, S], every donor into [0, B)."""
    return np.clip(np.asarray(rects, np.int64), 0, S).astype(np.int32), np.clip(np.asarray(donor, np.int64), 0, B - 1).astype(np.int32)


def cover(rects, S):
    """bool [B, S, S]: pixel (y, x) lies in some rectangle of the sample (empty rectangles cover nothing)."""
    B, K = rects.shape[:2]
    m = np.zeros((B, S, S), bool)
    for b in range(B):
        for x0, y0, x1, y1 in rects[b]:
            if x1 > x0 and y1 > y0:
                m[b, y0:y1, x0:x1] = True
    return m


def noise(S, seed, step, g, mean, std):
    """f32 [3, S, S]: the noise fill of the sample with draw word g, at every pixel."""
    Nw = [int(w) for w in words(g, step, 9, seed)]
    ns = Nw[0] | (Nw[1] << 32)
    q = np.arange(S * S, dtype=np.uint64)
    o = loader_ref.philox4x32_10(q, step & M32, (step >> 32) & M32, (DOMAIN + 10) & M32, ns)
    out = np.empty((3, S * S), np.float32)
    for c in range(3):
        u = augment_ref.unit(o[c]).astype(np.float32)          # (u24 + 1) * 2^-24: exact in fp32
        out[c] = (u - np.float32(mean[c])) / np.float32(std[c])
    return out.reshape(3, S, S)


def occluded_joints(rects, coords, S):
    """uint8 [B, J]: the joint's pixel lies in some rectangle (whatever its mask; no pixel: never covered)."""
    B = rects.shape[0]
    J = np.asarray(coords).shape[1]
    out = np.zeros((B, J), np.uint8)
    if J == 0:
        return out
    px, py = joint_pixels(coords, S)
    m = cover(rects, S)
    for b in range(B):
        for j in range(J):
            if px[b, j] >= 0:
                out[b, j] = m[b, py[b, j], px[b, j]]
    return out


def apply(x, rects, donor, fill, seed=0, step=0, draw_offset=0, fill_value=(0, 0, 0), mean=(0, 0, 0), std=(1, 1, 1)):
    """The occluded batch, as int32 bit patterns [B, 3, S, S], of x f32 [B, 3, S, S] (NaN payloads survive: the copy is
    done on the bits).  rects / donor as the kernel uses them (drawn, or given and clamped)."""
    bits = np.ascontiguousarray(x, np.float32).view(np.int32)
    B, _, S, _ = bits.shape
    out = bits.copy()
    m = cover(rects, S)
    for b in range(B):
        if not m[b].any():
            continue
        if fill == 'value':
            src = np.broadcast_to(np.asarray(fill_value, np.float32).view(np.int32)[:, None, None], (3, S, S))
        elif fill == 'noise':
            src = noise(S, seed, step, (draw_offset + b) & M32, mean, std).view(np.int32)
        else:
            src = bits[int(donor[b])]
        for c in range(3):
            out[b, c][m[b]] = src[c][m[b]]
    return out


def occlude(x, coords, mask, step, K=2, side_min=1, side_max=1, p24=1 << 24, fill='value', centre='uniform', seed=0,
            draw_offset=0, fill_value=(0, 0, 0), mean=(0, 0, 0), std=(1, 1, 1), rects=None, donor=None):
    """The whole call: (bits int32 [B, 3, S, S], rects, donor, occluded uint8 [B, J]).  Given `rects` (and `donor`) nothing is
    drawn and the returned rects / donor are the clamped ones the kernel uses."""
    x = np.asarray(x, np.float32)
    B, S = x.shape[0], x.shape[2]
    if rects is None:
        rects, donor = draw(B, S, K, side_min, side_max, p24, seed, step, draw_offset, centre, coords, mask)
    else:
        rects, donor = clamp_given(rects, donor, B, S)
    bits = apply(x, rects, donor, fill, seed, step, draw_offset, fill_value, mean, std)
    return bits, rects, donor, occluded_joints(rects, coords, S)
