"""numpy restatement of dsnt_joint_confusion and dsnt_target_mass (csrc/pckh.hip; rules in DESIGN.md section 21), and the
inputs of tests/test_confusion_cpu.py, tests/test_confusion_gpu.py and tests/test_target_mass_gpu.py.

Everything here is fp64 numpy on the host, one rounded operation at a time: `x * m00 + y * m10 + b0` left to right, the
squared differences, their sum, the root, the division by the head length.  The device may contract a multiply and an
add of that expression, so the generated cases keep every decision 1e-9 relative away from its edge (`margins`,
`mass_margin`; asserted over the fixed seeds by tests/test_confusion_cpu.py); the hand-built cases are in integers that
every order of operations computes exactly.
"""
import math

import numpy as np

THR = 0.5
MPII_MIRROR = [5, 4, 3, 2, 1, 0, 6, 7, 8, 9, 15, 14, 13, 12, 11, 10]      # dsnt.inference.HFLIP_INDICES


def mirror_of(J):
    """The mirror the tests use for J joints: MPII's for 16 (and for the first 16 of 17), pairs (2i, 2i + 1) for 64, joint
    0 alone and 1 <-> 2 for 3, 0 <-> 1 for 2, nothing for 1."""
    if J in (16, 17):
        return MPII_MIRROR + list(range(16, J))
    if J == 3:
        return [0, 2, 1]
    if J == 1:
        return [0]
    assert J % 2 == 0
    return [j ^ 1 for j in range(J)]


def f32(value):
    """A threshold as the kernels hold it: the fp64 value of its fp32 rounding."""
    return float(np.float32(value))


def project(xy, m, b):
    """Back-projection of points [B, K, 2] (any float type, widened to fp64) by m [B, 2, 2], b [B, 2]: row vector times
    matrix plus offset -> (ox, oy), each [B, K]."""
    x, y = xy[..., 0].astype(np.float64), xy[..., 1].astype(np.float64)
    with np.errstate(all='ignore'):
        return (x * m[:, None, 0, 0] + y * m[:, None, 1, 0] + b[:, None, 0],
                x * m[:, None, 0, 1] + y * m[:, None, 1, 1] + b[:, None, 1])


def distances(pred, target, m, b, head):
    """d[n, j, k]: prediction j of person n against the target of joint k, in head lengths, f64 [B, J, J]."""
    ox, oy = project(pred, m, b)
    gx, gy = project(target, m, b)
    with np.errstate(all='ignore'):
        dx, dy = ox[:, :, None] - gx[:, None, :], oy[:, :, None] - gy[:, None, :]
        return np.sqrt(dx * dx + dy * dy) / head[:, None, None]


def cells(pred, target, m, b, mask, head, thr=THR):
    """The column of every joint, int [B, J]: -1 where the joint is not counted.  A plain loop over persons and joints."""
    B, J = mask.shape
    t, d = f32(thr), distances(pred, target, m, b, head)
    out = np.full((B, J), -1, np.int64)
    for n in range(B):
        for j in range(J):
            if mask[n, j] != 1:
                continue
            c = J
            if d[n, j, j] <= t:
                c = j
            else:
                best = math.inf
                for k in range(J):
                    if k != j and mask[n, k] == 1 and d[n, j, k] <= t and d[n, j, k] < best:
                        best, c = d[n, j, k], k
            out[n, j] = c
    return out


def restate(pred, target, m, b, mask, head, mirror, thr=THR, start=None):
    """(table int64 [J, J + 1], mutual int64 [J]) of one batch, added to `start`."""
    B, J = mask.shape
    col = cells(pred, target, m, b, mask, head, thr)
    table, mutual = (np.zeros((J, J + 1), np.int64), np.zeros(J, np.int64)) if start is None else (start[0].copy(), start[1].copy())
    for n in range(B):
        for j in range(J):
            if col[n, j] < 0:
                continue
            table[j, col[n, j]] += 1
            mj = mirror[j]
            if mj != j and col[n, j] == mj and col[n, mj] == j:
                mutual[j] += 1
    return table, mutual


def kinds(table, mutual, mirror):
    """How many joints of each kind a pair of tables holds: dict of hit, mirror, other, nowhere, mutual."""
    J = len(mirror)
    hit = int(np.trace(table[:, :J]))
    mir = int(sum(table[j, mirror[j]] for j in range(J) if mirror[j] != j))
    nowhere = int(table[:, J].sum())
    return {'hit': hit, 'mirror': mir, 'other': int(table.sum()) - hit - mir - nowhere, 'nowhere': nowhere,
            'mutual': int(mutual.sum())}


def margins(pred, target, m, b, mask, head, thr=THR):
    """(the smallest |d_jk - t| / t, the smallest relative gap between two distances of one joint that are candidates or
    nearly so: d <= 2 t) over the counted j and annotated k with a finite distance."""
    t, d = f32(thr), distances(pred, target, m, b, head)
    B, J = mask.shape
    edge, gap = math.inf, math.inf
    for n in range(B):
        ann = mask[n] == 1
        for j in np.nonzero(ann)[0]:
            row = d[n, j][ann]
            row = np.sort(row[np.isfinite(row)])
            if row.size:
                edge = min(edge, float(np.abs(row - t).min() / t))
            near = row[row <= 2 * t]
            if near.size > 1:
                gap = min(gap, float((np.diff(near) / near[1:]).min()))
    return edge, gap


def transforms(r, B):
    """A transform per person that is no similarity: a rotation, an anisotropic scale and an offset; and head lengths."""
    a = r.uniform(0, 2 * np.pi, B)
    sx, sy = r.uniform(120, 180, B), r.uniform(60, 110, B)
    rot = np.stack([np.stack([np.cos(a), np.sin(a)], -1), np.stack([-np.sin(a), np.cos(a)], -1)], -2)
    m = rot * np.stack([sx, sy], -1)[:, :, None]              # diag(sx, sy) @ rot: x is stretched before it is turned
    return m, r.uniform(0, 400, (B, 2)), r.uniform(40, 120, B)


def case(B, J, seed):
    """(pred, target, m, b, mask, head) with every kind of joint in it.  Per joint one of: a hit (the target and a little
    noise), a prediction on the mirror joint's target, on another joint's target, far from everything, or NaN; per
    mirrored pair sometimes an exchange or a collapse of both onto one of the two.  Masks of 0, 1, 0.5 and 2, persons
    with every joint masked, and NaN targets wherever the mask is not 1."""
    r = np.random.default_rng(seed)
    mirror = np.array(mirror_of(J))
    target = r.uniform(-0.9, 0.9, (B, J, 2))
    noise = r.normal(0, 0.03, (B, J, 2))
    kind = r.choice(6, (B, J), p=[0.45, 0.15, 0.15, 0.15, 0.05, 0.05])
    other = (np.arange(J)[None, :] + r.integers(1, max(J, 2), (B, J))) % J        # another joint (itself when J == 1)
    onto = np.where(kind == 1, mirror[None, :], np.where(kind == 2, other, np.arange(J)[None, :]))
    pair = r.choice(3, (B, J), p=[0.7, 0.2, 0.1])                                  # per pair, read at its smaller index
    for j in range(J):
        mj = mirror[j]
        if mj > j:
            onto[:, j] = np.where(pair[:, j] == 1, mj, np.where(pair[:, j] == 2, j, onto[:, j]))
            onto[:, mj] = np.where(pair[:, j] == 1, j, np.where(pair[:, j] == 2, j, onto[:, mj]))
            kind[:, j] = np.where(pair[:, j] > 0, 0, kind[:, j])
            kind[:, mj] = np.where(pair[:, j] > 0, 0, kind[:, mj])
    pred = np.take_along_axis(target, onto[:, :, None].repeat(2, 2), 1) + noise
    pred = np.where((kind == 3)[:, :, None], target + r.uniform(1.0, 2.0, (B, J, 2)) * r.choice([-1, 1], (B, J, 2)), pred)
    pred = np.where((kind == 4)[:, :, None], np.nan, pred)
    pred[..., 1] = np.where(kind == 5, np.nan, pred[..., 1])
    mask = r.choice(np.array([0, 1, 1, 1, 1, 1, 0.5, 2], np.float32), (B, J))
    mask[r.random(B) < 0.1] = 0                                                    # nobody annotated
    mask[2 % B] = 0
    target = np.where((mask == 1)[:, :, None], target, np.nan)
    m, b, head = transforms(r, B)
    return pred.astype(np.float32), target.astype(np.float32), m, b, mask, head


# (B, J) of tests/test_confusion_gpu.py: a pass of a workgroup takes 256 // J persons, and 64 workgroups stride
SHAPES = [(255, 1), (256, 1), (257, 1), (84, 3), (85, 3), (86, 3), (15, 16), (16, 16), (17, 16), (1025, 16),
          (14, 17), (15, 17), (16, 17), (3, 64), (4, 64), (5, 64), (257, 64)]
SEEDS = {}                                                     # (B, J) -> seed, where the default B * 100 + J does not do


def shape_case(B, J):
    return case(B, J, SEEDS.get((B, J), B * 100 + J))


def hand(rows, J=3, heads=10.0):
    """A batch in exact numbers: `rows` of persons, each a list of J (pred xy, target xy, mask); identity transform."""
    B = len(rows)
    pred = np.array([[q[0] for q in p] for p in rows], np.float32).reshape(B, J, 2)
    target = np.array([[q[1] for q in p] for p in rows], np.float32).reshape(B, J, 2)
    mask = np.array([[q[2] for q in p] for p in rows], np.float32).reshape(B, J)
    return pred, target, np.tile(np.eye(2), (B, 1, 1)), np.zeros((B, 2)), mask, np.full(B, heads, np.float64)


NAN = float('nan')
FAR = (900.0, 900.0)
# name -> (one person of 3 joints with the mirror [0, 2, 1], head length 10, threshold 0.5: within 5;
#          the cells (j, column) that hold 1; mutual)
HAND = {
    # 3-4-5: the distance is 5 / 10 = 0.5 exactly, and <= holds
    'at_threshold': ([((0, 0), (3, 4), 1), (FAR, (0, 90), 0), (FAR, (90, 0), 0)], [(0, 0)], [0, 0, 0]),
    # (3, 4) and (5, 0) are both 5 away: the smaller index
    'tie': ([((0, 0), (500, 500), 1), ((3, 4), (3, 4), 1), ((5, 0), (5, 0), 1)], [(0, 1), (1, 1), (2, 2)], [0, 0, 0]),
    'tie_other_way': ([((0, 0), (500, 500), 1), ((5, 0), (5, 0), 1), ((3, 4), (3, 4), 1)], [(0, 1), (1, 1), (2, 2)],
                      [0, 0, 0]),
    # joint 1's target is 1.4 away and not annotated: it attracts nothing
    'unannotated': ([((0, 0), (500, 500), 1), ((1, 1), (1, 1), 0), ((90, 0), (90, 0), 1)], [(0, 3), (2, 2)], [0, 0, 0]),
    'nan_target_masked': ([((0, 0), (500, 500), 1), ((1, 1), (NAN, NAN), 0), ((90, 0), (90, 0), 1)], [(0, 3), (2, 2)],
                          [0, 0, 0]),
    'nan_prediction': ([((NAN, 0), (0, 0), 1), ((0, NAN), (0, 0), 1), ((90, 0), (90, 0), 1)], [(0, 3), (1, 3), (2, 2)],
                       [0, 0, 0]),
    'exchange': ([((0, 50), (0, 50), 1), ((20, 0), (0, 0), 1), ((0, 0), (20, 0), 1)], [(0, 0), (1, 2), (2, 1)], [0, 1, 1]),
    # both predictions on joint 1's target: joint 1 hits, joint 2 landed on its mirror, nothing was exchanged
    'collapse': ([((0, 50), (0, 50), 1), ((0, 0), (0, 0), 1), ((0, 1), (20, 0), 1)], [(0, 0), (1, 1), (2, 1)], [0, 0, 0]),
    # the exchange again with joint 1 masked 0.5: it is not counted, attracts nothing and exchanges nothing
    'partner_masked': ([((0, 50), (0, 50), 1), ((20, 0), (0, 0), 0.5), ((0, 0), (20, 0), 1)], [(0, 0), (2, 3)], [0, 0, 0]),
}
HAND_MIRROR = [0, 2, 1]


def hand_tables(name):
    ones, mutual = HAND[name][1:]
    table = np.zeros((3, 4), np.int64)
    for j, c in ones:
        table[j, c] += 1
    return table, np.array(mutual, np.int64)


# ------------------------------------------------------------------ dsnt_target_mass
def pixel_distances(h, w, gxy, m, b, head):
    """Distance in head lengths of every pixel centre of an h x w map of one person to the back-projected point gxy
    (fp64 pair): f64 [h, w].  The centres are dsnt.nn.generate_xy's: (2c + 1 - w) / w, (2r + 1 - h) / h."""
    x = ((2 * np.arange(w) + 1 - w) / w)[None, :]
    y = ((2 * np.arange(h) + 1 - h) / h)[:, None]
    with np.errstate(all='ignore'):
        ox, oy = x * m[0, 0] + y * m[1, 0] + b[0], x * m[0, 1] + y * m[1, 1] + b[1]
        dx, dy = ox - gxy[0], oy - gxy[1]
        return np.sqrt(dx * dx + dy * dy) / head


def restate_mass(hm, target, m, b, mask, head, mirror, thr=THR):
    """(out f32 [B, J, 2], pixels int64 [B, J, 2]: how many pixel centres each disc holds, -1 where out is NaN, margin:
    the smallest |d - t| / t over every pixel of every disc that is summed).  The sums are exact (math.fsum), then
    rounded to fp32 once."""
    B, J, h, w = hm.shape
    t = f32(thr)
    gx, gy = project(target, m, b)
    out = np.full((B, J, 2), np.nan, np.float32)
    pixels = np.full((B, J, 2), -1, np.int64)
    margin = math.inf
    for n in range(B):
        for j in range(J):
            if mask[n, j] != 1:
                continue
            mj = mirror[j]
            for s, k in enumerate((j, mj)):
                if s == 1 and (mj == j or mask[n, mj] != 1):
                    continue
                d = pixel_distances(h, w, (gx[n, k], gy[n, k]), m[n], b[n], head[n])
                inside = d <= t
                if t > 0 and np.isfinite(d).any():
                    margin = min(margin, float(np.abs(d[np.isfinite(d)] - t).min() / t))
                out[n, j, s] = np.float32(math.fsum(hm[n, j].astype(np.float64)[inside].tolist()))
                pixels[n, j, s] = int(inside.sum())
    return out, pixels, margin


def softmax_maps(logits):
    """Softmax over the pixels of f32 logits [B, J, h, w], in fp32."""
    z = logits.astype(np.float32)
    z = np.exp(z - z.max((2, 3), keepdims=True))
    return (z / z.sum((2, 3), keepdims=True)).astype(np.float32)


def mass_case(B, J, h, w, seed):
    """(hm, target, m, b, mask, head): softmax maps of seeded logits; targets inside the frame, some well outside it (a
    disc that holds no pixel), some head lengths so short that a disc falls between the pixel centres; masks of 0, 1 and
    0.5.  Map (0, 0) is bimodal: one mode on its own target, one on its mirror's."""
    r = np.random.default_rng(seed)
    mirror = mirror_of(J)
    target = r.uniform(-0.8, 0.8, (B, J, 2))
    target = np.where((r.random((B, J)) < 0.15)[:, :, None], target + 4.0, target)          # outside the map
    m, b, head = transforms(r, B)
    head = np.where(r.random(B) < 0.34, r.uniform(0.5, 2.0, B), head)                        # tiny discs
    mask = r.choice(np.array([0, 1, 1, 1, 0.5], np.float32), (B, J))
    mask[0, 0] = 1
    mask[0, mirror[0]] = 1
    target[0, 0], target[0, mirror[0]] = (-0.4, 0.3), (0.45, -0.35)
    head[0] = 100.0
    if B * J > 2:                                             # the last person's joint 1: counted, outside the map, and
        mask[B - 1, 1], mask[B - 1, mirror[1]] = 1, 0          # its partner not annotated
        target[B - 1, 1] = (4.0, -3.5)
    logits = r.normal(0, 1.0, (B, J, h, w))
    x, y = (2 * np.arange(w) + 1 - w) / w, (2 * np.arange(h) + 1 - h) / h
    for (tx, ty), peak in ((target[0, 0], 11.4), (target[0, mirror[0]], 11.0)):      # the pixel nearest to each target
        logits[0, 0, np.abs(y - ty).argmin(), np.abs(x - tx).argmin()] = peak
    return softmax_maps(logits), target.astype(np.float32), m, b, mask, head


def mass_pred(target, seed=11):
    """Predictions to go with the targets of `mass_case`: about as many hits as misses at 0.5 head lengths."""
    return (target + np.random.default_rng(seed).normal(0, 0.2, target.shape)).astype(np.float32)


MASS_SHAPES = [(B, J, h, w) for (h, w) in ((8, 8), (5, 7), (64, 64), (16, 260)) for B in (1, 3) for J in (2, 16)]
MASS_SEEDS = {}                                                # shape -> seed, where the default does not do


def mass_shape_case(B, J, h, w):
    return mass_case(B, J, h, w, MASS_SEEDS.get((B, J, h, w), 7000 + 1000 * B + 10 * J + h))
