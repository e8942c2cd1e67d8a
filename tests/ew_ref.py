"""The element-wise kernels of csrc/bn.hip, resample.hip, flat.hip, optim.hip and csrc/ew_bodies.h restated in numpy fp64, for
tests/test_ew_ref_cpu.py (which pins this file to the torch CPU operators), tests/test_elementwise_edges_gpu.py and
tests/test_bn_finalize_gpu.py (which hold the HIP kernels to it).  No device code: everything here takes and returns numpy arrays on the host.

Layouts are the kernels': NHWC activations, [M][C] rows for the BatchNorm pieces, flat vectors for the optimisers.
Inputs are the kernels' fp32 inputs taken to fp64; where a kernel's result is a selection (pool maximum, ReLU mask,
skipped element) the selection rule is spelled out, where it is arithmetic the fp64 value comes with the a-priori
fp32 rounding bound of the kernel's expression (`U` = 2^-24, `gamma(k)` = k U / (1 - k U): k rounded operations)."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
TILE_ROWS = 128            # csrc/ew_bodies.h: #define TILE_ROWS 128
FLAG_LOSS, FLAG_GRAD = 1, 2   # include/dsnt_hip.h: DSNT_FLAG_LOSS / DSNT_FLAG_GRAD


def gamma(k):
    return k * U / (1.0 - k * U)


# ---------------------------------------------------------------- host-side launch arithmetic (mirrors)
def flat_grid(n, block=256):
    """csrc/common.h `flat_grid()`: workgroups of a flat launch, capped at 4096."""
    g = (n + block - 1) // block
    return 1 if g < 1 else (4096 if g > 4096 else g)


def tile_cgs(tiles, C4):
    """csrc/ew_bodies.h `tile_cgs()`: float4 column groups a tile workgroup covers per pass."""
    return 16 if (tiles < 256 and C4 > 16 and C4 % 16 == 0) else (C4 if C4 < 256 else 256)


def tile_grid_y(tiles, C4):
    """csrc/ew_bodies.h `tile_grid_y()`."""
    c = tile_cgs(tiles, C4)
    return C4 // 16 if (c == 16 and C4 > 16) else 1


def tile_sum_ops(M, C):
    """Additions on the longest path to one tile partial (tile_reduce_kernel / tile_op_stats_body): the rows one lane
    walks, the `rpar` lane partials combined by the tile's first threads, and one for the fma of the second sum."""
    tiles = (M + TILE_ROWS - 1) // TILE_ROWS
    rpar = 256 // tile_cgs(tiles, C // 4)
    rows = min(M, TILE_ROWS)
    return (rows + rpar - 1) // rpar + rpar + 1


def apply_is_fixed(M, C, pro=False):
    """Which bn_act_bwd_apply_kernel the host picks (bn_act_bwd_apply_impl): FIXED when the grid stride is a multiple of
    C / 4; the _pro forms cap the grid at 128.  Returns (fixed, grid)."""
    n4 = M * C // 4
    grid = flat_grid(n4)
    if pro and grid > 128:
        grid = 128
    return (grid * 256) % (C // 4) == 0, grid


# ---------------------------------------------------------------- max-pools
def _pool_scan(taps):
    """ATen's max_pool2d rule over `taps`: a list of (value array, valid mask or None) in scan order.  The index starts at
    the window's first valid tap (255 until one is seen), the maximum at -inf; a tap replaces the maximum when
    `v > max or v != v` — so the first of several equal maxima wins, and a NaN, once taken, stays (nothing is > NaN) unless
    another NaN follows."""
    shape = taps[0][0].shape
    m = np.full(shape, -np.inf, dtype=taps[0][0].dtype)
    k = np.full(shape, 255, dtype=np.uint8)
    for p, (v, ok) in enumerate(taps):
        first = k == 255
        if ok is not None:
            first = first & ok
        k = np.where(first, np.uint8(p), k)
        with np.errstate(invalid='ignore'):
            take = (v > m) | (v != v)
        if ok is not None:
            take = take & ok
        m = np.where(take, v, m)
        k = np.where(take, np.uint8(p), k)
    return m, k


def maxpool2(x):
    """2x2 / stride 2 max-pool of `x` [N][H][W][C] (H, W even).  Returns (values [N][H/2][W/2][C] in x's type, index
    bytes: the winning tap dy * 2 + dx).  Scan order (0,0) (0,1) (1,0) (1,1)."""
    x = np.asarray(x)
    return _pool_scan([(x[:, dy::2, dx::2, :], None) for dy in (0, 1) for dx in (0, 1)])


def maxpool2_bwd(gy, idx, dtype=np.float64):
    """dx [N][2Ho][2Wo][C]: every output's gradient goes to the tap its index byte names (windows do not overlap)."""
    gy = np.asarray(gy, dtype=dtype)
    N, Ho, Wo, C = gy.shape
    dx = np.zeros((N, 2 * Ho, 2 * Wo, C), dtype=dtype)
    for p in range(4):
        dx[:, p // 2::2, p % 2::2, :] = np.where(idx == p, gy, 0)
    return dx


def maxpool3s2(x):
    """3x3 / stride 2 / pad 1 max-pool of `x` [N][H][W][C]: Ho = (H - 1) // 2 + 1.  Returns (values, index bytes: the
    winning tap r * 3 + s of the 3x3 window, padding taps never win).  Border windows have 2, 4 or 6 valid taps."""
    x = np.asarray(x)
    N, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.zeros((N, 2 * Ho + 1, 2 * Wo + 1, C), dtype=x.dtype)
    ok = np.zeros((1, 2 * Ho + 1, 2 * Wo + 1, 1), dtype=bool)
    xp[:, 1:H + 1, 1:W + 1, :] = x
    ok[:, 1:H + 1, 1:W + 1, :] = True
    taps = [(xp[:, r:r + 2 * Ho:2, s:s + 2 * Wo:2, :], np.broadcast_to(ok[:, r:r + 2 * Ho:2, s:s + 2 * Wo:2, :], (N, Ho, Wo, C)))
            for r in range(3) for s in range(3)]
    return _pool_scan(taps)


def maxpool3s2_bwd(gy, idx, H, W, dtype=np.float64):
    """Gather form: every input pixel sums the gradients of every window (at most 2 x 2 of them) that picked it.  Written
    per tap: for one tap the windows land on distinct pixels, so the slice update is a plain sum."""
    gy = np.asarray(gy, dtype=dtype)
    N, Ho, Wo, C = gy.shape
    dxp = np.zeros((N, 2 * Ho + 1, 2 * Wo + 1, C), dtype=dtype)
    for p in range(9):
        r, s = p // 3, p % 3
        dxp[:, r:r + 2 * Ho:2, s:s + 2 * Wo:2, :] += np.where(idx == p, gy, 0)
    return np.ascontiguousarray(dxp[:, 1:H + 1, 1:W + 1, :])


def tie_share(x, pool):
    """Share of windows whose maximum is held by more than one valid tap (`pool`: 2 or 3)."""
    x = np.asarray(x, dtype=np.float64)
    if pool == 2:
        taps = [(x[:, dy::2, dx::2, :], None) for dy in (0, 1) for dx in (0, 1)]
    else:
        N, H, W, C = x.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        xp = np.full((N, 2 * Ho + 1, 2 * Wo + 1, C), -np.inf)
        xp[:, 1:H + 1, 1:W + 1, :] = x
        ok = np.zeros((1, 2 * Ho + 1, 2 * Wo + 1, 1), dtype=bool)
        ok[:, 1:H + 1, 1:W + 1, :] = True
        taps = [(xp[:, r:r + 2 * Ho:2, s:s + 2 * Wo:2, :], ok[:, r:r + 2 * Ho:2, s:s + 2 * Wo:2, :]) for r in range(3) for s in range(3)]
    with np.errstate(invalid='ignore'):
        m = np.max(np.stack([np.where(ok, v, -np.inf) if ok is not None else v for v, ok in taps]), 0)
        hits = sum(((v == m) & (ok if ok is not None else True)).astype(np.int64) for v, ok in taps)
    return float((hits > 1).mean())


# ---------------------------------------------------------------- BatchNorm: tile sums
def _by_tile(t, M, C, rows=TILE_ROWS):
    tiles = (M + rows - 1) // rows
    pad = np.zeros((tiles * rows, C), dtype=np.float64)
    pad[:M] = t
    return pad.reshape(tiles, rows, C)


def tile_sums_of(t1, t2, M, C, rows=TILE_ROWS):
    """Per 128-row tile and channel, in fp64: (sum t1, sum t2, sum |t1|, sum |t2|), each [tiles][C].  (`rows`: another tile
    height, for hand-made partials of many tiles from a small x.)"""
    a, b = _by_tile(t1, M, C, rows), _by_tile(t2, M, C, rows)
    return a.sum(1), b.sum(1), np.abs(a).sum(1), np.abs(b).sum(1)


def tile_sums(x, M, C, rows=TILE_ROWS):
    """dsnt_bn_stats: (sum x, sum x^2, sum |x|, sum x^2) per tile and channel from the fp32 `x` [M][C]."""
    x = np.asarray(x, dtype=np.float64).reshape(M, C)
    return tile_sums_of(x, x * x, M, C, rows)


def relu_mask(x, scale, shift):
    """The ReLU mask of y = relu(bn(x)) as the kernels take it: `fma(x, scale, shift) <= 0` in fp32.  x * scale is exact
    in fp64 and the sum is rounded once, so the SIGN is that of the exact value, which the fp32 fma has too.  Returns
    (dead [M][C] bool, undecidable [M][C] bool): undecidable where |fma| < 4 * 2^-24 * (|x * scale| + |shift|) — there
    another correct fp32 program (scale and shift rounded in another order) may land on the other side of zero."""
    x = np.asarray(x, dtype=np.float64)
    sc, sh = np.asarray(scale, dtype=np.float64), np.asarray(shift, dtype=np.float64)
    z = (x * sc + sh).astype(np.float32).astype(np.float64)
    return z <= 0, np.abs(z) < 4 * U * (np.abs(x * sc) + np.abs(sh))


def bn_bwd_tile_sums(dz, x, mean, invstd, M, C):
    """dsnt_bn_act_bwd_reduce / dsnt_bn_add_act_bwd_reduce: (sum dz, sum dz * xhat, sum |dz|, sum |dz * xhat|) per tile and
    channel, xhat = (x - mean) * invstd, `dz` already masked.  (The kernel rounds xhat twice before the fma: two more
    operations on the second sum than tile_sum_ops() counts.)"""
    dz = np.asarray(dz, dtype=np.float64).reshape(M, C)
    xh = (np.asarray(x, dtype=np.float64).reshape(M, C) - np.asarray(mean, dtype=np.float64)) * np.asarray(invstd, dtype=np.float64)
    return tile_sums_of(dz, dz * xh, M, C)


# ---------------------------------------------------------------- BatchNorm: apply
APPLY_OPS = 6      # sc * (dz - c0 - (x - mu) * is * c1): sub, mul, mul | sub, sub | mul — six rounded operations; + 1 with a base


def bn_apply(da, x, scale, shift, mean, invstd, coef, relu, base=None):
    """dsnt_bn_act_bwd_apply in fp64: dx = scale * (dz - c0 - xhat * c1) (+ base), dz = da where the ReLU is alive.
    `coef` [2][C] = (c0, c1).  Returns (dx, undecidable mask — all False without relu —, bound): |fp32 result - dx| <=
    bound element by element, bound = gamma(k) * (|scale| * (|dz| + |c0| + |xhat * c1|) + |base|), k = APPLY_OPS (+ 1)."""
    da, x = np.asarray(da, dtype=np.float64), np.asarray(x, dtype=np.float64)
    sc, mu, is_ = (np.asarray(v, dtype=np.float64) for v in (scale, mean, invstd))
    c = np.asarray(coef, dtype=np.float64)
    c0, c1 = c[0], c[1]
    und = np.zeros(x.shape, dtype=bool)
    dz = da
    if relu:
        dead, und = relu_mask(x, scale, shift)
        dz = np.where(dead, 0.0, da)
    t = (x - mu) * is_ * c1
    dx = sc * (dz - c0 - t)
    mag = np.abs(sc) * (np.abs(dz) + np.abs(c0) + np.abs(t))
    k = APPLY_OPS
    if base is not None:
        b = np.asarray(base, dtype=np.float64)
        dx = dx + b
        mag = mag + np.abs(b)
        k += 1
    return dx, und, gamma(k) * mag


# ---------------------------------------------------------------- optimisers and the non-finite guard
def _f32(v):
    return float(np.float32(v))


def _guard(g, grad_scale, flag):
    """(blocked, skip mask or None, flag after).  flag[0] != 0 on entry: nothing changes.  An element whose fp32
    g * grad_scale is not finite is skipped and raises FLAG_GRAD in flag[1]."""
    if flag is None:
        return False, None, None
    flag = [int(flag[0]), int(flag[1])]
    if flag[0] != 0:
        return True, None, flag
    with np.errstate(over='ignore', invalid='ignore'):
        skip = ~np.isfinite(np.asarray(g, dtype=np.float32) * np.float32(grad_scale))
    if skip.any():
        flag[1] |= FLAG_GRAD
    return False, skip, flag


def rmsprop_step(p, g, sq, lr, alpha=0.99, eps=1e-8, weight_decay=0.0, grad_scale=1.0, flag=None):
    """dsnt_rmsprop_step (flag None) / _guarded: torch.optim.RMSprop without momentum or centring, on fp32 inputs in fp64;
    the hyper-parameters are the fp32 values the C ABI receives.

        gi = g * grad_scale (+ weight_decay * p);  s = alpha * sq + (1 - alpha) * gi * gi;  p -= lr * gi / (sqrt(s) + eps)

    Returns a dict: p, sq (fp64; skipped or blocked elements hold their input), flag, skip, and the fp32 rounding bounds
    bound_sq = gamma(9) * S, S = alpha sq + (1 - alpha) G^2, G = |g grad_scale| + |weight_decay p| (nine rounded operations
    reach s: scale and fma of gi, counted for both factors, 1 - alpha, two products, alpha * sq, the sum) and
    bound_p = gamma(1) * [ |p| + (lr G / D) * (7 + 4.5 * (S / s) * sqrt(s) / D) ], D = sqrt(s) + eps: the subtraction; product and
    quotient (2) and the two roundings of gi (2) on the update; sqrt, + eps (2) and the nine of s through d sqrt = ds / (2 sqrt s)
    on the divisor."""
    lr, alpha, eps, wd, gs = (_f32(v) for v in (lr, alpha, eps, weight_decay, grad_scale))
    p, g, sq = (np.asarray(v, dtype=np.float64) for v in (p, g, sq))
    blocked, skip, flag = _guard(g, gs, flag)
    if blocked:
        return {'p': p.copy(), 'sq': sq.copy(), 'flag': flag, 'skip': np.ones(p.shape, dtype=bool),
                'bound_p': np.zeros_like(p), 'bound_sq': np.zeros_like(p)}
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        gi = g * gs + wd * p
        G = np.abs(g * gs) + np.abs(wd * p)
        s = alpha * sq + (1.0 - alpha) * gi * gi
        S = alpha * sq + (1.0 - alpha) * G * G
        D = np.sqrt(s) + eps
        pn = p - lr * gi / D
        ratio = np.where(s > 0, S / np.where(s > 0, s, 1.0), 1.0)
        bound_p = gamma(1) * (np.abs(p) + lr * G / D * (7.0 + 4.5 * ratio * np.sqrt(s) / D))
        bound_sq = gamma(9) * S
    if skip is not None:
        pn, s = np.where(skip, p, pn), np.where(skip, sq, s)
        bound_p, bound_sq = np.where(skip, 0.0, bound_p), np.where(skip, 0.0, bound_sq)
    return {'p': pn, 'sq': s, 'flag': flag, 'skip': skip, 'bound_p': bound_p, 'bound_sq': bound_sq}


def sgd_step(p, g, buf, lr, momentum=0.9, weight_decay=0.0, grad_scale=1.0, first_step=False, flag=None):
    """dsnt_sgd_step (flag None) / _guarded: torch.optim.SGD (dampening 0, no Nesterov) on fp32 inputs in fp64.

        gi = g * grad_scale (+ weight_decay * p);  momentum != 0: buf = gi (first step) or momentum * buf + gi, gi = buf;
        p -= lr * gi                               momentum == 0: `buf` is never read or written (may be None)

    Returns a dict: p, buf, flag, skip and bound_buf = gamma(4) * B, B = |g grad_scale| + |weight_decay p| + |momentum buf|
    (scale, fma, product, sum), bound_p = gamma(6) * (|p| + lr B) (those four, the product with lr, the subtraction)."""
    lr, mom, wd, gs = (_f32(v) for v in (lr, momentum, weight_decay, grad_scale))
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    buf = None if buf is None else np.asarray(buf, dtype=np.float64)
    blocked, skip, flag = _guard(g, gs, flag)
    if blocked:
        return {'p': p.copy(), 'buf': None if buf is None else buf.copy(), 'flag': flag, 'skip': np.ones(p.shape, dtype=bool),
                'bound_p': np.zeros_like(p), 'bound_buf': np.zeros_like(p)}
    with np.errstate(over='ignore', invalid='ignore'):
        gi = g * gs + wd * p
        B = np.abs(g * gs) + np.abs(wd * p)
        bn = buf
        if mom != 0.0:
            if first_step:
                bn = gi
            else:
                bn = mom * buf + gi
                B = B + np.abs(mom * buf)
            gi = bn
        pn = p - lr * gi
        bound_p, bound_buf = gamma(6) * (np.abs(p) + lr * B), gamma(4) * B
    if skip is not None:
        pn = np.where(skip, p, pn)
        if mom != 0.0:
            bn = np.where(skip, buf, bn)
        bound_p, bound_buf = np.where(skip, 0.0, bound_p), np.where(skip, 0.0, bound_buf)
    return {'p': pn, 'buf': bn, 'flag': flag, 'skip': skip, 'bound_p': bound_p, 'bound_buf': bound_buf}


def nonfinite_flag(x, flag, code):
    """dsnt_nonfinite_flag: flag[0] |= code when `x` holds an inf or a NaN; a gradient flag an optimiser left in flag[1] is
    promoted into flag[0] (it blocks every update from here on); flag[1] itself stays."""
    f0, f1 = int(flag[0]), int(flag[1])
    if not np.isfinite(np.asarray(x)).all():
        f0 |= code
    if f1 != 0:
        f0 |= f1
    return [f0, f1]


# ---------------------------------------------------------------- the inputs both test modules use
def tie_input(N, H, W, C, seed, pool, nan_tap=None):
    """A tie-heavy NHWC fp32 tensor: relu(round(4 x) / 4), x ~ N(0, 0.25^2) — two thirds exact (+)zeros, the rest on four
    or five levels of a quarter grid (with N(0, 1) only 18 % of the 2x2 windows would hold a tie) —, with the edge windows planted in channels 0..4 (C >= 8) of the first window of image 0 and of one more
    window of the last image (`pool`: 2 or 3 — which pool's window geometry):
      channel 0: all taps equal (0.5)                 channel 1: zeros, the only maximum (2.0) at the LAST tap
      channel 2: -0.0 and +0.0 alternating, -0.0 first  channel 3: all taps -inf
      channel 4: one NaN in the whole tensor, at valid tap `nan_tap` (mod the window's taps) of the last planted window."""
    assert C >= 8
    r = np.random.default_rng(seed)
    x = (np.maximum(np.round(4.0 * (0.25 * r.standard_normal((N, H, W, C)))) / 4.0, 0.0) + 0.0).astype(np.float32)
    regions = [(0, 0, min(H, 2), 0, min(W, 2))]
    if H >= 4 and W >= 4:
        regions.append((N - 1, 1, 4, 1, 4) if pool == 3 else (N - 1, H - 2, H, W - 2, W))
    for n, r0, r1, c0, c1 in regions:
        cnt = (r1 - r0) * (c1 - c0)
        x[n, r0:r1, c0:c1, 0] = 0.5
        x[n, r0:r1, c0:c1, 1] = 0.0
        x[n, r1 - 1, c1 - 1, 1] = 2.0
        x[n, r0:r1, c0:c1, 2] = np.where(np.arange(cnt) % 2 == 0, -0.0, 0.0).reshape(r1 - r0, c1 - c0).astype(np.float32)
        x[n, r0:r1, c0:c1, 3] = -np.inf
    if nan_tap is not None:
        n, r0, r1, c0, c1 = regions[-1]
        t = nan_tap % ((r1 - r0) * (c1 - c0))
        x[n, r0 + t // (c1 - c0), c0 + t % (c1 - c0), 4] = np.nan
    return x


def int_grad(shape, seed):
    """Small integers (-3..3) as fp32: sums of them are exact in fp32 and fp64 alike."""
    return np.random.default_rng(seed).integers(-3, 4, shape).astype(np.float32)


def bn_case(M, C, seed):
    """x [M][C], gamma, beta, da in the range of the existing BatchNorm tests (|mean| < std: the one-pass variance is not
    what these tests are about), all fp32."""
    r = np.random.default_rng(seed)
    x = (r.standard_normal((M, C)) * 1.7 + 0.4).astype(np.float32)
    gamma = (r.uniform(-1, 1, C) + 1.5).astype(np.float32)
    beta = (r.standard_normal(C) * 0.2).astype(np.float32)
    da = r.standard_normal((M, C)).astype(np.float32)
    return x, gamma, beta, da


def bn_vectors(x, gamma, beta, eps=1e-5):
    """(mean, invstd, scale, shift) as fp32 vectors from the fp64 batch statistics of `x` [M][C] (biased variance): what
    dsnt_bn_finalize leaves — the apply and reduce kernels take them as given inputs."""
    x = np.asarray(x, dtype=np.float64)
    mu, var = x.mean(0), x.var(0)
    is_ = (1.0 / np.sqrt(var + eps)).astype(np.float32)
    mu = mu.astype(np.float32)
    sc = (gamma * is_).astype(np.float32)
    sh = (beta - mu * sc).astype(np.float32)
    return mu, is_, sc, sh


# ---------------------------------------------------------------- BatchNorm: the finalise step (partial[tiles][2][C] -> vectors)
U64 = 2.0 ** -53
BN_FROZEN = 2              # include/dsnt_hip.h: DSNT_BN_FROZEN


def gamma64(k):
    return k * U64 / (1.0 - k * U64)


def half_ulp32(v):
    """Half an fp32 unit in the last place of the binade `v` lies in (subnormal spacing, 2^-149, below 2^-126 and at 0)."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    e = np.where(v == 0, -125, np.frexp(v)[1])                  # frexp(0) says exponent 0: zero belongs to the subnormal binade
    return 0.5 * np.ldexp(1.0, np.maximum(e - 24, -149))


def exact_tile_sums(partial):
    """(S0, S1, A0, A1) per channel from partial[tiles][2][C]: the tile sums added EXACTLY (math.fsum: the correctly rounded
    fp64 value of the real sum, whatever the order) and the sums of their absolute values."""
    p = np.asarray(partial, dtype=np.float64)
    assert p.ndim == 3 and p.shape[1] == 2
    S = np.array([[math.fsum(p[:, k, c].tolist()) for c in range(p.shape[2])] for k in range(2)])
    A = np.array([[math.fsum(np.abs(p[:, k, c]).tolist()) for c in range(p.shape[2])] for k in range(2)])
    return S[0], S[1], A[0], A[1]


def combine_f32(partial):
    """What a left-to-right fp32 combine of the tile sums gives (the mistake the `cancelling` partials exist to show):
    (S0, S1) as fp64 views of fp32 accumulators."""
    p = np.asarray(partial, dtype=np.float32)
    acc = np.zeros((2, p.shape[2]), dtype=np.float32)
    for t in range(p.shape[0]):
        acc = acc + p[t]                      # fp32 + fp32, rounded once per addition
    return acc[0].astype(np.float64), acc[1].astype(np.float64)


def _is(var, eps):
    return 1.0 / np.sqrt(var + eps)


def bn_finalize(partial, M, gamma, beta, running_mean, running_var, momentum, eps, training, sum_err=None, sums=None):
    """dsnt_bn_finalize / bn_pro_forward in fp64 from the exact tile sums.  `momentum`, `eps`: taken as the fp32 values the
    ABI receives.  gamma / beta / running_* may be None (the ABI's NULL).  training = 0: the statistics are the running
    pair, `partial` is not read.  Returns a dict of fp64 vectors; every `bar_*` bounds |device fp32 value - reference|.

    With u = 2^-53, T tiles, A_k = sum |partial_k|:
      e_k  = gamma64(T) A_k            the kernels' fp64 combine, any order (`sum_err` = (e0, e1) replaces it: the error the
                                       tile sums themselves carry, for an end-to-end bar)
      dm   = e0 / M + 2u |mean|        mean = S0 * fl(1 / M): two roundings
      dv   = e1 / M + 2 |mean| dm + dm^2 + 4u (|S1| / M + mean^2)      var = S1 invM - mean^2, clamped at 0 as the kernels do
      invstd = fl32(1 / sqrt(var + eps)): half an fp32 ulp + max |is(var +- dv) - is(var)|, lower end clamped at 0 (is() is
               monotone: the interval's image, no first-order expansion)
      mean:  half an fp32 ulp + dm
      running_mean / running_var = (1 - m) old + m new (unbias): half an fp32 ulp + m dm / m unbias dv
    scale and shift are one and two fp32 operations on the device's OWN mean and invstd: scale_bits() / shift_ok().
    `sums`: (exact_tile_sums(partial), tiles) computed before, for several calls on the same partials."""
    m, eps = _f32(momentum), _f32(eps)
    out = {}
    if training:
        (S0, S1, A0, A1), T = sums if sums is not None else (exact_tile_sums(partial), np.asarray(partial).shape[0])
        e0, e1 = (gamma64(T) * A0, gamma64(T) * A1) if sum_err is None else sum_err
        mean = S0 / M
        raw = S1 / M - mean * mean
        var = np.maximum(raw, 0.0)
        dm = e0 / M + 2 * U64 * np.abs(mean)
        dv = e1 / M + 2 * np.abs(mean) * dm + dm * dm + 4 * U64 * (np.abs(S1) / M + mean * mean)
        out.update(S0=S0, S1=S1, A0=A0, A1=A1, var_raw=raw)
    else:
        mean = np.asarray(running_mean, dtype=np.float64)
        var = np.asarray(running_var, dtype=np.float64)
        dm, dv = np.zeros_like(mean), np.zeros_like(var)
    is_ = _is(var, eps)
    with np.errstate(divide='ignore'):
        spread = np.maximum(np.abs(_is(var + dv, eps) - is_), np.abs(_is(np.maximum(var - dv, 0.0), eps) - is_))
    out.update(mean=mean, var=var, invstd=is_, dm=dm, dv=dv, bar_mean=half_ulp32(mean) + dm, bar_invstd=half_ulp32(is_) + spread,
               bar_invstd_spread=spread)
    if training and running_mean is not None:
        unbias = M / (M - 1.0) if M > 1 else 1.0
        rm = (1.0 - m) * np.asarray(running_mean, dtype=np.float64) + m * mean
        rv = (1.0 - m) * np.asarray(running_var, dtype=np.float64) + m * var * unbias
        out.update(running_mean=rm, running_var=rv, bar_running_mean=half_ulp32(rm) + m * dm,
                   bar_running_var=half_ulp32(rv) + m * unbias * dv)
    return out


def scale_bits(gamma, invstd_got):
    """scale = fl32(gamma * invstd) on the device's own invstd — one fp32 multiply, nothing to contract; invstd itself
    when gamma is NULL.  Compare as bits."""
    is_ = np.asarray(invstd_got, dtype=np.float32)
    return is_.copy() if gamma is None else np.asarray(gamma, dtype=np.float32) * is_


def shift_ok(beta, mean_got, scale_got, shift_got):
    """shift = beta - mean * scale on the device's own fp32 mean and scale: the compiler may contract, so either
    fl32(beta - fl32(mean scale)) or the fused fl32(beta - mean scale).  The fused value is decided exactly (rationals:
    the product of two fp32 numbers needs 48 bits, the difference more than fp64 may hold).  Returns a bool per channel;
    zeros compare equal whatever their sign."""
    mu, sc, got = (np.asarray(v, dtype=np.float32) for v in (mean_got, scale_got, shift_got))
    b = np.zeros_like(mu) if beta is None else np.asarray(beta, dtype=np.float32)
    ok = got == b - mu * sc                                    # numpy fp32: two roundings
    for c in np.flatnonzero(~ok):
        g = got[c]
        if not np.isfinite(g):
            continue
        E = Fraction(float(b[c])) - Fraction(float(mu[c])) * Fraction(float(sc[c]))
        d = abs(E - Fraction(float(g)))
        lo, hi = (abs(E - Fraction(float(np.nextafter(g, np.float32(s))))) for s in (-np.inf, np.inf))
        even = (int(np.asarray(g).view(np.uint32)) & 1) == 0
        ok[c] = d <= lo and d <= hi and (even or (d < lo and d < hi))
    return ok


def bn_bwd_finalize(partial, M, flags, dgamma0, dbeta0, scale=None, dz_amax=None, sums=None):
    """dsnt_bn_bwd_finalize(_bound) / bn_pro_backward in fp64 from the exact tile sums (S0 = sum dz, S1 = sum dz xhat).
    `flags`: bit 0 = add to dgamma0 / dbeta0 (the fp32 vectors the launch finds; None = the ABI's NULL: nothing written),
    BN_FROZEN = both coefficient rows are zero, dgamma / dbeta as without it.  Bars (e_k as in bn_finalize):
      coef[k] = fl32(S_k fl(1 / M)):  half an fp32 ulp + e_k / M + 2u |S_k / M|        (frozen: exactly zero)
      dgamma = fl32(S1), dbeta = fl32(S0):  half an ulp + e_k; accumulated: one more fp32 addition — half an ulp of the sum.
    With `scale` and `dz_amax` (64 slots) the dict holds `bound(coef_got)`: per slot s the fp64 value of
      max over 16-channel blocks vb = s (mod 64), channels c of the block:  |scale_c| (max dz_amax + |coef0_c| + |coef1_c| sqrtf(M))
    on the device's own coef [2][C] (0 for a slot no block maps to), and `bar_bound_rel` = gamma(5): four fp32 operations
    (product, two sums, product; the rounded sqrtf(M) is an input), one spare.  `sums`: as in bn_finalize."""
    (S0, S1, A0, A1), T = sums if sums is not None else (exact_tile_sums(partial), np.asarray(partial).shape[0])
    e0, e1 = gamma64(T) * A0, gamma64(T) * A1
    frozen, acc = bool(flags & BN_FROZEN), bool(flags & 1)
    c0, c1 = (np.zeros_like(S0), np.zeros_like(S1)) if frozen else (S0 / M, S1 / M)
    out = {'S0': S0, 'S1': S1, 'coef': np.stack([c0, c1]),
           'bar_coef': np.zeros((2, S0.size)) if frozen else np.stack([half_ulp32(c0) + e0 / M + 2 * U64 * np.abs(c0),
                                                                        half_ulp32(c1) + e1 / M + 2 * U64 * np.abs(c1)])}
    for name, S, e, old in (('dgamma', S1, e1, dgamma0), ('dbeta', S0, e0, dbeta0)):
        if old is None:
            out[name] = None
            continue
        bar = half_ulp32(S) + e
        want = S
        if acc:
            want = S + np.asarray(old, dtype=np.float64)
            bar = bar + half_ulp32(want)
        out[name], out['bar_' + name] = want, bar
    if scale is not None:
        sc, dzmax = np.abs(np.asarray(scale, dtype=np.float64)), float(np.max(np.asarray(dz_amax, dtype=np.float64)))
        sqrtM = float(np.sqrt(np.float32(M)))              # sqrtf((float)M): correctly rounded on both sides
        C = S0.size

        def bound(coef_got):
            cg = np.abs(np.asarray(coef_got, dtype=np.float64)).reshape(2, C)
            per = sc * (dzmax + cg[0] + cg[1] * sqrtM)
            slots = np.zeros(64)
            for vb in range((C + 15) // 16):
                slots[vb & 63] = max(slots[vb & 63], per[vb * 16:vb * 16 + 16].max())
            return slots
        out['bound'], out['bar_bound_rel'] = bound, gamma(5)
    return out


def pro_mapping(C, NT):
    """bn_pro_sums<NT>'s index arithmetic (csrc/bn_pro.h): the 2C-wide row of partial[tiles][2][C] goes through the workgroup
    in chunks of NT columns; per chunk (nc columns, L = NT // nc tile lanes, idle = NT - nc L threads without a lane).
    Returns the list of (nc, L, idle), one per chunk."""
    ncol, out = 2 * C, []
    for cb in range(0, ncol, NT):
        nc = min(ncol - cb, NT)
        L = NT // nc
        out.append((nc, L, NT - nc * L))
    return out


def pro_reads(tiles, C, NT):
    """How often bn_pro_sums<NT> reads each element of partial[tiles][2C] — must be once, nothing beyond `tiles` —, and per
    chunk the largest number of trips of its 16-deep load batch any lane takes.  Mirrors the kernel's loops thread by thread."""
    ncol = 2 * C
    cnt = np.zeros((tiles, ncol), dtype=np.int64)
    trips = []
    for cb in range(0, ncol, NT):
        nc = min(ncol - cb, NT)
        L = NT // nc
        most = 0
        for tid in range(NT):
            col, lane = tid % nc, tid // nc
            if lane >= L:
                continue
            n = 0
            for r0 in range(lane, tiles, 16 * L):
                n += 1
                for u in range(16):
                    r = r0 + u * L
                    if r < tiles:
                        cnt[r, cb + col] += 1
            most = max(most, n)
        trips.append(most)
    return cnt, trips


# ---------------------------------------------------------------- BatchNorm: hand-made tile sums for the finalise tests
def partial_producer(T, C, seed, rows=TILE_ROWS, offset=0.0):
    """Tile sums as a producer leaves them: fl32 of tile_sums() of a bn_case x (+ `offset`), `rows` rows per tile, the last
    tile ragged.  Returns (partial [T][2][C] fp32, M, x)."""
    M = T * rows - (rows // 3 if T > 1 or rows > 1 else 0)
    x = bn_case(M, C, seed)[0]
    if offset:
        x = (x / np.float32(1.7) + np.float32(offset)).astype(np.float32)       # spread ~1 around `offset`
    s1, s2, _, _ = tile_sums(x, M, C, rows)
    return np.stack([s1, s2], 1).astype(np.float32), M, x


def partial_cancelling(T, C, seed, M=None):
    """Integer-valued tile sums that tell an fp64 combine from an fp32 one: both rows alternate +2^26, a small odd integer,
    -2^26, a small odd integer, ..., as many +2^26 as -2^26.  Every partial sum of any subset is an integer below 2^53: exact
    in fp64 in ANY order.  In fp32 a small term vanishes beside 2^26 (ulp 8): row 0 holds 1 or 3, so a left-to-right fp32
    combine loses EVERY small term up to the last -2^26 (all errors of one sign: they cannot cancel); row 1 holds odd
    values below 256, so that var > 0.  T >= 4.
    Returns (partial, M), M = 128 T - 37 unless given (the finalise step only divides by it)."""
    assert T >= 4
    r = np.random.default_rng(seed)
    p = np.empty((T, 2, C), dtype=np.float64)
    p[:, 0] = 2 * r.integers(0, 2, (T, C)) + 1
    p[:, 1] = 2 * r.integers(0, 128, (T, C)) + 1
    big = np.arange(0, T, 2)
    big = big[:len(big) // 2 * 2]                                 # even tiles, an even number of them
    for i, t in enumerate(big):
        p[t, :, :] = (1.0 if i % 2 == 0 else -1.0) * 2.0 ** 26
    return p.astype(np.float32), (128 * T - 37 if M is None else M)


def partial_constant(T, C, values, rows=TILE_ROWS):
    """Tile sums of channels with x = v everywhere (channel c: values[c % len(values)]), full tiles of `rows` (a power of two)
    rows: rows v and rows v^2, exact in fp32 for v of at most 12 significant bits.  Returns (partial, M, v per channel)."""
    v = np.array([values[c % len(values)] for c in range(C)], dtype=np.float64)
    p = np.empty((T, 2, C), dtype=np.float64)
    p[:, 0], p[:, 1] = rows * v, rows * v * v
    return p.astype(np.float32), T * rows, v
