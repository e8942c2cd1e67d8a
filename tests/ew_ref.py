"""The element-wise kernels of csrc/bn.hip, resample.hip, flat.hip, optim.hip and csrc/ew_bodies.h restated in numpy fp64, for
tests/test_ew_ref_cpu.py (which pins this file to the torch CPU operators) and tests/test_elementwise_edges_gpu.py
(which holds the HIP kernels to it).  No device code: everything here takes and returns numpy arrays on the host.

Layouts are the kernels': NHWC activations, [M][C] rows for the BatchNorm pieces, flat vectors for the optimisers.
Inputs are the kernels' fp32 inputs taken to fp64; where a kernel's result is a selection (pool maximum, ReLU mask,
skipped element) the selection rule is spelled out, where it is arithmetic the fp64 value comes with the a-priori
fp32 rounding bound of the kernel's expression (`U` = 2^-24, `gamma(k)` = k U / (1 - k U): k rounded operations)."""
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
def _by_tile(t, M, C):
    tiles = (M + TILE_ROWS - 1) // TILE_ROWS
    pad = np.zeros((tiles * TILE_ROWS, C), dtype=np.float64)
    pad[:M] = t
    return pad.reshape(tiles, TILE_ROWS, C)


def tile_sums_of(t1, t2, M, C):
    """Per 128-row tile and channel, in fp64: (sum t1, sum t2, sum |t1|, sum |t2|), each [tiles][C]."""
    a, b = _by_tile(t1, M, C), _by_tile(t2, M, C)
    return a.sum(1), b.sum(1), np.abs(a).sum(1), np.abs(b).sum(1)


def tile_sums(x, M, C):
    """dsnt_bn_stats: (sum x, sum x^2, sum |x|, sum x^2) per tile and channel from the fp32 `x` [M][C]."""
    x = np.asarray(x, dtype=np.float64).reshape(M, C)
    return tile_sums_of(x, x * x, M, C)


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
