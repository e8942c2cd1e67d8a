"""Trained-regime inputs, oracle runners and the yardstick for the DSNT head tests (no GPU, no fixture).

Used by tests/test_head_regimes_cpu.py (fp32 oracle against fp64 oracle) and tests/test_head_regimes_gpu.py (HIP against
the fp64 oracle).  Three parts:

* `make(regime, h, w, rows)`: deterministic `(logits [rows,1,h,w], target [rows,1,2], mask [rows,1])` per regime.
* `oracle(...)`: `dsnt_oracle` on the CPU in fp64 or fp32, returning coords, dist, reg_row, loss, dL/dlogits, p and
  v = dL/dp per row.
* `scale_rows` / `ratio_rows`: the conditioning scale S_r and the error ratio of a logit gradient (below), and
  `census`: which of the three JS branches of `head_loss_grad_kernel` each 256-pixel granule of a row takes.

The yardstick.  The gradient of a row with respect to its logits is g_i = p_i (v_i - sum_j p_j v_j), a difference of two
nearly equal terms on peaked rows.  Relative to the row's own largest |g_i| the fp32 oracle itself misses the fp64 oracle
by more than 1 on edge-peaked and one-hot rows, so no fp32 kernel can hold a bound of that kind.  The error is measured
instead against the size of the two terms that cancel,

    S_r = max_i |p_i v_i| + (max_i p_i) |sum_j p_j v_j|,        ratio_r = max_i |g_i - g64_i| / (2^-24 S_r),

with p and v from the fp64 oracle.  A row whose S_r is 0 (mask 0) must have an error of exactly 0: its ratio is 0 then and
infinite otherwise, so no row is left out.
"""
import functools
import zlib

import numpy as np
import torch

from dsnt_oracle import nn as onn, model as omodel

REGIMES = ('diffuse', 'peaked', 'edge', 'onehot', 'bimodal', 'offset', 'straddle')
REGS = ('none', 'js', 'kl', 'mse', 'var')
# shape -> why it is in the matrix (the dispatch of dsnt_head_fwd / dsnt_head_loss_grad in csrc/head_fwd.hip, head_loss.hip)
SHAPES = ((64, 64), (64, 48), (28, 28), (16, 16),   # VEC == 4 and w % 4 == 0: the fast JS form
          (14, 14),                                   # hw % 4 == 0, w % 4 != 0: VEC == 4 with the per-slot JS path
          (7, 7), (5, 5),                             # VEC == 1
          (4, 1024), (8, 512),                        # w + h > HEAD_SEP_MAX: tab == false
          (96, 96))                                   # > 4096 pixels: dsnt_head_loss_rows + dsnt_head_bwd
ROWS = 64
EPS24 = 2.0 ** -24


def sigma_of(h, w):
    return 0.3 if max(h, w) <= 7 else 2.0 / w


def coeff_of(reg):
    return 100.0 if reg == 'var' else 1.0


def matrix():
    """Every (regime, h, w, use_mask) of the test matrix; the regulariser kinds are the callers' outer loop."""
    return [(regime, h, w, use_mask) for (h, w) in SHAPES for regime in REGIMES for use_mask in (True, False)]


# ------------------------------------------------------------------ generators
def _bump(h, w, px, py, s):
    """-((c - px)^2 + (r - py)^2) / (2 s^2) per row: a Gaussian peak at pixel (px, py), s pixels wide, as logits."""
    c = np.arange(w, dtype=np.float64)[None, None, :]
    r = np.arange(h, dtype=np.float64)[None, :, None]
    return -((c - px[:, None, None]) ** 2 + (r - py[:, None, None]) ** 2) / (2.0 * s[:, None, None] ** 2)


def _peaked(rng, h, w, rows, s_lo=0.5, s_hi=4.0, noise=0.5):
    px, py = rng.uniform(0, w - 1, rows), rng.uniform(0, h - 1, rows)
    s = np.exp(rng.uniform(np.log(s_lo), np.log(s_hi), rows))
    return _bump(h, w, px, py, s) + noise * rng.standard_normal((rows, h, w))


def _diffuse(rng, h, w, rows):
    return rng.standard_normal((rows, h, w)) * rng.uniform(2, 4, rows)[:, None, None]


def _logits(regime, rng, h, w, rows):
    if regime == 'diffuse':
        return _diffuse(rng, h, w, rows)
    if regime == 'peaked':
        return _peaked(rng, h, w, rows)
    if regime == 'edge':                      # the peak within one pixel of a border (a quarter of the rows: of a corner)
        side = rng.randint(0, 4, rows)
        near = rng.uniform(0, 1, rows)
        px, py = rng.uniform(0, w - 1, rows), rng.uniform(0, h - 1, rows)
        px = np.where(side == 0, near, np.where(side == 1, w - 1 - near, px))
        py = np.where(side == 2, near, np.where(side == 3, h - 1 - near, py))
        corner = rng.uniform(0, 1, rows) < 0.25
        px = np.where(corner & (side >= 2), rng.uniform(0, 1, rows), px)
        py = np.where(corner & (side < 2), h - 1 - rng.uniform(0, 1, rows), py)
        s = rng.uniform(0.5, 2.0, rows)
        return _bump(h, w, px, py, s) + 0.5 * rng.standard_normal((rows, h, w))
    if regime == 'onehot':
        x = rng.standard_normal((rows, h, w))
        x.reshape(rows, -1)[np.arange(rows), rng.randint(0, h * w, rows)] += 200.0
        return x
    if regime == 'bimodal':
        a = _bump(h, w, rng.uniform(0, w - 1, rows), rng.uniform(0, h - 1, rows), rng.uniform(0.5, 3, rows))
        b = _bump(h, w, rng.uniform(0, w - 1, rows), rng.uniform(0, h - 1, rows), rng.uniform(0.5, 3, rows))
        return np.logaddexp(a, b + np.log(rng.uniform(0.2, 1.0, rows))[:, None, None]) \
            + 0.5 * rng.standard_normal((rows, h, w))
    if regime == 'offset':                    # row maxima above +100 (r % 3 == 0), whole rows below -100 (r % 3 == 1)
        x = np.where((np.arange(rows) % 2 == 0)[:, None, None], _peaked(rng, h, w, rows), _diffuse(rng, h, w, rows))
        r3 = np.arange(rows) % 3
        shift = np.where(r3 == 0, rng.uniform(100, 300, rows), np.where(r3 == 1, -rng.uniform(150, 400, rows), 0.0))
        return x + shift[:, None, None]
    if regime == 'straddle':
        # a broad smooth peak: p falls through 1e-16 at 8.6 s pixels from it and the target Gaussian (sigma = 1 pixel of
        # x) through 1e-30 at 11.8 pixels, so both circles cut through 256-pixel granules of the map
        ext = min(max(h, w), 64)
        s = rng.uniform(0.03, 0.125, rows) * ext
        return _bump(h, w, rng.uniform(0, w - 1, rows), rng.uniform(0, h - 1, rows), s) \
            + 0.05 * rng.standard_normal((rows, h, w))
    raise ValueError('unknown regime %r' % regime)


@functools.lru_cache(maxsize=None)
def _make(regime, h, w, rows):
    rng = np.random.RandomState(zlib.crc32(('head_regimes/%s/%d/%d/%d' % (regime, h, w, rows)).encode()))
    x = _logits(regime, rng, h, w, rows).astype(np.float32)
    # target: 0.25 to 2 pixels (pitch of x, 2 / w: the unit sigma is given in) from the centre of the arg-max pixel, on
    # whichever side keeps it away from the predicted coordinates: dist == 0 is NaN, "un-guarded like the reference"
    flat = x.reshape(rows, -1).astype(np.float64)
    am = flat.argmax(-1)
    xs, ys = (2.0 * np.arange(w) - (w - 1)) / w, (2.0 * np.arange(h) - (h - 1)) / h
    peak = np.stack([xs[am % w], ys[am // w]], -1)
    p = np.exp(flat - flat.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    pred = np.stack([(p.reshape(rows, h, w).sum(1) * xs).sum(-1), (p.reshape(rows, h, w).sum(2) * ys).sum(-1)], -1)
    pitch = 2.0 / w
    r, th = rng.uniform(0.25, 2.0, rows) * pitch, rng.uniform(0, 2 * np.pi, rows)
    off = np.stack([r * np.cos(th), r * np.sin(th)], -1)
    t = peak + off
    close = np.sqrt(((pred - t) ** 2).sum(-1)) < 0.2 * pitch
    t = np.where(close[:, None], peak - off, t)
    m = (rng.uniform(-1, 1, rows) > -0.6).astype(np.float32)
    if rows > 1:
        m[0], m[1] = 0.0, 1.0                 # both kinds of row in every mask
    else:
        m[:] = 1.0
    return x.reshape(rows, 1, h, w), t.astype(np.float32).reshape(rows, 1, 2), m.reshape(rows, 1)


def make(regime, h, w, rows=ROWS):
    """(logits [rows,1,h,w], target [rows,1,2], mask [rows,1]) as fp32 CPU tensors; the same call gives the same bits."""
    x, t, m = _make(regime, h, w, rows)
    return torch.from_numpy(x.copy()), torch.from_numpy(t.copy()), torch.from_numpy(m.copy())


# ------------------------------------------------------------------ oracle
def _reg_rows(reg, hm, t, sigma):
    h, w = hm.shape[-2], hm.shape[-1]
    if reg == 'js':
        return onn._js_2d(hm, onn.make_gauss(t, w, h, sigma))
    if reg == 'kl':
        return onn._kl_2d(hm, onn.make_gauss(t, w, h, sigma))
    if reg == 'mse':
        return ((hm - onn.make_gauss(t, w, h, sigma)) ** 2).sum(-1).sum(-1)
    if reg == 'var':
        xs, ys = onn.generate_xy(hm)
        mx = onn.expectation_2d(xs, hm)[..., None, None]
        my = onn.expectation_2d(ys, hm)[..., None, None]
        var = torch.stack([onn.expectation_2d((xs - mx) ** 2, hm), onn.expectation_2d((ys - my) ** 2, hm)], -1)
        return ((var - sigma ** 2) ** 2).sum(-1)
    return torch.zeros(hm.shape[:-2], dtype=hm.dtype)


def oracle(logits, target, mask, reg, sigma, coeff, dtype=torch.float64):
    """`dsnt_oracle` on the CPU in `dtype`: softmax heat-maps, DSNT, Euclidean loss + coeff * regulariser, backward.

    Returns numpy float64 arrays: coords [R,2], dist [R], reg_row [R], loss, g = dL/dlogits [R,hw], p [R,hw] and
    v = dL/dp [R,hw] (the gradient retained on the oracle's heat-map tensor)."""
    lo = logits.detach().clone().to(dtype).requires_grad_()
    hm = omodel.hm_preact(lo, 'softmax')
    hm.retain_grad()
    co = onn.dsnt(hm)
    t = target.to(dtype)
    m = None if mask is None else mask.to(dtype)
    loss = onn.euclidean_loss(co, t, m)
    if reg != 'none':
        # the functions omodel.calculate_reg_loss dispatches to (model.py:47-63), with sigma already in normalised units
        fn = {'js': onn.js_reg_loss, 'kl': onn.kl_reg_loss, 'mse': onn.mse_reg_loss, 'var': onn.variance_reg_loss}[reg]
        loss = loss + coeff * fn(hm, t, sigma, m)
    loss.backward()
    with torch.no_grad():
        dist = (co - t).pow(2).sum(-1).sqrt()
        reg_row = _reg_rows(reg, hm, t, sigma)
    rows = logits.shape[0] * logits.shape[1]
    f = lambda a, *s: a.detach().double().reshape(*s).numpy()
    return dict(coords=f(co, rows, 2), dist=f(dist, rows), reg_row=f(reg_row, rows), loss=float(loss.detach()),
                g=f(lo.grad, rows, -1), p=f(hm, rows, -1), v=f(hm.grad, rows, -1))


# ------------------------------------------------------------------ yardstick
def scale_rows(p, v):
    """S_r = max_i |p_i v_i| + (max_i p_i) |sum_j p_j v_j| from the fp64 oracle's p and v = dL/dp."""
    pv = p * v
    return np.abs(pv).max(-1) + p.max(-1) * np.abs(pv.sum(-1))


def ratio_rows(g, g64, S):
    """max_i |g_i - g64_i| / (2^-24 S_r) per row; a row with S_r == 0 gives 0 for an exact 0 error and inf otherwise.
    A non-finite g gives inf."""
    err = np.abs(np.asarray(g, dtype=np.float64) - g64).max(-1)
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = err / (EPS24 * S)
    return np.where(S > 0, r, np.where(err == 0, 0.0, np.inf))


def value_errors(got, o64):
    """The value bounds of the suite as ratios error / bound (<= 1 passes): coords 2e-6 absolute, dist, reg_row and
    loss 1e-5 max(1, |value|), and, when `got` has heat-maps, 2e-6 absolute and row sums within 1e-5 of 1."""
    out = {'coords': np.abs(got['coords'] - o64['coords']).max() / 2e-6,
           'dist': (np.abs(got['dist'] - o64['dist']) / (1e-5 * np.maximum(1.0, np.abs(o64['dist'])))).max(),
           'loss': abs(got['loss'] - o64['loss']) / (1e-5 * max(1.0, abs(o64['loss'])))}
    if got.get('reg_row') is not None:
        out['reg_row'] = (np.abs(got['reg_row'] - o64['reg_row'])
                          / (1e-5 * np.maximum(1.0, np.abs(o64['reg_row'])))).max()
    if got.get('p') is not None:
        out['hm'] = np.abs(got['p'] - o64['p']).max() / 2e-6
        out['hm_sum'] = np.abs(got['p'].sum(-1) - 1.0).max() / 1e-5
    return {k: (float(x) if np.isfinite(x) else float('inf')) for k, x in out.items()}


# ------------------------------------------------------------------ JS branch census
def census_applies(h, w):
    """The shapes that take the fast JS form of head_loss_grad_kernel: VEC == 4 (hw % 4 == 0, hw <= 4096), w % 4 == 0
    and the separable tables (`tab`: w + h <= HEAD_SEP_MAX = 512)."""
    return (h * w) % 4 == 0 and w % 4 == 0 and h * w <= 4096 and w + h <= 512


def census(p32, target, h, w, sigma):
    """Which JS branch each 256-pixel granule of each row takes in head_loss_grad_kernel (csrc/head_loss.hip, the block
    `if (VEC == 4 && (w & 3) == 0)` under `if (kind == 0 && tab)`).

    Mirrors, in fp32 numpy:
    * `exy[i] = expf(t * t * k)` with t = pos - target, `invz = 1 / (sum ex * sum ey + 1e-24f)`,
      `qy = exy[w + rr] * invz`, `qs[e] = qx[e] * qy`: the target Gaussian as a product of two rounded factors;
    * `i = (kk * HB + threadIdx.x) * 4` with `i < hw`: a wavefront (64 lanes) of chunk kk owns the 256 consecutive
      pixels [256 g, 256 g + 256), g = 4 kk + wave, each lane four of them, lanes beyond hw inactive;
    * `big = pmin > 1e-16f`, `far = qmax < 1e-30f` per lane, then `__all(big && far)` (branch 0: no transcendental),
      `__all(big)` (branch 1: logarithms only), otherwise `elem` (branch 2: the general path).

    p32: the fp32 heat-maps [R, hw]; target [R, 2].  Returns (branch [R, G] int, mixed [R, G] bool): `mixed` marks a
    granule whose active lanes do not all make the same choice (big && far / big only / neither).  The exponentials here
    are numpy's, not the device's, so a lane within an ulp of a threshold may be counted on the other side."""
    assert census_applies(h, w)
    R, hw = p32.shape[0], h * w
    p32 = np.asarray(p32, dtype=np.float32)
    t = np.asarray(target, dtype=np.float32).reshape(R, 2)
    k = np.float32(-0.5 * (1.0 / float(np.float32(sigma))) ** 2)
    xs = ((np.float32(2) * np.arange(w, dtype=np.float32) - np.float32(w - 1)) / np.float32(w)).astype(np.float32)
    ys = ((np.float32(2) * np.arange(h, dtype=np.float32) - np.float32(h - 1)) / np.float32(h)).astype(np.float32)
    with np.errstate(under='ignore'):
        dx, dy = xs[None, :] - t[:, 0:1], ys[None, :] - t[:, 1:2]
        ex, ey = np.exp(dx * dx * k).astype(np.float32), np.exp(dy * dy * k).astype(np.float32)
        invz = (np.float32(1) / (ex.sum(-1, dtype=np.float32) * ey.sum(-1, dtype=np.float32) + np.float32(1e-24)))
        qy = (ey * invz[:, None]).astype(np.float32)
        q = (ex[:, None, :] * qy[:, :, None]).astype(np.float32).reshape(R, hw)
    G = (hw + 255) // 256
    pad = G * 256 - hw
    active = np.ones(hw, bool)
    if pad:
        p32 = np.concatenate([p32, np.ones((R, pad), np.float32)], -1)
        q = np.concatenate([q, np.zeros((R, pad), np.float32)], -1)
        active = np.concatenate([active, np.zeros(pad, bool)])
    act = active.reshape(G, 64, 4)[:, :, 0][None]                       # [1, G, 64]: the lane has i < hw
    big = p32.reshape(R, G, 64, 4).min(-1) > np.float32(1e-16)
    far = q.reshape(R, G, 64, 4).max(-1) < np.float32(1e-30)
    all_bf = ((big & far) | ~act).all(-1)
    all_b = (big | ~act).all(-1)
    branch = np.where(all_bf, 0, np.where(all_b, 1, 2))
    lane = np.where(big & far, 0, np.where(big, 1, 2))
    lo = np.where(act, lane, 3).min(-1)
    hi = np.where(act, lane, -1).max(-1)
    return branch, lo != hi


def census_counts(branch, mixed):
    return {'all_big_far': int((branch == 0).sum()), 'all_big': int((branch == 1).sum()),
            'general': int((branch == 2).sum()), 'mixed': int(mixed.sum())}
