"""Operands, bounds and per-channel bars for the fp16x3 range tests (tests/test_f16x3_range_gpu.py).

An fp16x3 operand x is scaled by s = pow2_scale(bound) (csrc/conv_split.h: bound * s in [2^13, 2^14)) and stored as two fp16
planes h1 = fp16(x s), h2 = fp16(x s - h1).  Once |x s| < 2^-14 the low plane is an fp16 subnormal: x keeps only the absolute
precision 2^-25 / s <= bound 2^-38.  The profiles below put realistic small quantities into the operands (small channels, small
weight rows, small and zero images of a gradient) at a bound that is `LOOSE` times too large, and a probe whose exact result
depends on every subnormal plane element surviving.
"""
import math

import numpy as np
import torch

# The largest operand-bound looseness (bound / max|operand|) the range tests hold the kernels to, per kind of bound, as log2.
# Measured on full-size train steps (tests/test_bounds_gpu.py, which asserts that no launch is looser):
#   'a'  A operands: the train-mode BatchNorm+ReLU bound max_c |gamma_c| sqrt(M) + |beta_c| is the loose one, 2^7.1 at
#        hg2 batch 32 (sqrt(M) = 724 at 128 x 128) — held to 2^8;
#   'w'  weights: the prep launch's exact maximum — 2^0;
#   'g'  gradient operands (producer amax slots) and 'gf' the folded BatchNorm backward (dsnt_bn_bwd_finalize_bound):
#        2^0.9 at most — held to 2^2.
# These cover the configurations test_bounds_gpu walks (hg2 / hg1 batch 32, hg8 batch 16).  Not covered: the BatchNorm bound grows
# as sqrt(M), so batch 256 extrapolates to 2^8.6; the folded backward's |mean(dz xhat)| sqrt(M) term can reach sqrt(M) on real
# gradients correlated with xhat (the synthetic step's are not).  A gradient bound 2^8 too large is NOT harmless: a gradient
# channel 2^-14 below the largest one then keeps about 14 significant bits in the weight gradient (about 10x the per-channel bar).
# Both want a tighter bound (a recorded max|xhat| in place of sqrt(M)), not a looser test.
LOOSE_LOG2 = {'a': 8, 'w': 0, 'g': 2, 'gf': 2}
LOOSE_A = 2.0 ** LOOSE_LOG2['a']
LOOSE_G = 2.0 ** LOOSE_LOG2['g']

PROFILES = ('chan', 'wspread', 'grad', 'probe')


def pow2_scale(bound):
    """csrc/conv_split.h pow2_scale for a positive normal float."""
    return 2.0 ** (13 - math.floor(math.log2(bound)))


def rng(tag):
    import zlib
    return np.random.Generator(np.random.PCG64([7, zlib.crc32(tag.encode())]))


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def log_spread(r, n, lo):
    """n factors log-uniform over [2^lo, 1]."""
    return 2.0 ** r.uniform(lo, 0.0, n)


def heavy(r, shape, axis_n=0, lo=-12):
    """A concentrated gradient: n^3 (heavy-tailed), every image (leading axis) scaled by 2^U(lo, 0), image 1 entirely zero
    (a fully masked sample) when there are at least two."""
    v = r.standard_normal(shape) ** 3
    sc = log_spread(r, shape[axis_n], lo)
    if shape[axis_n] > 1:
        sc[1] = 0.0
    v *= sc.reshape((-1,) + (1,) * (len(shape) - 1))
    return v


# ------------------------------------------------------------------------------------------------------- the subnormal probe
# The probe fixes s = 2^13 by one element equal to its bound 1.5 (1.5 * 2^13 = 12288, an fp16).  Every other element is one of
#   * 'res': x s = h1 + h2, h1 an fp16 of magnitude in [2^-13, 1) (or an fp16 subnormal), h2 = j 2^-24 an fp16 SUBNORMAL with
#     |h2| < ulp(h1) / 2 — so fp16(x s) = h1 and x s - h1 = h2 exactly; x s has at most 24 significant bits (an fp32);
#   * 'pow2': x s = +-2^k, k in [-24, 12] (one fp16 plane, subnormal for k < -14).
# Every output element of a probe launch is ONE product res * pow2 (the other operand of each product is a power of two), so
# the fp64 result is exact and representable in fp32, and the split carries it exactly.  What remains is the MFMA: on MI355X a bare
# v_mfma_f32_32x32x16_f16 returns every single product of these operand pairs exactly, but the three-instruction chain of
# csrc/conv_split.h mma_split (a2 b1, then a1 b2, then a1 b1, each accumulating onto the last) rounds the small accumulator input
# when it is added to the large product: 32768 probe pairs on one wave gave 2130 inexact sums, worst 2^-14.1 of the result, e.g.
# a1 b1 = -0x1.c3cp-24 plus C = 0x1.d38p-37 returned -0x1.c3b2p-24 (exact: -0x1.c3b164p-24).  Every kernel's probe worst is
# the same 2^-14.0 to 2^-14.8, so the kernels add nothing to it.  The bar is PROBE_REL = 2^-13 per element: twice the
# instruction's own worst.  A flushed subnormal h1 removes its element; a flushed h2 changes it by up to 2^-11 of it (hand check:
# flushing h2 at one fwd1 split site fails the fwd1 probe in 226768 of 2097152 elements, and all three statistical fwd1 profiles).
PROBE_BOUND = 1.5
PROBE_S = pow2_scale(PROBE_BOUND)


def probe_res(r, n):
    e = r.integers(-13, 0, n)                         # exponent of h1: [2^e, 2^(e+1))
    m = r.integers(1025, 2048, n)                     # significand 1.x (never exactly 2^e: no rounding across a binade)
    h1 = m * 2.0 ** (e - 10)
    jmax = np.minimum(1023, 2.0 ** (e + 13) - 1)      # |h2| < ulp(h1) / 2 = 2^(e-11), and |h2| < 2^-14 (subnormal)
    j = np.floor(r.uniform(-1, 1, n) * (jmax + 1)).clip(-jmax, jmax)
    h2 = j * 2.0 ** -24
    sub = r.random(n) < 0.15                          # some elements are a bare fp16 subnormal
    h1 = np.where(sub, r.integers(1, 1024, n) * 2.0 ** -24, h1)
    h2 = np.where(sub, 0.0, h2)
    sign = np.where(r.random(n) < 0.5, -1.0, 1.0)
    return sign * (h1 + h2) / PROBE_S


def probe_pow2(r, n):
    sign = np.where(r.random(n) < 0.5, -1.0, 1.0)
    return sign * 2.0 ** r.integers(-24, 13, n).astype(np.float64) / PROBE_S


def assert_probe_exact(r_vals):
    """Self-check of the construction: every value is an fp32 whose scaled split is exact with a subnormal (or zero) h2."""
    v = np.asarray(r_vals, dtype=np.float64).ravel()
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    xs = (v * PROBE_S).astype(np.float32)
    h1 = xs.astype(np.float16).astype(np.float32)
    h2 = (xs - h1).astype(np.float16)
    assert np.array_equal(h1.astype(np.float64) + h2.astype(np.float64), xs.astype(np.float64))
    assert (np.abs(h2.astype(np.float64)) < 2.0 ** -14).all()


# --------------------------------------------------------------------------------------------------------------- bounds
def dev_amax(t, loose=1.0):
    """The 64-slot bound of a materialised operand as its producer leaves it (dsnt_amax), times `loose` (a power of two)."""
    from dsnt._lib import ptr, call
    b = torch.zeros(64, device=t.device)
    call('dsnt_amax', ptr(t), t.numel(), ptr(b))
    return b * loose


def bn_bound(gamma, beta, M, dev):
    """The engine's train-mode BatchNorm+ReLU bound, max_c |gamma_c| sqrt(M) + |beta_c| (dsnt_f16_prep_bn_bounds)."""
    import struct
    from dsnt._lib import ptr, call
    g, b = gamma.to(dev).contiguous(), beta.to(dev).contiguous()
    out = torch.zeros(64, device=dev)
    bits = struct.unpack('<I', struct.pack('<f', float(M) ** 0.5))[0]
    t = torch.tensor([[g.data_ptr(), b.data_ptr(), out.data_ptr(), g.numel(), bits]], dtype=torch.int64).to(dev)
    call('dsnt_f16_prep_bn_bounds', ptr(t), 1)
    torch.cuda.synchronize()
    return out


def prep_weights(w, stream_order=False):
    """fp16 planes and the bound of a weight tensor [Cout][R][S][Cin] from the per-step prep launch (dsnt_f16_prep_weights)."""
    from dsnt._lib import ptr, call
    n = w.numel()
    planes = torch.empty(2 * n, dtype=torch.float16, device=w.device)
    wb = torch.zeros(64, device=w.device)
    co, ci = (w.shape[0], w.shape[-1]) if stream_order else (0, 0)
    t = torch.tensor([[w.data_ptr(), planes.data_ptr(), wb.data_ptr(), n, n, co, ci]], dtype=torch.int64).to(w.device)
    call('dsnt_f16_prep_weights', ptr(t), 1, 7)
    torch.cuda.synchronize()
    return planes, wb


def bmax(*bounds):
    """The larger of several 64-slot bounds (every slot holds the maximum of the slots)."""
    m = max(float(b.max()) for b in bounds)
    return torch.full((64,), m, device=bounds[0].device)


# ------------------------------------------------------------------------------------------------------------------ bars
REPORT = {}


def per_channel(name, got, ref64, ref32, axis):
    """err_c <= max(4 err32_c, 2e-6 scale_c) for every channel c along `axis` (forward / data gradient: output channel over the
    batch; weight gradient: output-channel row).  Records the worst err_c / err32_c (over channels where fp32 has an error),
    the worst err_c / bar_c and the channels where fp32 is exact but the kernel is not; returns the failures."""
    dims = [d for d in range(got.dim()) if d != axis % got.dim()]
    got, ref64, ref32 = got.double().cpu(), ref64.double().cpu(), ref32.double().cpu()
    err = (got - ref64).abs().amax(dim=dims)
    err32 = (ref32 - ref64).abs().amax(dim=dims)
    scale = ref64.abs().amax(dim=dims)
    bar = torch.maximum(4 * err32, 2e-6 * scale)
    rec = REPORT.setdefault(name, {'err/err32': 0.0, 'err/bar': 0.0, 'fp32 exact, kernel not': 0})
    pos = err32 > 0
    if bool(pos.any()):
        rec['err/err32'] = max(rec['err/err32'], float((err[pos] / err32[pos]).max()))
    live = bar > 0
    if bool(live.any()):
        rec['err/bar'] = max(rec['err/bar'], float((err[live] / bar[live]).max()))
    rec['fp32 exact, kernel not'] += int(((err32 == 0) & (err > 0)).sum())
    bad = ~(err <= bar)                  # NaN is a failure; so is any error in a channel whose bar is zero
    return [(name, int(c), float(err[c]), float(err32[c]), float(scale[c])) for c in torch.nonzero(bad).flatten()[:6].tolist()]


def report_line(rec):
    return '  '.join('%s %.3g' % (k, v) if isinstance(v, float) else '%s %d' % (k, v) for k, v in rec.items())


PROBE_REL = 2.0 ** -13


def exact(name, got, ref64):
    """The probe: every element within PROBE_REL of the (exact, fp32-representable) fp64 result; zeros exactly zero."""
    got, ref64 = got.double().cpu(), ref64.double().cpu()
    assert torch.equal(ref64.float().double(), ref64), name + ': probe reference not exact in fp32'
    rel = (got - ref64).abs() / ref64.abs()
    rel = torch.where(ref64 == 0, torch.where(got == 0, 0.0, float('inf')), rel)
    worst = float(rel.max())
    rec = REPORT.setdefault(name + '/probe', {'worst rel': 0.0})
    rec['worst rel'] = max(rec['worst rel'], worst)
    diff = ~(rel <= PROBE_REL)
    if bool(diff.any()):
        i = torch.nonzero(diff)[0].tolist()
        return [(name, 'mismatches', int(diff.sum()), 'of', got.numel(), 'worst rel', worst, 'first', i, float(got[tuple(i)]),
                 float(ref64[tuple(i)]))]
    return []
