"""Host oracle of the split-plane operand preparation (csrc/conv_prep.hip, the space-to-depth half of csrc/flat.hip,
dsnt_zero_insert of csrc/resample.hip), written from the contract in csrc/conv_split.h's comments and include/dsnt_hip.h, for
tests/test_split_ref_cpu.py (the oracle's own properties) and tests/test_operand_prep_gpu.py (the kernels against it, bit for
bit).  numpy / torch on the CPU only: no device code and no dsnt._lib.

What these kernels compute is exactly defined — IEEE round-to-nearest-even conversions, exact fp32 subtractions, index
permutations — so everything here is compared as BIT PATTERNS, never within a tolerance (the one exception, the BatchNorm bound,
is arithmetic in fp32 and comes with its derived rounding bound).  fp16 planes are returned as numpy float16, bf16 planes as
uint16 (the upper half of the fp32 pattern; `bf16_to_f32` widens them).

Non-finite inputs (characterisation, deliberately narrow).  A NaN among the elements of a tensor does not enter its bound
(`amax` is the maximum over the elements that are not NaN), sits as a NaN in plane 0 at its own index, and leaves every other
element as if it were not there.  A +inf makes the bound +inf and sits as +inf in plane 0 at its own index.  Nothing else is
promised for non-finite inputs (the remaining planes at that index, and — with an infinite bound — the other elements)."""
import numpy as np
import torch

BOUND_SLOTS = 64                      # csrc/conv_split.h: #define DSNT_BOUND_SLOTS 64
SENT16 = 0x7B7B                       # sentinel of 16-bit plane buffers (fp16 61 280, bf16 1.3e36: never a plane of the inputs here)
SENT32 = 0x7FC00777                   # sentinel of fp32 buffers (a NaN with a payload)
GUARD = 8                             # sentinel cells checked behind every output


def f32_bits(x):
    a = np.asarray(x, dtype=np.float32)
    return (a if a.flags.c_contiguous else np.ascontiguousarray(a)).view(np.uint32)


def bits16(h):
    """Bit patterns of an fp16 array (bf16 planes are uint16 already)."""
    h = np.ascontiguousarray(h)
    return h.view(np.uint16) if h.dtype == np.float16 else h.astype(np.uint16, copy=False)


def bf16_to_f32(p):
    return (np.asarray(p, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


# ------------------------------------------------------------------------------------------------------------- the splits
def pow2_scale(bound):
    """conv_split.h: 2^k with bound * 2^k in [2^13, 2^14): bound = m 2^E, 1 <= m < 2 -> k = 13 - E, from the exponent FIELD of the
    fp32 pattern (so a zero or subnormal bound reads E = -127), E clamped to [-100, 100].  Hence 2^113 for 0 and subnormals,
    2^-87 for +inf.  Scalar or array; returns float32."""
    e = ((f32_bits(bound).astype(np.int64) & 0x7FFFFFFF) >> 23) - 127
    e = np.clip(e, -100, 100)
    s = ((127 + 13 - e).astype(np.uint32) << 23).view(np.float32)
    return s if np.ndim(bound) else s.reshape(())[()]


def f16x2(x, bound):
    """The two fp16 planes of x at `bound`: v = fp32(x s), s = pow2_scale(bound); h1 = fp16_rne(v); h2 = fp16_rne(fp32(v - h1)).
    fp16 subnormals are kept in both planes; v - h1 is exact in fp32 (h1 is v rounded to 11 bits).  A zero keeps its sign in
    h1 and h2 = v - h1 is +0 whenever h1 == v.  Returns (h1, h2, v)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        v = x * np.float32(pow2_scale(np.float32(bound)))
        h1 = v.astype(np.float16)
        h2 = (v - h1.astype(np.float32)).astype(np.float16)
    return h1, h2, v


def _bf16_rne(x):
    """fp32 -> bf16 by the conversion (torch's CPU cast rounds to nearest even); uint16 patterns."""
    t = torch.from_numpy(np.array(x, dtype=np.float32)).to(torch.bfloat16)          # (a copy: torch wants a writable array)
    return t.view(torch.int16).numpy().view(np.uint16)


def _bf16_rne_by_hand(x):
    u = f32_bits(x)
    return (((u + np.uint32(0x7FFF) + ((u >> 16) & np.uint32(1))) & np.uint32(0xFFFF0000)) >> 16).astype(np.uint16)


def _bf16x3(x, rne):
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        p1 = rne(x)
        r1 = x - bf16_to_f32(p1)
        p2 = rne(r1)
        p3 = rne(r1 - bf16_to_f32(p2))
    return p1, p2, p3


def bf16x3(x):
    """The three bf16 planes of x: p1 = bf16_rne(x), p2 = bf16_rne(x - p1), p3 = bf16_rne(x - p1 - p2), subtractions in fp32
    (both exact).  EXACT DOMAIN: p1 + p2 + p3 == x for x = +-0 and for every fp32 with 2^-100 <= |x| < 2^100.  Far below
    (|x| < 2^-110) the third plane is a bf16 subnormal and no longer holds the last bits; near the top of the range p1 rounds
    to infinity.  The planes themselves are defined (and compared) everywhere; only the sum is not claimed outside the domain."""
    return _bf16x3(x, _bf16_rne)


def bf16x3_by_hand(x):
    """The same split with the rounding in integers, as pack_dgrad_all_kernel does it:
    (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000.  Equal to bf16x3 for every finite x whose plane 0 is finite; for the last half
    bf16 ulp under FLT_MAX plane 0 is +-inf in both forms, plane 1 -+inf, and plane 2 a NaN whose payload differs — the integer
    form does not know NaNs (tests/test_split_ref_cpu.py)."""
    return _bf16x3(x, _bf16_rne_by_hand)


def in_exact_domain(x):
    a = np.abs(np.asarray(x, dtype=np.float32))
    return (a == 0) | ((a >= np.float32(2.0 ** -100)) & (a < np.float32(2.0 ** 100)))


def restrict_exact(x, fill):
    """x with the elements outside bf16x3's exact domain replaced by `fill` (keeping their sign)."""
    x = np.asarray(x, dtype=np.float32)
    return np.where(in_exact_domain(x), x, np.copysign(np.float32(fill), x)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- the bounds
def amax(x):
    """max |x| over the elements that are not NaN (0 for an all-zero or all-NaN tensor), as float32."""
    a = np.abs(np.asarray(x, dtype=np.float32)).ravel()
    a = a[~np.isnan(a)]
    return np.float32(a.max()) if a.size else np.float32(0)


def bn_bound(gamma, beta, sqrtM):
    """max_c(|gamma_c| sqrt(M) + |beta_c|) in fp64 (sqrtM: the fp32 value the kernel is handed)."""
    g, b = np.abs(np.asarray(gamma, dtype=np.float64)), np.abs(np.asarray(beta, dtype=np.float64))
    return float((g * float(sqrtM) + b).max())


BN_BOUND_REL = 2.0 ** -23 * (1 + 2.0 ** -23)   # fp32 |gamma| sqrt(M) + |beta|: two roundings, (1 + 2^-24)^2 - 1 (one if contracted)


# ------------------------------------------------------------------------------------------------- layouts, as plain gathers
def stream_order(plane, Cout, Cin):
    """OHWI 3x3 [Cout][9][Cin] -> the stream layout [Cin / 16][9 taps][Cout][16] (flat)."""
    assert Cin % 16 == 0 and plane.size == Cout * 9 * Cin
    return np.ascontiguousarray(plane.reshape(Cout, 9, Cin // 16, 16).transpose(2, 1, 0, 3)).ravel()


def s2d_input(x):
    """NCHW [N][C <= 4][H][W] (H, W even) -> [N][H/2+1][W/2+1][16]:
    dst[n][1+i][1+j][(dy*2+dx)*4 + c] = src[n][c][2i+dy][2j+dx]; channels C..3, block row 0 and block column 0 are zero."""
    N, C, H, W = x.shape
    out = np.zeros((N, H // 2 + 1, W // 2 + 1, 2, 2, 4), dtype=x.dtype)
    out[:, 1:, 1:, :, :, :C] = x.reshape(N, C, H // 2, 2, W // 2, 2).transpose(0, 2, 4, 3, 5, 1)
    return out.reshape(N, H // 2 + 1, W // 2 + 1, 16)


def s2d_weights(w):
    """OHWI [Cout][7][7][4] -> [Cout][4][4][16]: w2[co][R][S][(dy*2+dx)*4 + c] = w[co][2R+dy-1][2S+dx-1][c], zero outside the 7x7
    (a zero row on top and a zero column on the left make it 8x8)."""
    Cout = w.shape[0]
    w8 = np.zeros((Cout, 8, 8, 4), dtype=w.dtype)
    w8[:, 1:, 1:] = w
    return np.ascontiguousarray(w8.reshape(Cout, 4, 2, 4, 2, 4).transpose(0, 1, 3, 2, 4, 5)).reshape(Cout, 4, 4, 16)


def s2d_weights_back(g2):
    """The back = 1 gather: dw[co][r][s][c] = dw2[co][(r+1)/2][(s+1)/2][(((r+1)&1)*2 + ((s+1)&1))*4 + c]."""
    Cout = g2.shape[0]
    g8 = g2.reshape(Cout, 4, 4, 2, 2, 4).transpose(0, 1, 3, 2, 4, 5).reshape(Cout, 8, 8, 4)
    return np.ascontiguousarray(g8[:, 1:, 1:])


def zero_insert(dy, Hs, Ws, s):
    """NHWC [N][Ho][Wo][C] -> [N][Hs][Ws][C]: out[n][oh*s][ow*s][c] = dy[n][oh][ow][c], +0 elsewhere."""
    N, Ho, Wo, C = dy.shape
    assert Hs >= (Ho - 1) * s + 1 and Ws >= (Wo - 1) * s + 1
    out = np.zeros((N, Hs, Ws, C), dtype=dy.dtype)
    out[:, 0:(Ho - 1) * s + 1:s, 0:(Wo - 1) * s + 1:s] = dy
    return out


def pack_dgrad(w):
    """OHWI [Cout][R][S][Cin] -> [Cin][R][S][Cout]: wd[ci][R-1-r][S-1-s][co] = w[co][r][s][ci]."""
    return np.ascontiguousarray(w[:, ::-1, ::-1, :].transpose(3, 1, 2, 0))


# --------------------------------------------------------------------------------------------- inputs that make rounding visible
# Classes of designed_values(), dealt to the indices i < n - 1 with i % (2 len + 1) < len (so a class meets every lane of a
# float4 and both halves of a packed conversion); the other indices are log-uniform over 40 binades below the bound with a
# random sign; index n - 1 holds the bound itself.  `v` = x s is the scaled value, s = pow2_scale(bound).
CLASSES = ('bf16_tie_even',    # low 16 bits 0x8000, bit 16 clear: plane 0 rounds down
           'bf16_tie_odd',     # low 16 bits 0x8000, bit 16 set: plane 0 rounds up
           'f16_tie_hi',       # v half way between two fp16 normals (both parities)
           'f16_tie_lo',       # v = h1 + r, r half way between two fp16 normals: the tie is in the LOW plane
           'f16_tie_sub',      # v = (j + 1/2) 2^-24: a tie between fp16 subnormals (j = 0: 2^-25 ties to zero)
           'lo_subnormal',     # 2^-14 <= |v| < 2^-3: the low plane is an fp16 subnormal
           'hi_subnormal',     # 2^-24 <= |v| < 2^-14: the high plane is
           'vanish',           # |v| <= 2^-25: both planes are zero (and just above: the smallest survivor)
           'zero',             # +0 and -0
           'f32_subnormal')    # an fp32 subnormal input


def _special(r, k, m, bound, s):
    """m values (float64, each exactly an fp32) of class k."""
    sign = np.where(r.random(m) < 0.5, -1.0, 1.0)
    name = CLASSES[k]
    if name.startswith('bf16_tie'):
        mag = (float(bound) * 2.0 ** -r.uniform(1.0, 12.0, m)).astype(np.float32)   # a binade below the bound's, or lower
        u = mag.view(np.uint32) & np.uint32(0xFFFE0000) | np.uint32(0x8000)
        if name == 'bf16_tie_odd':
            u |= np.uint32(0x10000)
        return sign * u.view(np.float32).astype(np.float64)
    if name == 'f16_tie_hi':
        e = r.integers(-14, 13, m)
        v = (r.integers(1024, 2048, m) + 0.5) * 2.0 ** (e - 10)
    elif name == 'f16_tie_lo':
        e = r.integers(-2, 13, m)                       # h1 in [2^e, 2^(e+1)), r in [2^(e-12), 2^(e-11)): 24 bits in all
        sub = np.where(r.random(m) < 0.5, -1.0, 1.0)
        v = r.integers(1025, 2047, m) * 2.0 ** (e - 10) + sub * (r.integers(1024, 2048, m) + 0.5) * 2.0 ** (e - 22)
    elif name == 'f16_tie_sub':
        j = r.integers(0, 1024, m)
        j[::5] = 0
        v = (j + 0.5) * 2.0 ** -24
    elif name == 'lo_subnormal':
        v = r.integers(1 << 23, 1 << 24, m) * 2.0 ** (r.integers(-14, -3, m) - 23)
    elif name == 'hi_subnormal':
        v = r.integers(1 << 23, 1 << 24, m) * 2.0 ** (r.integers(-24, -14, m) - 23)
    elif name == 'vanish':
        v = r.integers(1 << 23, 1 << 24, m) * 2.0 ** (r.integers(-40, -25, m) - 24)   # < 2^-25
        v[::3] = 2.0 ** -25                                                         # the tie: to even, zero
        v[1::3] = 2.0 ** -25 * (1 + 2.0 ** -23)                                     # just above: rounds to 2^-24
    elif name == 'zero':
        return sign * 0.0
    else:
        return sign * r.integers(1, 1 << 23, m) * 2.0 ** -149
    return sign * v / float(s)


def designed_values(r, n, bound=1.0):
    """n fp32 values with max |x| == `bound` (a positive normal fp32), held by the LAST element; see CLASSES.  Give it a bound
    whose significand is just under 2 (|x s| just under 2^14 at the last index) and one that is a power of two."""
    bound = np.float32(bound)
    assert np.isfinite(bound) and 2.0 ** -60 <= bound <= 2.0 ** 60
    s = pow2_scale(bound)
    m = n - 1
    x = np.where(r.random(m) < 0.5, -1.0, 1.0) * float(bound) * 2.0 ** -r.uniform(0.0, 40.0, m)
    cls = np.arange(m) % (2 * len(CLASSES) + 1)
    for k in range(len(CLASSES)):
        at = np.nonzero(cls == k)[0]
        if at.size:
            x[at] = _special(r, k, at.size, bound, s)
    x32 = np.append(x, float(bound)).astype(np.float32)
    assert np.array_equal(x32[:m][cls < len(CLASSES)].astype(np.float64), x[cls < len(CLASSES)]), 'a designed value is no fp32'
    assert amax(x32) == bound
    return x32


def _is_tie16(v, h):
    """v (fp32, exact) lies half way between h = fp16_rne(v) and its neighbour (away from a binade edge)."""
    d = np.abs(v.astype(np.float64) - h.astype(np.float64))
    with np.errstate(invalid='ignore', over='ignore'):
        ulp = np.spacing(np.abs(h)).astype(np.float64)
    return (d > 0) & (d == ulp / 2)


def classify(x, bound):
    """Counts of what designed_values promises, measured on the values themselves."""
    x = np.asarray(x, dtype=np.float32)
    u = f32_bits(x)
    h1, h2, v = f16x2(x, bound)
    a1, a2, av = np.abs(h1.astype(np.float64)), np.abs(h2.astype(np.float64)), np.abs(v.astype(np.float64))
    normal = (np.abs(x) >= np.float32(2.0 ** -126))
    low = (u & np.uint32(0xFFFF)) == np.uint32(0x8000)
    bbits = int(f32_bits(np.float32(bound)).reshape(-1)[0])
    return {
        'bf16_tie_even': int((low & normal & ((u >> 16) & 1 == 0)).sum()),
        'bf16_tie_odd': int((low & normal & ((u >> 16) & 1 == 1)).sum()),
        'f16_tie_hi': int((_is_tie16(v, h1) & (a1 >= 2.0 ** -14)).sum()),
        'f16_tie_hi_even_down': int((_is_tie16(v, h1) & (a1 >= 2.0 ** -14) & (a1 < av)).sum()),
        'f16_tie_hi_even_up': int((_is_tie16(v, h1) & (a1 >= 2.0 ** -14) & (a1 > av)).sum()),
        'f16_tie_lo': int((_is_tie16(v - h1.astype(np.float32), h2) & (a2 >= 2.0 ** -14)).sum()),
        'f16_tie_sub': int((_is_tie16(v, h1) & (a1 < 2.0 ** -14) & (a1 > 0)).sum()),
        'lo_subnormal': int(((a2 > 0) & (a2 < 2.0 ** -14) & (a1 >= 2.0 ** -14)).sum()),
        'hi_subnormal': int(((a1 > 0) & (a1 < 2.0 ** -14)).sum()),
        'vanish': int((normal & (av <= 2.0 ** -25) & (a1 == 0) & (a2 == 0)).sum()),
        'vanish_tie': int((normal & (av == 2.0 ** -25) & (a1 == 0) & (a2 == 0)).sum()),
        'smallest_survivor': int(((av > 2.0 ** -25) & (av < 2.0 ** -24) & (a1 == 2.0 ** -24)).sum()),
        'zero_pos': int((u == 0).sum()),
        'zero_neg': int((u == np.uint32(0x80000000)).sum()),
        'f32_subnormal': int(((x != 0) & ~normal).sum()),
        'log_uniform_binades': int(np.unique(np.floor(np.log2(np.abs(x[normal & (np.abs(x) <= bound)]).astype(np.float64)))).size),
        'bound_at_last': int(x[-1] == np.float32(bound)),
        'bound_pow2': int((bbits & 0x7FFFFF) == 0),
        'bound_near2': int((bbits & 0x7FFFFF) == 0x7FFFFF),
    }


# ------------------------------------------------------------------------------------- the comparison the GPU test makes
def plane_buffer_len(n, plane_stride, planes):
    return (planes - 1) * plane_stride + n + GUARD


def expected_planes(planes, plane_stride):
    """The whole 16-bit output buffer of a split launch as it must look afterwards: plane k at k * plane_stride, and the
    sentinel in the gaps between planes (plane_stride > n) and in the GUARD cells behind the last one."""
    n = planes[0].size
    buf = np.full(plane_buffer_len(n, plane_stride, len(planes)), SENT16, dtype=np.uint16)
    for k, p in enumerate(planes):
        buf[k * plane_stride:k * plane_stride + n] = bits16(p).ravel()
    return buf


def same_bits(name, got, want, skip=None):
    """Equality of two integer arrays of bit patterns (same dtype and shape), optionally but for the indices `skip`; the
    message names the first differing element.  THE comparison of tests/test_operand_prep_gpu.py — its strength is shown in
    tests/test_split_ref_cpu.py by handing it wrong kernels' outputs."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.dtype.kind in 'ui' and got.shape == want.shape, (
        name, got.dtype, want.dtype, got.shape, want.shape)
    bad = got != want
    if skip is not None:
        bad.ravel()[np.asarray(skip).ravel()] = False
    if bad.any():
        i = np.argwhere(bad)[0]
        raise AssertionError('%s: %d of %d elements differ, first at %s: got 0x%x, want 0x%x' % (
            name, int(bad.sum()), bad.size, i.tolist(), int(got[tuple(i)]), int(want[tuple(i)])))
