"""The operand-preparation kernels of the split-precision convolutions (csrc/conv_prep.hip, the space-to-depth half of
csrc/flat.hip, dsnt_zero_insert of csrc/resample.hip) against the host oracle tests/split_ref.py, through the C ABI.

Bars.  These kernels round to nearest even, subtract exactly and permute, so every comparison is on BIT PATTERNS
(split_ref.same_bits; tests/test_split_ref_cpu.py shows that it catches truncation, flushed fp16 subnormals, two swapped
stream-order indices and a dropped last pass).  The one arithmetic result, the BatchNorm bound, is held to its derived fp32
rounding bound.  Every output buffer is a sentinel first and is compared whole: the gap between planes
(plane_stride > n) and split_ref.GUARD cells behind every output must still be the sentinel afterwards.

Inputs are split_ref.designed_values: ties of both parities in either plane, subnormal high and low planes, vanishing
values, +-0, fp32 subnormals, the bound itself at the last index — at a bound whose significand is just under 2 and at a
power of two.

Sizes.  4 (one float4), 1028 (a ragged second workgroup) and BIG = 4 (2 * 2048 * 256 + 3): the split launches cap their grid
at 2048 x 256 threads, so every thread makes a second pass and three float4 groups a third; dsnt_amax (1024 workgroups) makes
four and a bit.  BIG is 16 MB of fp32, the largest tensor here, and each kernel meets it in one parametrisation."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest
import torch

import split_ref as R
from f16x3_util import LOOSE_A

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BIG = 4 * (2 * 2048 * 256 + 3)
SIZES = [4, 1028, BIG]
NEAR2 = float(np.float32(2.0 - 2.0 ** -23))          # significand just under 2
F_SENT = 777.0


def rng(*seed):
    return np.random.default_rng(list(seed))


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(DEV)


def buf16(n):
    return torch.full((n,), R.SENT16, dtype=torch.int16, device=DEV)


def buf32(n):
    return torch.full((n,), R.SENT32, dtype=torch.int32, device=DEV)


def host16(t):
    return t.cpu().numpy().view(np.uint16)


def host32(t):
    return t.cpu().numpy().view(np.uint32)


def sent32(n):
    return np.full(n, R.SENT32, dtype=np.uint32)


def with_guard(a):
    """Expected content of a buf32: the fp32 array `a` as bits, then GUARD sentinels."""
    return np.concatenate([R.f32_bits(a).ravel(), sent32(R.GUARD)])


def call(name, *args):
    from dsnt._lib import call as c, ptr
    c(name, *[ptr(a) if isinstance(a, torch.Tensor) else a for a in args])


@functools.lru_cache(maxsize=None)
def designed(n, bound, seed=0):
    """Shared and read-only."""
    x = R.designed_values(rng(41, seed, n), n, bound)
    x.setflags(write=False)
    return x


def exact_designed(n, bound, seed=0):
    return R.restrict_exact(designed(n, bound, seed), np.float32(bound) / 3)


def slots(value, how='all'):
    s = np.zeros(R.BOUND_SLOTS, dtype=np.float32)
    if how == 'all':
        s[:] = value
    else:
        s[37] = value
    return dev(s)


def bounds_for(n):
    """Both kinds of bound at the small sizes; the big size once, with |x s| just under 2^14 at the last index."""
    return (NEAR2 * 0.125,) if n == BIG else (NEAR2 * 0.125, 4.0)


# ============================================================================================ dsnt_split_f16x2
@pytest.mark.parametrize('n', SIZES)
def test_split_f16x2(n):
    """Both planes at every size, tight and padded plane stride, the bound in all 64 slots / in slot 37 alone (bound64 is
    the maximum of the slots) / LOOSE_A = 2^8 too large (eight more bits go to the low plane and below)."""
    if n == BIG:
        assert n // 4 > 2 * 2048 * 256 and n // 4 - 2 * 2048 * 256 == 3
    for bound in bounds_for(n):
        x = designed(n, bound)
        xd = dev(x)
        for loose, hows in ((1.0, ('all', 'one')), (LOOSE_A, ('all',))):
            b = np.float32(bound) * np.float32(loose)
            planes = list(R.f16x2(x, b)[:2])
            for how in hows:
                bd = slots(b, how)
                for stride in (n, n + 12):
                    out = buf16(R.plane_buffer_len(n, stride, 2))
                    call('dsnt_split_f16x2', xd, out, n, stride, bd)
                    R.same_bits('split_f16x2 n %d bound %r x %g (%s) stride %d' % (n, bound, loose, how, stride),
                                host16(out), R.expected_planes(planes, stride))


def test_split_f16x2_of_zeros_at_a_zero_bound():
    """Bound 0 (scale clamped to 2^113) on an all-zero tensor: plane 0 keeps the sign of each zero, plane 1 is +0."""
    n = 1028
    x = np.zeros(n, dtype=np.float32)
    x[1::3] = -0.0
    out = buf16(R.plane_buffer_len(n, n + 4, 2))
    call('dsnt_split_f16x2', dev(x), out, n, n + 4, slots(0.0))
    want = R.expected_planes(list(R.f16x2(x, 0.0)[:2]), n + 4)
    assert set(want[:n].tolist()) == {0, 0x8000} and not want[n + 4:2 * n + 4].any()
    R.same_bits('zeros', host16(out), want)


# ================================================================================================== dsnt_amax
def _amax_check(name, x):
    out = torch.full((R.BOUND_SLOTS + R.GUARD,), F_SENT, device=DEV)
    call('dsnt_amax', dev(x), x.size, out)
    o = out.cpu().numpy()
    want = R.amax(x)
    assert (o[R.BOUND_SLOTS:] == F_SENT).all(), name
    s = o[:R.BOUND_SLOTS]
    assert R.f32_bits(s.max())[()] == R.f32_bits(want)[()], (name, float(s.max()), float(want))
    assert (s >= 0).all() and (s <= want).all() and not np.signbit(s).any(), name
    return out


@pytest.mark.parametrize('n', SIZES)
def test_amax(n):
    """The maximum at index 0, at the last index and — BIG: in the third pass of the 1024-workgroup grid — in the middle;
    negative; an all-zero tensor; an fp32-subnormal maximum; and the entry clears its output, so a second call on a smaller
    tensor lowers the value."""
    x = designed(n, NEAR2 * 0.125)
    mid = 4 * (2 * 1024 * 256 + 12345) + 2 if n == BIG else n // 2
    assert 0 < mid < n - 1
    out = _amax_check('last', x)
    for at in (0, mid):
        y = x.copy()
        y[at], y[-1] = -x[-1], x[at]
        _amax_check('at %d, negative' % at, y)
    _amax_check('negative at last', -x)
    z = np.zeros(n, dtype=np.float32)
    z[1::3] = -0.0
    _amax_check('zeros', z)
    sub = (rng(42, n).integers(0, 1 << 22, n) * 2.0 ** -149).astype(np.float32)
    sub[mid] = -np.float32((2 ** 23 - 1) * 2.0 ** -149)
    assert 0 < R.amax(sub) < np.float32(2.0 ** -126)
    _amax_check('subnormal', sub)
    small = np.ascontiguousarray(x[:4] * np.float32(0.25))
    call('dsnt_amax', dev(small), 4, out)
    assert R.f32_bits(out[:R.BOUND_SLOTS].max().item())[()] == R.f32_bits(R.amax(small))[()] and R.amax(small) < R.amax(x)


# ===================================================================================== dsnt_f16_prep_weights
# n / 4 of the plain rows: one float4; less than a pass; around one pass of 1024 groups; around one unrolled pass of 4096;
# tail passes only with a partial last one; one unrolled pass + three tail passes + one group; ResNet's 64 -> 64 3x3 filter
# (two unrolled passes, one full tail pass); nine unrolled passes exactly.  Magnitudes 2^-20 ... 2^6, bounds alternately a
# power of two and just under one; one row of zeros.  Stream rows (Cout, Cin): n / 4 = 3456 (tail passes only, partial
# last one) and 11520 (two unrolled passes, three tail passes, a partial one).
PLAIN_N4 = [1, 16, 1023, 1024, 1025, 4095, 4096, 4097, 3 * 1024 + 5, 7 * 1024 + 1, 9216, 36864]
PLAIN_LOG2 = [-20, -18, -15, -13, -10, -8, -6, -3, -1, 1, 4, 6]
STREAM_ROWS = [(48, 32), (64, 80)]


def _prep_rows(row_ints):
    rows = []
    for i, (n4, e) in enumerate(zip(PLAIN_N4, PLAIN_LOG2)):
        bound = 2.0 ** e if i % 2 else NEAR2 * 2.0 ** (e - 1)
        rows.append((designed(4 * n4, bound, seed=i), 0, 0))
        if i == 5:
            z = np.zeros(4 * 1025, dtype=np.float32)
            z[2::5] = -0.0
            rows.append((z, 0, 0))
    if row_ints == 5:
        return [rows[k] for k in (4, 1, 6, 11, 8)]
    for k, (co, ci) in enumerate(STREAM_ROWS):
        rows.append((designed(co * 9 * ci, NEAR2 * 2.0 ** (-5 + 3 * k), seed=20 + k), co, ci))
    assert [r[0].size // 4 for r in rows[-2:]] == [3456, 11520]
    return rows


@pytest.mark.parametrize('row_ints', [7, 5])
def test_f16_prep_weights_table(row_ints):
    """Every row of one launch: its bound (all 64 slots, bit for bit the maximum) and its two planes — in stream order for
    the stream rows — with the rows' outputs back to back in one buffer, so that a row writing outside its own cells lands
    in a neighbour's planes, gap or guard."""
    rows = _prep_rows(row_ints)
    src = dev(np.concatenate([r[0] for r in rows]))
    strides = [r[0].size + (12 if k % 2 else 0) for k, r in enumerate(rows)]
    lens = [R.plane_buffer_len(r[0].size, st, 2) for r, st in zip(rows, strides)]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out = buf16(int(offs[-1]))
    W = R.BOUND_SLOTS + R.GUARD
    bnd = buf32(len(rows) * W)
    table, s_off = [], 0
    for k, (x, co, ci) in enumerate(rows):
        assert src.data_ptr() % 16 == 0 and (out.data_ptr() + 2 * int(offs[k])) % 8 == 0
        table.append([src.data_ptr() + 4 * s_off, out.data_ptr() + 2 * int(offs[k]), bnd.data_ptr() + 4 * k * W, x.size, strides[k]]
                     + ([co, ci] if row_ints == 7 else []))
        s_off += x.size
    call('dsnt_f16_prep_weights', dev(np.array(table, dtype=np.int64)), len(rows), row_ints)
    got, gotb = host16(out), host32(bnd)
    for k, (x, co, ci) in enumerate(rows):
        b = R.amax(x)
        name = 'row %d (n/4 %d, bound %g, stream %d x %d)' % (k, x.size // 4, b, co, ci)
        R.same_bits(name + ' bound', gotb[k * W:(k + 1) * W], np.concatenate([np.full(R.BOUND_SLOTS, R.f32_bits(b)[()], dtype=np.uint32),
                                                                            sent32(R.GUARD)]))
        planes = [R.bits16(h) for h in R.f16x2(x, b)[:2]]
        if co:
            planes = [R.stream_order(p, co, ci) for p in planes]
        R.same_bits(name, got[offs[k]:offs[k + 1]], R.expected_planes(planes, strides[k]))


# ===================================================================================== dsnt_s2d_weights_prep
@pytest.mark.parametrize('Cout', [8, 64, 72])
def test_s2d_weights_prep(Cout):
    """The stem's one-launch preparation (Cout 72: the loop form past 16 groups per thread): the re-packed filter, its bound
    and its fp16 and bf16 planes are the references applied to split_ref.s2d_weights of the filter; w2 may be NULL."""
    bound = NEAR2 * 0.25 if Cout != 64 else 0.5
    w = designed(Cout * 196, bound, seed=3).reshape(Cout, 7, 7, 4)
    w2 = R.s2d_weights(w).ravel()
    n = w2.size
    assert n == Cout * 256 and R.amax(w2) == np.float32(bound)
    want_b = np.concatenate([np.full(R.BOUND_SLOTS, R.f32_bits(np.float32(bound))[()], dtype=np.uint32), sent32(R.GUARD)])
    want16 = R.expected_planes(list(R.f16x2(w2, bound)[:2]), n)
    want6 = R.expected_planes(list(R.bf16x3(w2)), n)
    wd = dev(w)
    for with_w2 in (True, False):
        o2, p16, p6, bnd = buf32(n + R.GUARD), buf16(want16.size), buf16(want6.size), buf32(R.BOUND_SLOTS + R.GUARD)
        call('dsnt_s2d_weights_prep', wd, o2 if with_w2 else None, p16, p6, bnd, Cout)
        R.same_bits('w2', host32(o2), with_guard(w2) if with_w2 else sent32(n + R.GUARD))
        R.same_bits('bound', host32(bnd), want_b)
        R.same_bits('fp16 planes', host16(p16), want16)
        R.same_bits('bf16 planes', host16(p6), want6)


# ========================================================================================= dsnt_split_bf16x3
@pytest.mark.parametrize('n', SIZES)
def test_split_bf16x3(n):
    """On the designed values restricted to the exact domain the three planes (plane stride n) equal the reference and — on
    the host, in fp64 — sum to the input exactly.  At the middle size also on the unrestricted values (fp32 subnormals
    among them): the planes are defined there too, only their sum is not claimed."""
    for bound in bounds_for(n):
        for x in [exact_designed(n, bound)] + ([designed(n, bound)] if n == 1028 else []):
            dom = R.in_exact_domain(x)
            out = buf16(R.plane_buffer_len(n, n, 3))
            call('dsnt_split_bf16x3', dev(x), out, n)
            got = host16(out)
            R.same_bits('split_bf16x3 n %d bound %r' % (n, bound), got, R.expected_planes(list(R.bf16x3(x)), n))
            total = sum(R.bf16_to_f32(got[k * n:(k + 1) * n]).astype(np.float64) for k in range(3))
            assert np.array_equal(total[dom], x.astype(np.float64)[dom])
        assert R.in_exact_domain(exact_designed(n, bound)).all() and (n != 1028 or not dom.all())


# ============================================================================ dsnt_conv_pack_dgrad(_all)
PACK_CONVS = [(128, 3, 3, 128), (256, 1, 1, 128), (16, 1, 1, 256), (256, 1, 1, 16), (64, 7, 7, 4), (48, 3, 3, 80), (36, 1, 1, 20),
              (4, 1, 1, 4)]


def _pack_weights():
    return [exact_designed(co * r * s * ci, (NEAR2 if k % 2 else 1.0) * 2.0 ** (k - 6), seed=50 + k).reshape(co, r, s, ci)
            for k, (co, r, s, ci) in enumerate(PACK_CONVS)]


def test_pack_dgrad_all():
    """Every convolution of one launch: the fp32 pack is the index formula, ALL THREE bf16 planes (the kernel rounds by hand,
    in integers) are the reference split of it, and the GUARD cells left between consecutive convolutions stay untouched."""
    ws = _pack_weights()
    rows, off_s, off_d = [], 0, 0
    for w in ws:
        rows.append([off_s, off_d, *w.shape])
        off_s += w.size
        off_d += (w.size + 7) // 8 * 8 + R.GUARD
    total = off_d
    out, planes = buf32(total + R.GUARD), buf16(3 * total + R.GUARD)
    call('dsnt_conv_pack_dgrad_all', dev(np.array(rows, dtype=np.int32)), len(ws), dev(np.concatenate([w.ravel() for w in ws])),
         out, planes, total)
    want, want_p = sent32(total + R.GUARD), np.full(3 * total + R.GUARD, R.SENT16, dtype=np.uint16)
    for w, row in zip(ws, rows):
        wd = R.pack_dgrad(w).ravel()
        want[row[1]:row[1] + wd.size] = R.f32_bits(wd)
        for k, p in enumerate(R.bf16x3(wd)):
            want_p[k * total + row[1]:k * total + row[1] + wd.size] = p
    R.same_bits('fp32 pack', host32(out), want)
    R.same_bits('bf16 planes', host16(planes), want_p)


def test_pack_dgrad():
    for w in _pack_weights():
        co, r, s, ci = w.shape
        out = buf32(w.size + R.GUARD)
        call('dsnt_conv_pack_dgrad', dev(w), out, co, r, s, ci)
        R.same_bits('pack_dgrad %s' % (w.shape,), host32(out), with_guard(R.pack_dgrad(w)))


# =================================================================================== dsnt_f16_prep_bn_bounds
def test_f16_prep_bn_bounds():
    """max_c(|gamma_c| sqrt(M) + |beta_c|) for several rows of one launch: all 64 slots equal, and within
    2^-23 (1 + 2^-23) of the fp64 value.  That bar is DERIVED, not measured: the fp32 product and sum round twice,
    (1 + 2^-24)^2 - 1, or once where the compiler contracts them into an fma; abs and max are exact."""
    r = rng(43)
    W = R.BOUND_SLOTS + R.GUARD
    cases = []
    for C_ in (4, 60, 64, 68, 256):
        for M in (2 * 1 * 1, 32 * 128 * 128):
            g = (r.standard_normal(C_) * 2.0 ** r.uniform(-6, 2)).astype(np.float32)
            b = (r.standard_normal(C_) * 2.0 ** r.uniform(-6, 2)).astype(np.float32)
            g[r.integers(C_)] *= -3.0                                  # the deciding channel anywhere, also past lane 63's first trip
            cases.append((g, b, M))
    cases.insert(3, (np.zeros(60, dtype=np.float32), -np.zeros(60, dtype=np.float32), 32 * 128 * 128))
    assert any((g < 0).any() and (b < 0).any() for g, b, _ in cases)
    keep = [(dev(g), dev(b)) for g, b, _ in cases]
    out = torch.full((len(cases) * W,), F_SENT, device=DEV)
    table = []
    for k, ((g, b, M), (gd, bd)) in enumerate(zip(cases, keep)):
        sq = np.float32(np.sqrt(np.float64(M)))
        table.append([gd.data_ptr(), bd.data_ptr(), out.data_ptr() + 4 * k * W, g.size, struct.unpack('<I', struct.pack('<f', sq))[0]])
    call('dsnt_f16_prep_bn_bounds', dev(np.array(table, dtype=np.int64)), len(cases))
    o = out.cpu().numpy().reshape(len(cases), W)
    for k, (g, b, M) in enumerate(cases):
        ref = R.bn_bound(g, b, np.float32(np.sqrt(np.float64(M))))
        s = o[k, :R.BOUND_SLOTS]
        print('bn bound row %d C %d M %d: out %.9g ref %.17g err/bar %.3f' % (
            k, g.size, M, s[0], ref, abs(float(s[0]) - ref) / (R.BN_BOUND_REL * ref) if ref else 0.0))
        assert (o[k, R.BOUND_SLOTS:] == F_SENT).all() and (R.f32_bits(s) == R.f32_bits(s)[0]).all(), k
        assert abs(float(s[0]) - ref) <= R.BN_BOUND_REL * ref, (k, float(s[0]), ref)


# ==================================================================================================== layouts
@pytest.mark.parametrize('C_,N,H,W', [(1, 3, 6, 10), (2, 3, 2, 2), (3, 3, 6, 10), (4, 3, 2, 2), (4, 3, 6, 10), (3, 3, 2, 2),
                                      (3, 1, 1024, 1024)])
def test_s2d_input(C_, N, H, W):
    """The space-to-depth image against the gather, without a tail and with the amax tail (which RAISES 64 zeroed slots to
    max |image|).  1 x 3 x 1024 x 1024: 513 x 513 x 4 items, past one stride of the flat grid (4096 x 256)."""
    from dsnt._lib import BnTail
    if H == 1024:
        assert (H // 2 + 1) * (W // 2 + 1) * 4 > 4096 * 256
    x = designed(N * C_ * H * W, NEAR2 * 2.0, seed=7).reshape(N, C_, H, W)
    want = with_guard(R.s2d_input(x))
    xd = dev(x)
    out = buf32(want.size)
    call('dsnt_s2d_input', xd, out, N, C_, H, W, None)
    R.same_bits('s2d_input', host32(out), want)
    out = buf32(want.size)
    am = torch.zeros(R.BOUND_SLOTS + R.GUARD, device=DEV)
    t = BnTail()
    t.amax = am.data_ptr()
    call('dsnt_s2d_input', xd, out, N, C_, H, W, C.byref(t))
    R.same_bits('s2d_input with tail', host32(out), want)
    a = am.cpu().numpy()
    assert R.f32_bits(a.max())[()] == R.f32_bits(R.amax(x))[()] and not a[R.BOUND_SLOTS:].any()


@pytest.mark.parametrize('Cout', [3, 72])
def test_s2d_weights_both_ways(Cout):
    w = designed(Cout * 196, 1.0, seed=8).reshape(Cout, 7, 7, 4)
    out = buf32(Cout * 256 + R.GUARD)
    call('dsnt_s2d_weights', dev(w), out, Cout, 0)
    R.same_bits('forward', host32(out), with_guard(R.s2d_weights(w)))
    g2 = designed(Cout * 256, NEAR2, seed=9).reshape(Cout, 4, 4, 16)
    back = buf32(Cout * 196 + R.GUARD)
    call('dsnt_s2d_weights', dev(g2), back, Cout, 1)
    R.same_bits('back', host32(back), with_guard(R.s2d_weights_back(g2)))


@pytest.mark.parametrize('s,Ho,Wo,eh,ew', [(2, 3, 5, 0, 0), (2, 3, 5, 1, 2), (3, 2, 4, 0, 0), (3, 2, 4, 2, 1), (4, 3, 2, 0, 0),
                                           (4, 3, 2, 3, 5), (2, 1, 1, 0, 0)])
def test_zero_insert(s, Ho, Wo, eh, ew):
    """Strides 2, 3, 4 at the minimal Hs x Ws = (Ho-1) s + 1 x (Wo-1) s + 1 and with slack rows and columns."""
    N, C_ = 2, 8
    Hs, Ws = (Ho - 1) * s + 1 + eh, (Wo - 1) * s + 1 + ew
    dy = designed(N * Ho * Wo * C_, NEAR2, seed=10).reshape(N, Ho, Wo, C_)
    out = buf32(N * Hs * Ws * C_ + R.GUARD)
    call('dsnt_zero_insert', dev(dy), out, N, Ho, Wo, C_, Hs, Ws, s)
    R.same_bits('zero_insert', host32(out), with_guard(R.zero_insert(dy, Hs, Ws, s)))


# ========================================================================================= NaN and infinity
def _prep_one(x):
    n = x.size
    out, bnd = buf16(R.plane_buffer_len(n, n, 2)), buf32(R.BOUND_SLOTS + R.GUARD)
    xd = dev(x)
    call('dsnt_f16_prep_weights', dev(np.array([[xd.data_ptr(), out.data_ptr(), bnd.data_ptr(), n, n, 0, 0]], dtype=np.int64)), 1, 7)
    am = torch.full((R.BOUND_SLOTS,), F_SENT, device=DEV)
    call('dsnt_amax', xd, n, am)
    return host16(out), host32(bnd), am.cpu().numpy()


def test_one_nan_among_the_weights():
    """Characterisation (split_ref's docstring): a NaN does not enter the bound, is a NaN in plane 0 at its index, and every
    other element is bit-exact — so the non-finite guard fires on the loss the NaN reaches, not on a poisoned scale."""
    n, at = 4 * 1025, 4 * 1024 + 1
    x = designed(n, NEAR2 * 0.125).copy()
    x[at] = np.nan
    got, bnd, am = _prep_one(x)
    b = R.amax(x)
    assert b == np.float32(NEAR2 * 0.125)
    assert (bnd[:R.BOUND_SLOTS] == R.f32_bits(b)[()]).all() and R.f32_bits(am.max())[()] == R.f32_bits(b)[()]
    assert (got[at] & 0x7C00) == 0x7C00 and (got[at] & 0x03FF) != 0
    R.same_bits('the other elements', got, R.expected_planes(list(R.f16x2(x, b)[:2]), n), skip=[at, n + at])


def test_one_infinity_among_the_weights():
    n, at = 4 * 1025, 4 * 1024 + 2
    x = designed(n, NEAR2 * 0.125).copy()
    x[at] = np.inf
    got, bnd, am = _prep_one(x)
    assert (bnd[:R.BOUND_SLOTS] == 0x7F800000).all() and am.max() == np.inf
    assert got[at] == 0x7C00
