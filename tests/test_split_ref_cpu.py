"""tests/split_ref.py held to its own definitions on the CPU: the properties csrc/conv_split.h states for pow2_scale and the two
splits, every index formula against a second, independent formulation, the classes designed_values promises, and — last —
the comparison helper of tests/test_operand_prep_gpu.py handed the output of four subtly wrong kernels, so that the strength
of the GPU test is itself tested without running a wrong kernel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import split_ref as R

N_BIG = 1 << 22


def rng(seed):
    return np.random.default_rng(seed)


def finite_patterns(r, n):
    u = r.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    u = u[(u & np.uint32(0x7F800000)) != np.uint32(0x7F800000)]
    return u.view(np.float32)


# ------------------------------------------------------------------------------------------------------------ pow2_scale
def test_pow2_scale_puts_the_bound_in_the_top_fp16_binade():
    r = rng(1)
    b = (2.0 ** r.uniform(-99, 99, 200000)).astype(np.float32)
    s = R.pow2_scale(b)
    p = b.astype(np.float64) * s.astype(np.float64)
    assert s.dtype == np.float32 and (p >= 2.0 ** 13).all() and (p < 2.0 ** 14).all()
    assert (np.log2(s.astype(np.float64)) % 1 == 0).all()
    # the sign bit is not part of the exponent field
    assert np.array_equal(R.pow2_scale(-b), s)


def test_pow2_scale_clamps():
    assert R.pow2_scale(np.float32(0)) == np.float32(2.0 ** 113)
    assert R.pow2_scale(np.float32(2.0 ** -140)) == np.float32(2.0 ** 113)
    assert R.pow2_scale(np.float32(2.0 ** -126)) == np.float32(2.0 ** 113)        # E = -126 clamps to -100 as well
    assert R.pow2_scale(np.float32(2.0 ** -100)) == np.float32(2.0 ** 113)
    assert R.pow2_scale(np.float32(2.0 ** -99)) == np.float32(2.0 ** 112)
    assert R.pow2_scale(np.float32(np.inf)) == np.float32(2.0 ** -87)
    assert R.pow2_scale(np.float32(2.0 ** 101)) == np.float32(2.0 ** -87)
    assert R.pow2_scale(np.float32(1.0)) == 8192.0 and R.pow2_scale(np.float32(1.9999999)) == 8192.0
    assert R.pow2_scale(np.float32(2.0)) == 4096.0
    # where tests/f16x3_util.py's log2 form is valid the two agree
    import f16x3_util
    for b in (1.5, 0.03, 724.1, 2.0 ** -20, 64.0):
        assert R.pow2_scale(np.float32(b)) == f16x3_util.pow2_scale(float(np.float32(b)))


# ----------------------------------------------------------------------------------------------------------------- f16x2
def test_f16x2_error_bound_of_two_roundings():
    """|v - h1 - h2| <= max(2^-22 |v|, 2^-25) in scaled units: h2 rounds a residual <= 2^-11 |v| to 11 bits, or — once it is
    an fp16 subnormal — to a multiple of 2^-24.  Hence |x - (h1 + h2) / s| <= max(2^-22 |x|, 2^-38 bound)."""
    r = rng(2)
    bound = np.float32(1.7)
    x = np.concatenate([R.designed_values(r, N_BIG // 2, bound),
                        (r.uniform(-1, 1, N_BIG // 2) * float(bound)).astype(np.float32)])
    h1, h2, v = R.f16x2(x, bound)
    v64 = v.astype(np.float64)
    err = np.abs(v64 - h1.astype(np.float64) - h2.astype(np.float64))
    bar = np.maximum(2.0 ** -22 * np.abs(v64), 2.0 ** -25)
    assert (err <= bar).all() and (err / bar).max() == 1.0
    s = float(R.pow2_scale(bound))
    assert np.array_equal(v64, x.astype(np.float64) * s)                      # the scaling is exact (no fp32 underflow here)
    errx = np.abs(x.astype(np.float64) - (h1.astype(np.float64) + h2.astype(np.float64)) / s)
    assert (errx <= np.maximum(2.0 ** -22 * np.abs(x.astype(np.float64)), 2.0 ** -38 * float(bound))).all()
    assert np.isfinite(h1.astype(np.float32)).all() and np.abs(v64).max() < 2.0 ** 14


def test_fp16_conversion_of_numpy_is_torch_s_bit_for_bit():
    """The oracle's fp32 -> fp16 rounding is numpy's; torch's CPU cast, a second implementation, gives the same bits on the
    scaled designed values (ties, subnormals, vanishing values) and on random ones below fp16's overflow."""
    r = rng(16)
    _, _, v = R.f16x2(R.designed_values(r, N_BIG // 2, BOUND), BOUND)
    v = np.concatenate([v, (r.standard_normal(N_BIG // 2) * 2.0 ** r.uniform(-30, 14, N_BIG // 2)).astype(np.float32)])
    v = v[np.abs(v) < 65504]
    assert np.array_equal(R.bits16(v.astype(np.float16)), torch.from_numpy(v).to(torch.float16).view(torch.int16).numpy().view(np.uint16))


def test_f16x2_underflow_costs_2_to_the_minus_38_of_the_bound():
    """The case conv_split.h's comment had as 2^-40: bound 1.0, x = 2^-38 -> v = 2^-25 ties to even (zero) in plane 0, the
    residual 2^-25 does the same in plane 1: both planes zero, error 2^-38 bound — attained."""
    h1, h2, v = R.f16x2(np.array([2.0 ** -38, -2.0 ** -38, 2.0 ** -38 * (1 + 2.0 ** -23)], dtype=np.float32), 1.0)
    assert v[0] == np.float32(2.0 ** -25)
    assert R.bits16(h1).tolist() == [0x0000, 0x8000, 0x0001] and R.bits16(h2)[:2].tolist() == [0x0000, 0x8000]


def test_f16x2_keeps_subnormals_and_the_sign_of_zero():
    x = np.array([0.0, -0.0, 2.0 ** -37, -3 * 2.0 ** -37, 2.0 ** -26 + 2.0 ** -37], dtype=np.float32)   # s = 2^13
    h1, h2, _ = R.f16x2(x, 1.0)
    assert R.bits16(h1).tolist() == [0x0000, 0x8000, 0x0001, 0x8003, 0x0800]
    assert R.bits16(h2).tolist() == [0, 0, 0, 0, 0x0001]


# ----------------------------------------------------------------------------------------------------------------- bf16x3
def _sum3(p):
    return sum(R.bf16_to_f32(q).astype(np.float64) for q in p)


def test_bf16x3_is_exact_on_its_domain():
    r = rng(3)
    x = (np.where(r.random(N_BIG) < 0.5, -1.0, 1.0) * 2.0 ** r.uniform(-100, 100, N_BIG)).astype(np.float32)
    u = x.view(np.uint32).copy()
    u[::7] = u[::7] & np.uint32(0xFFFE0000) | np.uint32(0x8000)               # forced plane-0 ties, bit 16 clear ...
    u[3::7] = u[3::7] & np.uint32(0xFFFE0000) | np.uint32(0x18000)            # ... and set
    x = u.view(np.float32)
    x = x[(np.abs(x) >= np.float32(2.0 ** -100)) & (np.abs(x) < np.float32(2.0 ** 100))]
    assert x.size > N_BIG - 64 and R.in_exact_domain(x).all()
    p = R.bf16x3(x)
    assert int((_sum3(p) != x.astype(np.float64)).sum()) == 0
    # the planes shrink by 2^-8 each (8 bits per plane)
    a = [np.abs(R.bf16_to_f32(q).astype(np.float64)) for q in p]
    assert (a[1] <= 2.0 ** -8 * a[0]).all() and (a[2] <= 2.0 ** -8 * np.maximum(a[1], 2.0 ** -9 * a[0])).all()
    z = R.bf16x3(np.array([0.0, -0.0], dtype=np.float32))
    assert [q.tolist() for q in z] == [[0, 0x8000], [0, 0], [0, 0]]


def test_bf16x3_exactness_is_not_claimed_far_below_the_domain():
    """Below 2^-110 a 24-bit significand no longer fits: the third plane would need bits under the smallest bf16 subnormal 2^-133."""
    x = np.array([(1 + 2.0 ** -23) * 2.0 ** -112], dtype=np.float32)
    assert not R.in_exact_domain(x).any() and _sum3(R.bf16x3(x))[0] != float(x[0])


def test_bf16_rounding_by_hand_equals_the_conversion():
    x = finite_patterns(rng(4), N_BIG)
    a, b = R.bf16x3(x), R.bf16x3_by_hand(x)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    fin = np.isfinite(R.bf16_to_f32(a[0]))                       # all but the last half bf16 ulp under FLT_MAX
    assert (~fin).sum() < 1e-4 * x.size and (np.abs(x[~fin]) >= np.float32(2.0 ** 128 - 2.0 ** 119)).all()
    assert np.array_equal(a[2][fin], b[2][fin]) and np.isnan(R.bf16_to_f32(a[2][~fin])).all() and np.isnan(R.bf16_to_f32(b[2][~fin])).all()
    ties = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3FFF8000, 0x7F7F8000, 0x00008000, 0x00018000], dtype=np.uint32)
    got = R.bf16x3_by_hand(ties.view(np.float32))[0]
    assert got.tolist() == [0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x4000, 0x7F80, 0x0000, 0x0002]
    assert np.array_equal(R.bf16x3(ties.view(np.float32))[0], got)


# ---------------------------------------------------------------------------------------------------------------- layouts
def test_stream_order_is_the_permutation_the_header_states():
    for Cout, Cin in ((48, 32), (64, 80), (1, 16)):
        n = Cout * 9 * Cin
        ids = np.arange(n, dtype=np.int64)
        out = R.stream_order(ids, Cout, Cin)
        assert np.array_equal(np.sort(out), ids)
        # second formulation: scatter every source element to its computed destination
        co, tap, c = np.unravel_index(ids, (Cout, 9, Cin))
        dst = (((c // 16) * 9 + tap) * Cout + co) * 16 + c % 16
        want = np.empty(n, dtype=np.int64)
        want[dst] = ids
        assert np.array_equal(out, want)
        # one K step (16 channels of one tap, every output channel) is one contiguous block
        blk = out.reshape(Cin // 16, 9, Cout * 16)[1 % (Cin // 16), 4]
        co_b, tap_b, c_b = np.unravel_index(blk, (Cout, 9, Cin))
        assert (tap_b == 4).all() and (c_b // 16 == 1 % (Cin // 16)).all()


def test_space_to_depth_forms_compute_the_stem_convolution():
    """s2d_input and s2d_weights against torch: pixel_unshuffle for the image, and the 7x7 / stride 2 / pad 3 convolution
    itself — on integers, so fp64 is exact and the two convolutions must be EQUAL."""
    r = rng(5)
    for C, (H, W) in ((3, (6, 10)), (1, (2, 2)), (4, (8, 6)), (2, (4, 12))):
        x = r.integers(-9, 10, (3, C, H, W)).astype(np.float64)
        w = np.zeros((5, 7, 7, 4))
        w[..., :C] = r.integers(-9, 10, (5, 7, 7, C))
        xs, w2 = R.s2d_input(x), R.s2d_weights(w)
        assert xs.shape == (3, H // 2 + 1, W // 2 + 1, 16) and w2.shape == (5, 4, 4, 16)
        pu = F.pixel_unshuffle(torch.from_numpy(x), 2).reshape(3, C, 2, 2, H // 2, W // 2).permute(0, 4, 5, 2, 3, 1).numpy()
        assert np.array_equal(xs[:, 1:, 1:].reshape(3, H // 2, W // 2, 2, 2, 4)[..., :C], pu)
        assert not xs[:, 0].any() and not xs[:, :, 0].any() and not xs.reshape(3, H // 2 + 1, W // 2 + 1, 4, 4)[..., C:].any()
        want = F.conv2d(torch.from_numpy(x), torch.from_numpy(w[..., :C]).permute(0, 3, 1, 2), stride=2, padding=3)
        got = F.conv2d(torch.from_numpy(xs).permute(0, 3, 1, 2), torch.from_numpy(w2).permute(0, 3, 1, 2), stride=1, padding=1)
        assert torch.equal(got, want)


def test_s2d_weights_back_is_the_adjoint_and_the_left_inverse():
    r = rng(6)
    w = r.integers(-9, 10, (6, 7, 7, 4)).astype(np.float64)
    g2 = r.integers(-9, 10, (6, 4, 4, 16)).astype(np.float64)
    assert np.array_equal(R.s2d_weights_back(R.s2d_weights(w)), w)
    assert (R.s2d_weights(w) * g2).sum() == (w * R.s2d_weights_back(g2)).sum()
    # the header's formula, element by element
    back = R.s2d_weights_back(g2)
    for co, rr, ss, c in ((0, 0, 0, 0), (5, 6, 6, 3), (2, 3, 4, 1), (1, 0, 5, 2)):
        assert back[co, rr, ss, c] == g2[co, (rr + 1) // 2, (ss + 1) // 2, (((rr + 1) & 1) * 2 + ((ss + 1) & 1)) * 4 + c]


def test_zero_insert_is_the_scatter_half_of_conv_transpose2d():
    r = rng(7)
    for s, (Ho, Wo), (eh, ew) in ((2, (3, 5), (0, 0)), (3, (2, 4), (2, 1)), (4, (3, 2), (3, 5)), (2, (1, 1), (1, 0))):
        dy = r.integers(1, 10, (2, Ho, Wo, 8)).astype(np.float64)
        Hs, Ws = (Ho - 1) * s + 1 + eh, (Wo - 1) * s + 1 + ew
        eye = torch.eye(8, dtype=torch.float64).reshape(8, 8, 1, 1)
        t = F.conv_transpose2d(torch.from_numpy(dy).permute(0, 3, 1, 2), eye, stride=s)
        t = F.pad(t, (0, ew, 0, eh)).permute(0, 2, 3, 1).numpy()
        assert np.array_equal(R.zero_insert(dy, Hs, Ws, s), t)


def test_pack_dgrad_against_the_loop_and_as_an_involution():
    r = rng(8)
    for Cout, Rr, S, Cin in ((4, 1, 1, 4), (5, 3, 3, 7), (3, 7, 7, 2)):
        w = r.standard_normal((Cout, Rr, S, Cin)).astype(np.float32)
        wd = R.pack_dgrad(w)
        want = np.empty((Cin, Rr, S, Cout), dtype=np.float32)
        for co in range(Cout):
            for a in range(Rr):
                for b in range(S):
                    for ci in range(Cin):
                        want[ci, Rr - 1 - a, S - 1 - b, co] = w[co, a, b, ci]
        assert np.array_equal(wd, want) and np.array_equal(R.pack_dgrad(wd), w)


# ----------------------------------------------------------------------------------------------------------------- bounds
def test_amax_and_bn_bound():
    assert R.amax(np.array([1.0, -3.0, np.nan, 2.0], dtype=np.float32)) == 3.0
    assert R.amax(np.zeros(8, dtype=np.float32)) == 0 and R.f32_bits(R.amax(np.array([-0.0], dtype=np.float32)))[()] == 0
    assert R.amax(np.array([1.0, np.inf], dtype=np.float32)) == np.inf
    assert R.amax(np.array([np.nan], dtype=np.float32)) == 0
    assert R.bn_bound([1.0, -2.0, 0.5], [0.0, -0.25, 9.0], 4.0) == 11.0


# --------------------------------------------------------------------------------------------------------- designed values
@pytest.mark.parametrize('bound', [1.0, float(np.float32(2.0 - 2.0 ** -23)) * 2.0 ** -3, 2.0 ** -20, 64.0])
def test_designed_values_contain_every_class(bound):
    x = R.designed_values(rng(9), 1 << 16, bound)
    c = R.classify(x, bound)
    per = (x.size - 1) // (2 * len(R.CLASSES) + 1)
    for k in ('bf16_tie_even', 'bf16_tie_odd', 'f16_tie_lo', 'lo_subnormal', 'hi_subnormal', 'f32_subnormal'):
        assert c[k] >= per, (k, c)
    assert c['f16_tie_hi'] >= per and min(c['f16_tie_hi_even_down'], c['f16_tie_hi_even_up']) >= per // 4, c
    assert c['f16_tie_sub'] >= per // 2 and c['vanish'] >= per and c['vanish_tie'] >= per // 3 and c['smallest_survivor'] >= per // 4, c
    assert min(c['zero_pos'], c['zero_neg']) >= per // 4, c
    assert c['log_uniform_binades'] >= 40 and c['bound_at_last'] == 1 and c['bound_pow2'] + c['bound_near2'] == 1, c
    assert float(np.abs(x).max()) == float(np.float32(bound)) and np.isfinite(x).all()
    h1, _, v = R.f16x2(x, bound)
    assert 2.0 ** 13 <= abs(float(v[-1])) < 2.0 ** 14 and np.isfinite(h1.astype(np.float32)).all()
    if c['bound_near2']:
        assert float(v[-1]) == 2.0 ** 14 - 2.0 ** -10                        # just under 2^14; plane 0 rounds it to 2^14


def test_designed_values_at_the_smallest_sizes():
    for n in (4, 8, 1028):
        x = R.designed_values(rng(10), n, 1.0)
        assert x.shape == (n,) and x[-1] == 1.0 and R.amax(x) == 1.0
    # every class meets every lane of a float4 and both halves of a packed pair
    m = (1 << 16) - 1
    cls = np.arange(m) % (2 * len(R.CLASSES) + 1)
    for k in range(len(R.CLASSES)):
        assert set((np.nonzero(cls == k)[0] % 4).tolist()) == {0, 1, 2, 3}


# ------------------------------------------------------------------------ the GPU test's comparison, fed four wrong kernels
def _f16_planes_with(cvt, x, bound):
    v = x * np.float32(R.pow2_scale(np.float32(bound)))
    h1 = cvt(v)
    return h1, cvt(v - h1.astype(np.float32))


def _truncate16(v):
    h = v.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(v)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float16)


def _flush16(v):
    h = v.astype(np.float16)
    return np.where(np.abs(h) < np.float16(2.0 ** -14), np.copysign(np.float16(0), h), h).astype(np.float16)


BOUND = float(np.float32(2.0 - 2.0 ** -23)) * 0.125


def test_comparison_passes_the_right_answer_and_reports_the_first_difference():
    x = R.designed_values(rng(11), 4 * 9216, BOUND)
    h1, h2, _ = R.f16x2(x, BOUND)
    want = R.expected_planes([h1, h2], x.size + 16)
    R.same_bits('same', want.copy(), want)
    got = want.copy()
    got[77] ^= 1
    with pytest.raises(AssertionError, match=r'1 of \d+ elements differ, first at \[77\]'):
        R.same_bits('one bit', got, want)
    R.same_bits('skipped', got, want, skip=[77])
    # the gap between the planes and the guard cells are part of what is compared
    for at in (x.size, x.size + 15, want.size - 1, want.size - R.GUARD):
        got = want.copy()
        got[at] = 0
        with pytest.raises(AssertionError):
            R.same_bits('sentinel', got, want)


@pytest.mark.parametrize('wrong', ['truncation', 'flushed fp16 subnormals'])
def test_comparison_catches_a_wrong_fp16_rounding(wrong):
    x = R.designed_values(rng(12), 1028, BOUND)
    want = R.expected_planes(list(R.f16x2(x, BOUND)[:2]), x.size)
    got = R.expected_planes(list(_f16_planes_with(_truncate16 if wrong == 'truncation' else _flush16, x, BOUND)), x.size)
    with pytest.raises(AssertionError, match='differ'):
        R.same_bits(wrong, got, want)
    # ... in each plane on its own
    for k in (0, 1):
        with pytest.raises(AssertionError, match='differ'):
            R.same_bits(wrong, got[k * x.size:(k + 1) * x.size], want[k * x.size:(k + 1) * x.size])


def test_comparison_catches_truncation_in_the_bf16_planes():
    x = R.restrict_exact(R.designed_values(rng(13), 1028, BOUND), BOUND / 3)
    want = R.expected_planes(list(R.bf16x3(x)), x.size + 8)
    chopped = R._bf16x3(x, lambda a: (R.f32_bits(a) >> 16).astype(np.uint16))
    got = R.expected_planes(list(chopped), x.size + 8)
    assert np.array_equal(_sum3(chopped), x.astype(np.float64))               # the sum is still exact: only the bits tell
    with pytest.raises(AssertionError, match='differ'):
        R.same_bits('bf16 truncation', got, want)


def test_comparison_catches_two_swapped_stream_indices():
    Cout, Cin = 48, 32
    x = R.designed_values(rng(14), Cout * 9 * Cin, BOUND)
    h1, h2, _ = R.f16x2(x, BOUND)
    want = R.expected_planes([R.stream_order(R.bits16(h), Cout, Cin) for h in (h1, h2)], x.size)
    swapped = [np.ascontiguousarray(R.bits16(h).reshape(Cout, 9, Cin // 16, 16).transpose(2, 0, 1, 3)).ravel() for h in (h1, h2)]
    with pytest.raises(AssertionError, match='differ'):
        R.same_bits('tap and Cout swapped', R.expected_planes(swapped, x.size), want)
    with pytest.raises(AssertionError, match='differ'):
        R.same_bits('plain order', R.expected_planes([h1, h2], x.size), want)


@pytest.mark.parametrize('n4', [1025, 3 * 1024 + 5, 9216 + 7, 11520])
def test_comparison_catches_a_dropped_last_partial_pass(n4):
    """A row whose last (partial) pass of 1024 float4 groups is not written keeps the sentinel there."""
    x = R.designed_values(rng(15), 4 * n4, BOUND)
    want = R.expected_planes(list(R.f16x2(x, BOUND)[:2]), x.size + 12)
    got = want.copy()
    done = (n4 - 1) // 1024 * 1024 * 4
    for k in (0, 1):
        got[k * (x.size + 12) + done:k * (x.size + 12) + x.size] = R.SENT16
    with pytest.raises(AssertionError, match='differ'):
        R.same_bits('last pass dropped', got, want)
    # even one missing float4 group — the last
    got = want.copy()
    got[x.size - 4:x.size] = R.SENT16
    with pytest.raises(AssertionError, match=r'4 of'):
        R.same_bits('last group dropped', got, want)
