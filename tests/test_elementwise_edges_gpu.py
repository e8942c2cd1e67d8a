"""The element-wise HIP kernels (csrc/bn.hip, resample.hip, flat.hip, optim.hip, ew_bodies.h) against tests/ew_ref.py (numpy
fp64), through the C ABI, at the sizes and inputs where the rest of the suite does not go: past one grid stride of the flat launches (a),
all three code paths of the BatchNorm backward apply (b), every thread mapping of the tile reductions (c), pools on
tied, NaN and -inf windows (d), the optimisers and the non-finite guard element by element (e).

Bars.  Where a kernel selects or copies (pools, masks, skipped elements, fill, layout, fused vs plain) the result must be
EQUAL — compared as bits where a -0.0 or a NaN can occur.  Where it computes, the bar is the a-priori fp32 rounding bound of
its expression against the fp64 value of the same fp32 inputs, element by element: gamma(k) * (sum of the absolute values of
the terms), k the rounded operations, stated where each bar is formed (ew_ref.py returns them).  build.py compiles
these units with `-O3 -fno-slp-vectorize` and no fast-math flag; for HIP the compiler's default is correctly rounded fp32
division and sqrtf (-fhip-fp32-correctly-rounded-divide-sqrt), so neither adds to k; fp contraction (the default) only
removes roundings.  tests/test_ew_ref_cpu.py shows that torch's own fp32 CPU kernels meet the same bars, so none is
widened.  No bar comes from a kernel's output.

Sizes.  flat_grid() caps a flat launch at 4096 x 256 threads, so W work items need 2 * 2^20 < W < 3 * 2^20 for a second
and (part of the threads) a third trip; W is never a multiple of 256 (ragged last workgroup).  A float4 item is four
floats and a pool window four of those, so the pools' inputs are the largest tensors here (35 M floats)."""

import numpy as np
import pytest
import torch

import ew_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TRIP = 256 * 4096                      # work items of one grid stride
N_SCALAR = 2621443                     # scalar kernels: 2.5 strides + 3
NB, HO, WO, CF = 5, 165, 167, 64       # float4 kernels: 5 * 165 * 167 * 16 = 2 204 400 items (2.1 strides), Ho != Wo
SENT = -777.0


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(DEV)


def host(t):
    return t.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def call(name, *args):
    from dsnt._lib import call as c, ptr
    c(name, *[ptr(a) if isinstance(a, torch.Tensor) else a for a in args])


def _premise_items(W):
    """More than two grid strides, fewer than three, ragged — and the launch capped."""
    assert 2 * TRIP < W < 3 * TRIP and W % 256 != 0 and R.flat_grid(W) == 4096


def _within(got, want, bound, skip=None):
    err = np.abs(got.astype(np.float64) - want)
    bad = err > bound
    if skip is not None:
        bad &= ~skip
    assert not bad.any(), 'first at %s: err %.3e bound %.3e (%d elements)' % (
        np.argwhere(bad)[0], err[bad].flat[0], np.asarray(bound)[bad].flat[0] if np.ndim(bound) else bound, bad.sum())


# ================================================================ a. second trip of every flat loop
def test_second_trip_bn_forward_and_relu_backward():
    """dsnt_bn_act_fwd, dsnt_bn_add_act_fwd, dsnt_relu_bwd, n4 = 137 775 * 16 = 2 204 400.  y = fma(x, scale, shift): one
    rounding, bar gamma(1) (|x scale| + |shift|); + res: gamma(2) (... + |res|); the ReLU and relu_bwd select: relu_bwd exact."""
    M, Cc = NB * HO * WO, CF
    _premise_items(M * Cc // 4)
    r = np.random.default_rng(21)
    x, res = r.standard_normal((M, Cc)).astype(np.float32), r.standard_normal((M, Cc)).astype(np.float32)
    sc, sh = (r.uniform(0.5, 1.5, Cc)).astype(np.float32), (r.standard_normal(Cc) * 0.3).astype(np.float32)
    xd, rd, scd, shd = dev(x), dev(res), dev(sc), dev(sh)
    x64 = x.astype(np.float64)
    lin, mag = x64 * sc + sh, np.abs(x64 * sc) + np.abs(sh)
    for relu in (0, 1):
        y = torch.full((M, Cc), SENT, device=DEV)
        call('dsnt_bn_act_fwd', xd, scd, shd, relu, y, M, Cc)
        _within(host(y), np.maximum(lin, 0) if relu else lin, R.gamma(1) * mag)
        y2 = torch.full((M, Cc), SENT, device=DEV)
        call('dsnt_bn_add_act_fwd', xd, scd, shd, rd, relu, y2, M, Cc)
        _within(host(y2), np.maximum(lin + res, 0) if relu else lin + res, R.gamma(2) * (mag + np.abs(res)))
    yh = host(y2)                                     # relu output of the block tail: exact zeros where dead
    dz = torch.full((M, Cc), SENT, device=DEV)
    call('dsnt_relu_bwd', rd, y2, dz, M * Cc)
    assert np.array_equal(bits(host(dz)), bits(np.where(yh > 0, res, np.float32(0))))


def test_second_trip_maxpool2():
    """dsnt_maxpool2_fwd / _bwd / _bwd_add / _bwd_amax over 5 x 165 x 167 x 16 = 2 204 400 windows: values, index bytes and
    routed (integer) gradients exact, accumulate 0 and 1; the amax slots hold max |dx| exactly."""
    N, H, W, Cc = NB, 2 * HO, 2 * WO, CF
    _premise_items(N * HO * WO * Cc // 4)
    x = np.random.default_rng(22).standard_normal((N, H, W, Cc)).astype(np.float32)
    y_ref, k_ref = R.maxpool2(x)
    xd = dev(x)
    y = torch.full((N, HO, WO, Cc), SENT, device=DEV)
    idx = torch.full((N, HO, WO, Cc), 9, dtype=torch.uint8, device=DEV)
    call('dsnt_maxpool2_fwd', xd, y, idx, N, H, W, Cc)
    assert np.array_equal(host(y), y_ref) and np.array_equal(host(idx), k_ref)
    del xd
    gy = R.int_grad(y_ref.shape, 23)
    dx_ref = R.maxpool2_bwd(gy, k_ref, np.float32)
    gyd = dev(gy)
    dx = torch.full((N, H, W, Cc), SENT, device=DEV)
    call('dsnt_maxpool2_bwd', gyd, idx, dx, 0, N, H, W, Cc)
    assert np.array_equal(host(dx), dx_ref)
    am = torch.zeros(64, device=DEV)
    call('dsnt_maxpool2_bwd_amax', gyd, idx, dx, 1, N, H, W, Cc, am)
    assert np.array_equal(host(dx), 2 * dx_ref) and am.max().item() == 6.0 == float(np.abs(2 * dx_ref).max())
    extra = R.int_grad(x.shape, 24)
    ed = dev(extra)
    am.zero_()
    call('dsnt_maxpool2_bwd_add', gyd, idx, dx, 1, ed, N, H, W, Cc, am)
    want = 3 * dx_ref + extra
    assert np.array_equal(host(dx), want) and am.max().item() == float(np.abs(want).max())
    call('dsnt_maxpool2_bwd_add', gyd, idx, dx, 0, ed, N, H, W, Cc, None)
    assert np.array_equal(host(dx), dx_ref + extra)


def test_second_trip_upsample2():
    """dsnt_upsample2_add_fwd over 5 x 162 x 170 x 16 = 2 203 200 items: one addition of two fp32 values, correctly rounded
    by IEEE — exact against the fp64 sum rounded to fp32.  dsnt_upsample2_bwd / _amax over 5 x 165 x 167 x 16 low pixels:
    (v0 + v1) + (v2 + v3) (+ old): integer inputs, exact, accumulate 0 and 1; amax == max |dlow|."""
    N, H, W, Cc = NB, 162, 170, CF
    _premise_items(N * H * W * Cc // 4)
    r = np.random.default_rng(25)
    up, low = r.standard_normal((N, H, W, Cc)).astype(np.float32), r.standard_normal((N, H // 2, W // 2, Cc)).astype(np.float32)
    out = torch.full((N, H, W, Cc), SENT, device=DEV)
    call('dsnt_upsample2_add_fwd', dev(up), dev(low), out, N, H, W, Cc)
    want = (up.astype(np.float64) + np.repeat(np.repeat(low, 2, 1), 2, 2)).astype(np.float32)
    assert np.array_equal(host(out), want)
    del out
    H, W = 2 * HO, 2 * WO
    go = R.int_grad((N, H, W, Cc), 26)
    want = go[:, 0::2, 0::2] + go[:, 0::2, 1::2] + go[:, 1::2, 0::2] + go[:, 1::2, 1::2]
    god = dev(go)
    dl = torch.full((N, HO, WO, Cc), SENT, device=DEV)
    call('dsnt_upsample2_bwd', god, dl, 0, N, H, W, Cc)
    assert np.array_equal(host(dl), want)
    am = torch.zeros(64, device=DEV)
    call('dsnt_upsample2_bwd_amax', god, dl, 1, N, H, W, Cc, am)
    assert np.array_equal(host(dl), 2 * want) and am.max().item() == float(np.abs(2 * want).max())


def test_second_trip_maxpool3s2():
    """dsnt_maxpool3s2_fwd over 5 x 165 x 167 x 16 windows of a 329 x 334 image (H odd, W even: the last window row has its
    bottom taps valid, the last column not), dsnt_maxpool3s2_bwd over the 5 x 329 x 334 x 16 input items (nine trips):
    exact, accumulate 0 and 1."""
    N, H, W, Cc = NB, 2 * HO - 1, 2 * WO, CF
    _premise_items(N * HO * WO * Cc // 4)
    x = np.random.default_rng(27).standard_normal((N, H, W, Cc)).astype(np.float32)
    y_ref, k_ref = R.maxpool3s2(x)
    assert y_ref.shape == (N, HO, WO, Cc)
    y = torch.full((N, HO, WO, Cc), SENT, device=DEV)
    idx = torch.full((N, HO, WO, Cc), 99, dtype=torch.uint8, device=DEV)
    call('dsnt_maxpool3s2_fwd', dev(x), y, idx, N, H, W, Cc)
    assert np.array_equal(host(y), y_ref) and np.array_equal(host(idx), k_ref)
    gy = R.int_grad(y_ref.shape, 28)
    dx_ref = R.maxpool3s2_bwd(gy, k_ref, H, W, np.float32)
    gyd = dev(gy)
    dx = torch.full((N, H, W, Cc), SENT, device=DEV)
    call('dsnt_maxpool3s2_bwd', gyd, idx, dx, 0, N, H, W, Cc)
    assert np.array_equal(host(dx), dx_ref)
    call('dsnt_maxpool3s2_bwd', gyd, idx, dx, 1, N, H, W, Cc)
    assert np.array_equal(host(dx), 2 * dx_ref)


def test_second_trip_axpy_fill_layout():
    """dsnt_axpy / _amax loop over float4 items with a scalar tail: n = 4 * 2 204 400 + 3 (the issue's scalar n would leave
    its float4 loop at one trip).  y = a x (+ y): bar gamma(1) |a x| resp. gamma(2) (|a x| + |y|); amax == max |y| exactly.
    dsnt_fill_zero (n = 2 621 443) and the two layout kernels (N * HW = 5 * 440 881 pixels, C = 3 padded to 4) are exact."""
    n = 4 * NB * HO * WO * CF // 4 + 3
    _premise_items(n // 4)
    r = np.random.default_rng(29)
    x, y0 = r.standard_normal(n).astype(np.float32), r.standard_normal(n).astype(np.float32)
    a = float(np.float32(0.37))
    xd = dev(x)
    y = torch.full((n,), SENT, device=DEV)
    call('dsnt_axpy', xd, y, a, 0, n)
    _within(host(y), a * x.astype(np.float64), R.gamma(1) * np.abs(a * x.astype(np.float64)))
    y, am = dev(y0), torch.zeros(64, device=DEV)
    call('dsnt_axpy_amax', xd, y, a, 1, n, am)
    _within(host(y), a * x.astype(np.float64) + y0, R.gamma(2) * (np.abs(a * x.astype(np.float64)) + np.abs(y0)))
    assert am.max().item() == y.abs().max().item()

    _premise_items(N_SCALAR)
    buf = torch.full((N_SCALAR + 8,), SENT, device=DEV)
    call('dsnt_fill_zero', buf, N_SCALAR)
    assert (buf[:N_SCALAR] == 0).all().item() and (buf[N_SCALAR:] == SENT).all().item()

    N, Cs, HW, Cpad = 5, 3, 440881, 4
    _premise_items(N * HW)
    src = r.standard_normal((N, Cs, HW)).astype(np.float32)
    dst = torch.full((N, HW, Cpad), SENT, device=DEV)
    call('dsnt_nchw_to_nhwc', dev(src), dst, N, Cs, HW, Cpad)
    want = np.zeros((N, HW, Cpad), np.float32)
    want[:, :, :Cs] = np.transpose(src, (0, 2, 1))
    assert np.array_equal(host(dst), want)
    back = torch.full((N, Cs, HW), SENT, device=DEV)
    call('dsnt_nhwc_to_nchw', dst, back, N, Cs, HW, Cpad)
    assert np.array_equal(host(back), src)


# ================================================================ b. bn_act_bwd_apply: all three code paths
def _apply_inputs(M, Cc):
    x, gamma, beta, da = R.bn_case(M, Cc, seed=M + Cc)
    mu, is_, sc, sh = R.bn_vectors(x, gamma, beta)
    r = np.random.default_rng(M)
    coef = (r.standard_normal((2, Cc)) * 0.05).astype(np.float32)
    third = r.standard_normal((M, Cc)).astype(np.float32)
    return x, da, mu, is_, sc, sh, coef, third


def _check_apply(M, Cc, launch, coef_dev=None):
    """relu 0 / 1 x base absent / dx itself / a third tensor.  `launch(d, relu, mode, dx, am)` runs the entry point; `coef_dev`:
    the coefficients it will use when they are not the synthetic ones.  Bar: gamma(6) |scale| (|dz| + |c0| + |xhat c1|) — sub,
    mul, mul, sub, sub, mul — and gamma(7) (... + |base|) with a base; elements whose ReLU mask is undecidable (at most 0.1 %)
    are left out.  amax must be max |dx| exactly, and a third-tensor base stays intact."""
    x, da, mu, is_, sc, sh, coef, third = _apply_inputs(M, Cc)
    if coef_dev is not None:
        coef = host(coef_dev)
    d = {k: dev(v) for k, v in dict(x=x, da=da, mu=mu, is_=is_, sc=sc, sh=sh, coef=coef, third=third).items()}
    for relu in (0, 1):
        want0, und, bound0 = R.bn_apply(da, x, sc, sh, mu, is_, coef, relu)        # the fp64 reference, once per relu
        assert und.mean() <= 1e-3
        want1, bound1 = want0 + third, R.gamma(7) * (bound0 / R.gamma(6) + np.abs(third))
        for mode in ('none', 'self', 'third'):
            dx = dev(third) if mode == 'self' else torch.full((M, Cc), SENT, device=DEV)
            am = torch.zeros(64, device=DEV)
            launch(d, relu, mode, dx, am)
            _within(host(dx), want0 if mode == 'none' else want1, bound0 if mode == 'none' else bound1, skip=und)
            assert am.max().item() == dx.abs().max().item()
            assert np.array_equal(host(d['third']), third)


def _plain_launch(M, Cc):
    def launch(d, relu, mode, dx, am):
        if mode == 'third':
            call('dsnt_bn_act_bwd_apply_base', d['da'], d['x'], d['sc'], d['sh'], d['mu'], d['is_'], d['coef'], relu, d['third'], dx, M, Cc, am)
        else:
            call('dsnt_bn_act_bwd_apply_amax', d['da'], d['x'], d['sc'], d['sh'], d['mu'], d['is_'], d['coef'], relu, dx,
                 1 if mode == 'self' else 0, M, Cc, am)
    return launch


def test_apply_fixed_two_in_flight_loop_and_tail():
    """FIXED kernel, C = 64 (C4 = 16 divides every stride): n4 = 2.5 * 2^20 + 16 (M = 163 841), the smallest shape at which
    the two-in-flight loop runs (once, for every thread) AND its `if (i < n4)` tail runs for part of the threads
    (i < n4 - 2^21 = 524 304)."""
    M, Cc = 163841, 64
    n4 = M * Cc // 4
    assert n4 == 5 * TRIP // 2 + 16 and R.apply_is_fixed(M, Cc) == (True, 4096)
    assert TRIP < n4 - TRIP and 0 < n4 - 2 * TRIP < TRIP
    _check_apply(M, Cc, _plain_launch(M, Cc))


@pytest.mark.parametrize('M,Cc', [(350, 48), (100003, 48), (350, 80), (60003, 80)])
def test_apply_generic_kernel(M, Cc):
    """bn_act_bwd_apply_kernel<false>: picked when grid * 256 is no multiple of C / 4.  C = 48 (C4 = 12) needs a grid that is
    no multiple of 3, C = 80 (C4 = 20) none of 5: M = 350 gives grids of 17 and 28 workgroups (one trip, ragged), the large
    M the capped grid of 4096 (4096 % 3 = 4096 % 5 = 1) with n4 > 2^20, so the loop takes a second trip with another i % C4."""
    fixed, grid = R.apply_is_fixed(M, Cc)
    assert not fixed and (grid * 256) % (Cc // 4) != 0 and grid % (3 if Cc == 48 else 5) != 0
    assert (M * Cc // 4 > TRIP) == (M > 50000) and (grid == 4096) == (M > 50000)
    _check_apply(M, Cc, _plain_launch(M, Cc))


@pytest.mark.parametrize('accp', [0, 1])
def test_apply_pro_two_in_flight_at_the_capped_grid(accp):
    """dsnt_bn_act_bwd_apply_pro / _pro_base cap the grid at 128 workgroups (stride 32 768): C = 128, n4 = 2.5 * 32 768 + 32
    (M = 2561, 21 tiles: within C <= 256, ntiles * C <= 16384) runs the two-in-flight loop once and the tail for part of the
    threads.  coef, dgamma, dbeta == the stand-alone dsnt_bn_bwd_finalize bit for bit (accumulate_params 0 and 1); dx against
    ew_ref with the coef the prologue left."""
    M, Cc = 2561, 128
    n4, tiles = M * Cc // 4, (M + 127) // 128
    assert n4 == 5 * 32768 // 2 + Cc // 4 and R.apply_is_fixed(M, Cc, pro=True) == (True, 128) and tiles * Cc <= 16384
    x, da, mu, is_, sc, sh, _, _ = _apply_inputs(M, Cc)
    part = torch.empty(tiles, 2, Cc, device=DEV)
    call('dsnt_bn_act_bwd_reduce', dev(da), dev(x), dev(sc), dev(sh), dev(mu), dev(is_), 1, part, M, Cc)
    init_g, init_b = torch.full((Cc,), 0.25, device=DEV), torch.full((Cc,), -0.5, device=DEV)
    dg_ref, db_ref, coef_ref = init_g.clone(), init_b.clone(), torch.empty(2, Cc, device=DEV)
    call('dsnt_bn_bwd_finalize', part, tiles, M, Cc, dg_ref, db_ref, accp, coef_ref)

    def launch(d, relu, mode, dx, am):
        dg, db, coef = init_g.clone(), init_b.clone(), torch.full((2, Cc), SENT, device=DEV)
        if mode == 'third':
            call('dsnt_bn_act_bwd_apply_pro_base', d['da'], d['x'], d['sc'], d['sh'], d['mu'], d['is_'], part, tiles, dg, db, accp, coef,
                 relu, d['third'], dx, M, Cc, am)
        else:
            call('dsnt_bn_act_bwd_apply_pro', d['da'], d['x'], d['sc'], d['sh'], d['mu'], d['is_'], part, tiles, dg, db, accp, coef,
                 relu, dx, 1 if mode == 'self' else 0, M, Cc, am)
        assert torch.equal(coef, coef_ref) and torch.equal(dg, dg_ref) and torch.equal(db, db_ref)
    _check_apply(M, Cc, launch, coef_ref)


# ================================================================ c. tile reductions in every mapping
TILE_CASES = [
    (32768 + 37, 128),      # tiles >= 256: cgs = C4 = 32, rpar = 8
    (32768 + 37, 64),       # tiles >= 256: cgs = C4 = 16, rpar = 16
    (300, 80),              # cgs = 20: rpar = 12, 16 idle threads that must stay out of red[]
    (300, 96),              # C4 = 24 > 16, no multiple of 16: cgs = 24, rpar = 10, 16 idle threads
    (1000, 192),            # C4 = 48: the 16-lane mapping with gridDim.y = 3
    (200, 1032),            # C4 = 258: two cg0 passes of 256 lanes, the second masked to 2
    (129, 8),               # a one-row last tile, cgs = 2
    (1, 4),                 # one row in all, cgs = 1, rpar = 256
]
TILE_PREMISE = {(32805, 128): (32, 1, 8), (32805, 64): (16, 1, 16), (300, 80): (20, 1, 12), (300, 96): (24, 1, 10), (1000, 192): (16, 3, 16),
                (200, 1032): (256, 1, 1), (129, 8): (2, 1, 128), (1, 4): (1, 1, 256)}


def _tile_premise(M, Cc):
    tiles = (M + 127) // 128
    cgs = R.tile_cgs(tiles, Cc // 4)
    assert (cgs, R.tile_grid_y(tiles, Cc // 4), 256 // cgs) == TILE_PREMISE[(M, Cc)]
    assert (tiles >= 256) == (M > 32768)
    return tiles


def _check_sums(part, s1, s2, a1, a2, n1, n2, slack1=0.0, slack2=0.0):
    got = host(part).astype(np.float64)
    _within(got[:, 0], s1, R.gamma(n1) * a1 + slack1)
    _within(got[:, 1], s2, R.gamma(n2) * a2 + slack2)


@pytest.mark.parametrize('M,Cc', TILE_CASES)
def test_tile_reductions(M, Cc):
    """dsnt_bn_stats, dsnt_bn_act_bwd_reduce (relu 0, 1), dsnt_bn_add_act_bwd_reduce (relu 0, 1) per tile and channel against
    ew_ref.  Bar: the recursive-summation bound gamma(n) * sum |term|, n = rows one lane walks + rpar lane partials + 1 for the
    fma (tile_sum_ops); the second backward sum has two more operations (xhat = (x - mean) * invstd is rounded twice before
    the fma).  Terms of elements whose ReLU mask is undecidable may be in or out: their |term| is added to the bar."""
    tiles = _tile_premise(M, Cc)
    x, gamma, beta, da = R.bn_case(M, Cc, seed=M + Cc)
    mu, is_, sc, sh = R.bn_vectors(x, gamma, beta)
    n = R.tile_sum_ops(M, Cc)
    xd, dad, mud, isd, scd, shd = (dev(v) for v in (x, da, mu, is_, sc, sh))
    part = torch.full((tiles, 2, Cc), SENT, device=DEV)
    call('dsnt_bn_stats', xd, part, M, Cc)
    _check_sums(part, *R.tile_sums(x, M, C=Cc), n, n)
    dead, und = R.relu_mask(x, sc, sh)
    xh = (x.astype(np.float64) - mu) * is_.astype(np.float64)
    for relu in (0, 1):
        dz = np.where(dead, 0.0, da) if relu else da.astype(np.float64)
        sl1, sl2 = (R.tile_sums_of(np.where(und, np.abs(da), 0.0), np.where(und, np.abs(da * xh), 0.0), M, Cc)[:2] if relu else (0.0, 0.0))
        part.fill_(SENT)
        call('dsnt_bn_act_bwd_reduce', dad, xd, scd, shd, mud, isd, relu, part, M, Cc)
        _check_sums(part, *R.bn_bwd_tile_sums(dz, x, mu, is_, M, Cc), n, n + 2, sl1, sl2)
    # the block tail: the mask comes from the stored output y (> 0), dz is written
    y = np.maximum(np.random.default_rng(M).standard_normal((M, Cc)), 0).astype(np.float32)
    yd = dev(y)
    for relu in (0, 1):
        dz_ref = np.where(y > 0, da, np.float32(0)) if relu else da
        part.fill_(SENT)
        dzd = torch.full((M, Cc), SENT, device=DEV)
        call('dsnt_bn_add_act_bwd_reduce', dad, yd, xd, mud, isd, relu, dzd, part, M, Cc)
        assert np.array_equal(bits(host(dzd)), bits(dz_ref))
        _check_sums(part, *R.bn_bwd_tile_sums(dz_ref, x, mu, is_, M, Cc), n, n + 2)


def _factor_pool(M):
    """N, Ho, Wo with N * Ho * Wo == M: a batch of 5, 3 or 2 where M has the factor, the rest as square as it goes."""
    nb = next((b for b in (5, 3, 2) if M % b == 0 and M > b), 1)
    r = M // nb
    ho = max(d_ for d_ in range(1, int(r ** 0.5) + 1) if r % d_ == 0)
    return nb, ho, r // ho


@pytest.mark.parametrize('M,Cc', TILE_CASES)
def test_fused_producers_equal_bn_stats(M, Cc):
    """dsnt_maxpool2_fwd_stats, dsnt_upsample2_add_fwd_stats, dsnt_bn_act_fwd_stats: stored output == the plain kernel's and
    tile sums == dsnt_bn_stats over it, bit for bit, in every mapping.  (The up-sampled output needs even H and W: its M is
    the next multiple of 8 with H = 4 — the same tiles and mapping but for the last tile's rows.)"""
    tiles = _tile_premise(M, Cc)
    r = np.random.default_rng(M * 7 + Cc)

    def stats_of(t, rows):
        want = torch.full(((rows + 127) // 128, 2, Cc), SENT, device=DEV)
        call('dsnt_bn_stats', t, want, rows, Cc)
        return want
    N, Ho, Wo = _factor_pool(M)
    assert N * Ho * Wo == M
    xd = dev(r.standard_normal((N, 2 * Ho, 2 * Wo, Cc)).astype(np.float32))
    y, y2 = torch.full((N, Ho, Wo, Cc), SENT, device=DEV), torch.full((N, Ho, Wo, Cc), SENT, device=DEV)
    k, k2 = (torch.full((N, Ho, Wo, Cc), 9, dtype=torch.uint8, device=DEV) for _ in range(2))
    part = torch.full((tiles, 2, Cc), SENT, device=DEV)
    call('dsnt_maxpool2_fwd', xd, y, k, N, 2 * Ho, 2 * Wo, Cc)
    call('dsnt_maxpool2_fwd_stats', xd, y2, k2, part, N, 2 * Ho, 2 * Wo, Cc, None)
    assert torch.equal(y, y2) and torch.equal(k, k2) and torch.equal(part, stats_of(y, M))

    Mu = (M + 7) // 8 * 8
    H, W = 4, Mu // 4
    assert ((Mu + 127) // 128 >= 256) == (tiles >= 256) and R.tile_cgs((Mu + 127) // 128, Cc // 4) == R.tile_cgs(tiles, Cc // 4)
    upd, lowd = dev(r.standard_normal((1, H, W, Cc)).astype(np.float32)), dev(r.standard_normal((1, H // 2, W // 2, Cc)).astype(np.float32))
    o, o2 = torch.full((1, H, W, Cc), SENT, device=DEV), torch.full((1, H, W, Cc), SENT, device=DEV)
    part = torch.full(((Mu + 127) // 128, 2, Cc), SENT, device=DEV)
    call('dsnt_upsample2_add_fwd', upd, lowd, o, 1, H, W, Cc)
    call('dsnt_upsample2_add_fwd_stats', upd, lowd, o2, part, 1, H, W, Cc, None)
    assert torch.equal(o, o2) and torch.equal(part, stats_of(o, Mu))

    x2 = dev(r.standard_normal((M, Cc)).astype(np.float32))
    sc, sh = dev(r.uniform(0.5, 1.5, Cc).astype(np.float32)), dev((r.standard_normal(Cc) * 0.3).astype(np.float32))
    for relu in (0, 1):
        z, z2 = torch.full((M, Cc), SENT, device=DEV), torch.full((M, Cc), SENT, device=DEV)
        part = torch.full((tiles, 2, Cc), SENT, device=DEV)
        call('dsnt_bn_act_fwd', x2, sc, sh, relu, z, M, Cc)
        call('dsnt_bn_act_fwd_stats', x2, sc, sh, relu, z2, part, M, Cc, None)
        assert torch.equal(z, z2) and torch.equal(part, stats_of(z, M))


# ================================================================ d. pools on ties
def _tie_case(pool, H, W, nan_tap):
    N, Cc = 3, 8
    x = R.tie_input(N, H, W, Cc, seed=H * 100 + W, pool=pool, nan_tap=nan_tap)
    clean = R.tie_input(N, H, W, Cc, seed=H * 100 + W, pool=pool, nan_tap=None)
    share = R.tie_share(clean, pool)
    assert share >= 1.0 / 3.0, share          # 12x20: 0.46 of the 2x2 windows; 3x3: 0.44 .. 0.5 hold their maximum more than once
    return N, Cc, x


@pytest.mark.parametrize('nan_tap', [None, 0, 1, 2, 3])
def test_maxpool2_on_ties(nan_tap):
    """dsnt_maxpool2_fwd and dsnt_maxpool2_fwd_stats on relu(round(4 x) / 4) with the planted windows of ew_ref.tie_input
    (all equal, only maximum at the last tap, -0.0 beside +0.0, all -inf, one NaN at tap `nan_tap`): value BITS and index
    bytes == ew_ref, the two forwards equal to each other byte for byte; backwards with integer gy exact, accumulate 0 / 1
    and dsnt_maxpool2_bwd_add.  A `>=` for the `>` moves the arg-max of every tied window to its last maximum."""
    H, W = 12, 20
    N, Cc, x = _tie_case(2, H, W, nan_tap)
    y_ref, k_ref = R.maxpool2(x)
    xd = dev(x)
    Ho, Wo = H // 2, W // 2
    y, y2 = (torch.full((N, Ho, Wo, Cc), SENT, device=DEV) for _ in range(2))
    k, k2 = (torch.full((N, Ho, Wo, Cc), 9, dtype=torch.uint8, device=DEV) for _ in range(2))
    part = torch.empty((N * Ho * Wo + 127) // 128, 2, Cc, device=DEV)
    call('dsnt_maxpool2_fwd', xd, y, k, N, H, W, Cc)
    call('dsnt_maxpool2_fwd_stats', xd, y2, k2, part, N, H, W, Cc, None)
    assert np.array_equal(bits(host(y)), bits(y_ref)) and np.array_equal(host(k), k_ref)
    assert np.array_equal(bits(host(y2)), bits(host(y))) and torch.equal(k2, k)
    gy = R.int_grad(y_ref.shape, 31)
    dx_ref = R.maxpool2_bwd(gy, k_ref, np.float32)
    gyd, dx = dev(gy), torch.full((N, H, W, Cc), SENT, device=DEV)
    call('dsnt_maxpool2_bwd', gyd, k, dx, 0, N, H, W, Cc)
    assert np.array_equal(host(dx), dx_ref)
    call('dsnt_maxpool2_bwd', gyd, k, dx, 1, N, H, W, Cc)
    assert np.array_equal(host(dx), 2 * dx_ref)
    extra = R.int_grad(x.shape, 32)
    call('dsnt_maxpool2_bwd_add', gyd, k, dx, 1, dev(extra), N, H, W, Cc, None)
    assert np.array_equal(host(dx), 3 * dx_ref + extra)
    call('dsnt_maxpool2_bwd_add', gyd, k, dx, 0, dev(extra), N, H, W, Cc, None)
    assert np.array_equal(host(dx), dx_ref + extra)


@pytest.mark.parametrize('hw', [(1, 5), (7, 9), (16, 16)])
@pytest.mark.parametrize('nan_tap', [None, 0, 4, 8])
def test_maxpool3s2_on_ties(hw, nan_tap):
    """dsnt_maxpool3s2_fwd / _bwd on the same kind of input; (1, 5), (7, 9), (16, 16) give border windows of 2, 4 and 6
    valid taps (and 3: H = 1).  Value bits and index bytes == ew_ref; the gather backward with integer gy exact, accumulate
    0 and 1."""
    H, W = hw
    N, Cc, x = _tie_case(3, H, W, nan_tap)
    y_ref, k_ref = R.maxpool3s2(x)
    Ho, Wo = y_ref.shape[1:3]
    y = torch.full((N, Ho, Wo, Cc), SENT, device=DEV)
    k = torch.full((N, Ho, Wo, Cc), 99, dtype=torch.uint8, device=DEV)
    call('dsnt_maxpool3s2_fwd', dev(x), y, k, N, H, W, Cc)
    assert np.array_equal(bits(host(y)), bits(y_ref)) and np.array_equal(host(k), k_ref)
    gy = R.int_grad(y_ref.shape, 33)
    dx_ref = R.maxpool3s2_bwd(gy, k_ref, H, W, np.float32)
    gyd, dx = dev(gy), torch.full((N, H, W, Cc), SENT, device=DEV)
    call('dsnt_maxpool3s2_bwd', gyd, k, dx, 0, N, H, W, Cc)
    assert np.array_equal(host(dx), dx_ref)
    call('dsnt_maxpool3s2_bwd', gyd, k, dx, 1, N, H, W, Cc)
    assert np.array_equal(host(dx), 2 * dx_ref)


# ================================================================ e. optimisers and the guard
OPT_SETTINGS = [(0.0, 1.0), (1e-4, 1.0), (0.0, 1.0 / 3.0), (1e-4, 0.5)]          # (weight_decay, grad_scale)
_OPT = {}


def _opt_data():
    """Parameters and three gradients of n = 2 621 443 (2.5 grid strides + 3), made once and never changed."""
    if not _OPT:
        r = np.random.default_rng(41)
        _OPT['p'] = r.standard_normal(N_SCALAR).astype(np.float32)
        _OPT['g'] = [(r.standard_normal(N_SCALAR) * (0.1 + i)).astype(np.float32) for i in range(3)]
        for v in [_OPT['p']] + _OPT['g']:
            v.setflags(write=False)
    _premise_items(N_SCALAR)
    return _OPT['p'], _OPT['g']


def _rms(p, g, sq, wd, gs, flag=None):
    if flag is None:
        call('dsnt_rmsprop_step', p, g, sq, N_SCALAR, 2.5e-4, 0.99, 1e-8, wd, gs)
    else:
        call('dsnt_rmsprop_step_guarded', p, g, sq, N_SCALAR, 2.5e-4, 0.99, 1e-8, wd, gs, flag)


def _sgd(p, g, buf, mom, wd, gs, first, flag=None):
    if flag is None:
        call('dsnt_sgd_step', p, g, buf, N_SCALAR, 0.2, mom, wd, gs, first)
    else:
        call('dsnt_sgd_step_guarded', p, g, buf, N_SCALAR, 0.2, mom, wd, gs, first, flag)


@pytest.mark.parametrize('wd,gs', OPT_SETTINGS)
def test_rmsprop_three_steps(wd, gs):
    """dsnt_rmsprop_step: every step against ew_ref.rmsprop_step from the SAME fp32 state (the device's, read back before the
    step), every element: bars bound_sq = gamma(9) S and bound_p (ew_ref.rmsprop_step spells out the count).  The guarded form
    on finite gradients: bitwise the unguarded result, flag stays [0, 0]."""
    p0, grads = _opt_data()
    p, sq = dev(p0), torch.zeros(N_SCALAR, device=DEV)
    pg, sqg, flag = p.clone(), sq.clone(), torch.zeros(2, dtype=torch.int32, device=DEV)
    for g in grads:
        ph, sqh, gd = host(p), host(sq), dev(g)
        _rms(p, gd, sq, wd, gs)
        _rms(pg, gd, sqg, wd, gs, flag)
        out = R.rmsprop_step(ph, g, sqh, 2.5e-4, 0.99, 1e-8, wd, gs)
        _within(host(sq), out['sq'], out['bound_sq'])
        _within(host(p), out['p'], out['bound_p'])
        assert torch.equal(p, pg) and torch.equal(sq, sqg) and flag.tolist() == [0, 0]


@pytest.mark.parametrize('momentum', [0.9, 0.0])
@pytest.mark.parametrize('wd,gs', OPT_SETTINGS)
def test_sgd_three_steps(wd, gs, momentum):
    """dsnt_sgd_step, first_step 1 then 0, every step and element against ew_ref.sgd_step from the same fp32 state: bars
    bound_buf = gamma(4) B (scale, fma, product, sum) and bound_p = gamma(6) (|p| + lr B).  momentum 0: the buffer passed is
    sentinel-filled and must stay untouched.  Guarded on finite gradients == unguarded, bitwise; flag [0, 0]."""
    p0, grads = _opt_data()
    p = dev(p0)
    buf = torch.full((N_SCALAR,), SENT if momentum == 0 else 0.0, device=DEV)
    pg, bufg, flag = p.clone(), buf.clone(), torch.zeros(2, dtype=torch.int32, device=DEV)
    for i, g in enumerate(grads):
        ph, bh, gd = host(p), host(buf), dev(g)
        _sgd(p, gd, buf, momentum, wd, gs, 1 if i == 0 else 0)
        _sgd(pg, gd, bufg, momentum, wd, gs, 1 if i == 0 else 0, flag)
        out = R.sgd_step(ph, g, bh, 0.2, momentum, wd, gs, first_step=(i == 0))
        _within(host(p), out['p'], out['bound_p'])
        if momentum == 0:
            assert (buf == SENT).all().item()
        else:
            _within(host(buf), out['buf'], out['bound_buf'])
        assert torch.equal(p, pg) and torch.equal(buf, bufg) and flag.tolist() == [0, 0]


def _planted(g):
    """inf, -inf and NaN at about 1 position in 10^5 — index 0, the last index, one position in the second and one in the
    third trip of the loop among them — and a finite 3e38 that overflows only after grad_scale = 2."""
    g = g.copy()
    pos = np.unique(np.concatenate([[0, N_SCALAR - 1, TRIP + 12345, 2 * TRIP + 777], np.random.default_rng(43).integers(0, N_SCALAR, 26)]))
    g[pos] = np.resize(np.array([np.inf, -np.inf, np.nan], np.float32), pos.size)
    over = np.array([5, TRIP + 5, N_SCALAR - 2])
    assert not np.isin(over, pos).any()
    g[over] = np.float32(3e38)
    return g, np.sort(np.concatenate([pos, over]))


@pytest.mark.parametrize('kind', ['rmsprop', 'sgd'])
def test_guarded_steps_skip_exactly_the_nonfinite_elements(kind):
    """dsnt_rmsprop_step_guarded / dsnt_sgd_step_guarded (weight_decay 1e-4, grad_scale 2, a state with history).  flag[0]
    preset: parameters and state keep their bits, flag[1] stays 0.  Planted non-finite gradients: exactly those positions keep
    parameter and state bits, every other element meets the oracle's bars, flag == [0, DSNT_FLAG_GRAD]."""
    p0, grads = _opt_data()
    wd, gs = 1e-4, 2.0
    p, st = dev(p0), torch.zeros(N_SCALAR, device=DEV)
    step = (lambda g_, first, fl: _rms(p, g_, st, wd, gs, fl)) if kind == 'rmsprop' else (lambda g_, first, fl: _sgd(p, g_, st, 0.9, wd, gs, first, fl))
    flag = torch.zeros(2, dtype=torch.int32, device=DEV)
    step(dev(grads[0]), 1, flag)                       # history
    ph, sh = host(p), host(st)
    assert not np.array_equal(ph, p0) and flag.tolist() == [0, 0]
    blocked = torch.tensor([R.FLAG_LOSS, 0], dtype=torch.int32, device=DEV)
    step(dev(grads[1]), 0, blocked)
    assert np.array_equal(bits(host(p)), bits(ph)) and np.array_equal(bits(host(st)), bits(sh)) and blocked.tolist() == [R.FLAG_LOSS, 0]
    g, where = _planted(grads[1])
    step(dev(g), 0, flag)
    if kind == 'rmsprop':
        out, state, bs = R.rmsprop_step(ph, g, sh, 2.5e-4, 0.99, 1e-8, wd, gs, flag=[0, 0]), 'sq', 'bound_sq'
    else:
        out, state, bs = R.sgd_step(ph, g, sh, 0.2, 0.9, wd, gs, first_step=False, flag=[0, 0]), 'buf', 'bound_buf'
    assert np.array_equal(np.flatnonzero(out['skip']), where) and out['flag'] == [0, R.FLAG_GRAD]
    pn, sn = host(p), host(st)
    assert np.array_equal(bits(pn[where]), bits(ph[where])) and np.array_equal(bits(sn[where]), bits(sh[where]))
    _within(pn, out['p'], out['bound_p'])
    _within(sn, out[state], out[bs])
    assert (pn != ph).sum() >= N_SCALAR - where.size - N_SCALAR // 1000          # and the rest did move
    assert flag.tolist() == [0, R.FLAG_GRAD]


def test_nonfinite_flag_and_promotion():
    """dsnt_nonfinite_flag over n = 2 621 443: a clean tensor leaves the flag alone; one non-finite value at the LAST index
    (third trip, ragged workgroup) raises `code`; a pending flag[1] is promoted into flag[0], after which a guarded step changes
    nothing."""
    p0, grads = _opt_data()
    x = dev(grads[0])
    flag = torch.zeros(2, dtype=torch.int32, device=DEV)
    call('dsnt_nonfinite_flag', x, N_SCALAR, flag, R.FLAG_LOSS)
    assert flag.tolist() == R.nonfinite_flag(grads[0], [0, 0], R.FLAG_LOSS) == [0, 0]
    for v in (float('inf'), float('nan')):
        bad = x.clone()
        bad[-1] = v
        flag.zero_()
        call('dsnt_nonfinite_flag', bad, N_SCALAR, flag, R.FLAG_LOSS)
        assert flag.tolist() == R.nonfinite_flag(host(bad), [0, 0], R.FLAG_LOSS) == [R.FLAG_LOSS, 0]
    flag = torch.tensor([0, R.FLAG_GRAD], dtype=torch.int32, device=DEV)
    call('dsnt_nonfinite_flag', x, N_SCALAR, flag, R.FLAG_LOSS)
    assert flag.tolist() == R.nonfinite_flag(grads[0], [0, R.FLAG_GRAD], R.FLAG_LOSS) == [R.FLAG_GRAD, R.FLAG_GRAD]
    p, sq = dev(p0), torch.full((N_SCALAR,), 0.5, device=DEV)
    _rms(p, x, sq, 0.0, 1.0, flag)
    _sgd(p, x, sq, 0.9, 0.0, 1.0, 0, flag)
    assert np.array_equal(bits(host(p)), bits(p0)) and (sq == 0.5).all().item()
