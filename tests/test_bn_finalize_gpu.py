"""The BatchNorm finalise step — partial[tiles][2][C] (fp32 tile sums) -> mean / invstd / scale / shift and the running
statistics, or dgamma / dbeta / coef and the bound of dx — against tests/ew_ref.py's exact oracle, through the C ABI, in all
six places it lives: dsnt_bn_finalize, dsnt_bn_bwd_finalize (with DSNT_BN_FROZEN), dsnt_bn_bwd_finalize_bound,
bn_pro_forward<512> inside dsnt_conv_fwd_pro, bn_pro_backward<256> inside dsnt_bn_act_bwd_apply_pro and _pro_base.

The step is a pure function of a few KB, so the partials are made on the host (R.partial_*), each kind asserted to be
what it claims before any launch (the unmarked tests below run without a GPU):
  producer    fl32 of R.tile_sums of a bn_case x, last tile ragged;
  cancelling  integer tiles alternating +-2^26 with small odd integers: exact in fp64 in any order, wrong in fp32;
  constant    x = v everywhere: var is exactly 0, invstd sits at 1 / sqrt(eps);
  offset      mean 300 against spread 1: the interval bar of invstd is wide there (DESIGN.md has the numbers), a dropped
              tile still misses the mean bar.
Bars: R.bn_finalize / R.bn_bwd_finalize state them; none comes from a kernel's output.  scale is compared as bits, shift
against its two admissible bit patterns, both on the device's own mean / invstd.  Every output array carries 16 sentinel
elements behind C that must come back untouched, and the partial buffer one tile row of NaN behind `tiles`: a read past the
end poisons the result.

Shapes.  Stand-alone kernels (FIN_T = 1024: 16 channels x 64 tile lanes per block, the lane loop unrolled four-fold): tile
counts 1, 2, 63, 64, 65, 257, 1027, 4096 — one trip, the lane boundary, unrolled trips plus a remainder, the production
maximum (128 x 128 at batch 32) —, channel counts 4 (12 masked threads per lane), 20 (second block masked to 4), 64, 272
(17 blocks), 1040 for the bound (65 blocks: slot 0 takes two).  Prologues: PRO_C x the three tile counts of PRO_TILES, the
thread mapping of each in PRO_PREMISE (asserted from R.pro_mapping, the host mirror of bn_pro_sums)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ew_ref as R

gpu = pytest.mark.gpu
DEV = torch.device('cuda:0')
SENT = -777.0
PAD = 16
MOM, EPS = 0.1, 1e-5
ERR_ARG = 3                            # include/dsnt_hip.h: DSNT_ERR_ARG

# (tiles, C, kind): 14 (tiles, C) pairs
FIN_CASES = [(1, 4, 'producer'), (2, 20, 'producer'), (63, 64, 'producer'), (64, 4, 'cancelling'), (64, 272, 'producer'),
             (65, 272, 'cancelling'), (65, 20, 'constant'), (257, 64, 'offset'), (257, 20, 'cancelling'), (1027, 20, 'producer'),
             (1027, 272, 'cancelling'), (1027, 64, 'offset'), (4096, 64, 'cancelling'), (4096, 64, 'producer'), (4096, 4, 'constant')]
CONSTANTS = [7.25, -1234.5, 0.0, 1.0, -0.5, 100.0]

PRO_C = [4, 20, 64, 128, 160, 256]
# (C, NT) -> chunks of (columns, tile lanes, idle threads): bn_pro_sums<NT>, NT = 256 in the apply, 512 in the convolutions
PRO_PREMISE = {
    (4, 256): [(8, 32, 0)], (20, 256): [(40, 6, 16)], (64, 256): [(128, 2, 0)], (128, 256): [(256, 1, 0)],
    (160, 256): [(256, 1, 0), (64, 4, 0)],           # two chunks, the sum / cross-term boundary (column 160) inside the first
    (256, 256): [(256, 1, 0), (256, 1, 0)],
    (4, 512): [(8, 64, 0)], (20, 512): [(40, 12, 32)], (64, 512): [(128, 4, 0)], (128, 512): [(256, 2, 0)],
    (160, 512): [(320, 1, 192)], (256, 512): [(512, 1, 0)],
}
# (C, NT) -> tile counts: one, a second trip of the 16-deep load batch in every chunk (16 L + 1, L the chunks' largest), the
# most the entries take (tiles * C <= 16384)
PRO_TILES = {
    (4, 256): (1, 513, 4096), (20, 256): (1, 97, 819), (64, 256): (1, 33, 256), (128, 256): (1, 17, 128), (160, 256): (1, 65, 102),
    (256, 256): (1, 17, 64),
    (4, 512): (1, 1025, 4096), (20, 512): (1, 193, 819), (64, 512): (1, 65, 256), (128, 512): (1, 33, 128), (160, 512): (1, 17, 102),
    (256, 512): (1, 17, 64),
}


# ================================================================ host side: partials, premises
@functools.lru_cache(maxsize=None)
def _case(kind, T, Cc, small_M=False):
    """(partial [T][2][C] fp32, M, exact sums) of one case; small_M: a row count of about 2 T (the apply prologues run their
    apply on M rows — the finalise step only divides by M)."""
    seed = 1000 * T + Cc
    if kind == 'producer':
        rows = 2 if small_M else (R.TILE_ROWS if T <= 65 else 4)
        part, M, _ = R.partial_producer(T, Cc, seed, rows=rows)
    elif kind == 'offset':
        part, M, _ = R.partial_producer(T, Cc, seed, rows=2 if small_M else 4, offset=300.0)
    elif kind == 'cancelling':
        part, M = R.partial_cancelling(T, Cc, seed, M=2 * T - 1 if small_M else None)
    elif kind == 'constant':
        part, M, _ = R.partial_constant(T, Cc, CONSTANTS, rows=2 if small_M else R.TILE_ROWS)
    else:
        raise ValueError(kind)
    assert part.shape == (T, 2, Cc) and part.dtype == np.float32 and np.isfinite(part).all()
    part.setflags(write=False)
    return part, M, (R.exact_tile_sums(part), T)


def _claims(kind, T, Cc, small_M=False):
    """Every kind is what it says, by the oracle alone."""
    part, M, sums = _case(kind, T, Cc, small_M)
    o = R.bn_finalize(None, M, None, None, None, None, MOM, EPS, 1, sums=sums)
    eps = float(np.float32(EPS))
    if kind == 'producer':
        assert (part[:, 1] >= 0).all()
        if M >= 64:                                                         # (a statement about samples: not for a handful of rows)
            assert (np.abs(o['mean']) < np.sqrt(o['var'])).all()            # bn_case: |mean| < std
            assert (o['bar_invstd'] <= 4 * R.U * o['invstd']).all()         # the bar is tight here: two fp32 ulps
    elif kind == 'cancelling':
        p64 = part.astype(np.float64)
        assert (p64 == np.round(p64)).all() and (np.abs(p64) == 2.0 ** 26).any(0).all() and (p64 % 2 == 1).any(0).all()
        assert max(o['A0'].max(), o['A1'].max()) < 2.0 ** 53                # every partial sum exact in fp64, in any order
        assert (o['S0'] == p64[:, 0].sum(0)).all() and (o['S1'] == p64[:, 1].sum(0)).all()
        assert (o['var_raw'] > 0).all() and (o['dv'] <= 2.0 ** -20 * (o['var'] + eps)).all()
        f0, _ = R.combine_f32(part)
        miss = np.abs(f0 / M - o['mean']) / o['bar_mean']
        assert (miss >= 10).all(), miss.min()                               # an fp32 combine is told apart, tenfold
    elif kind == 'constant':
        v = np.array([CONSTANTS[c % len(CONSTANTS)] for c in range(Cc)])
        rows = M // T
        assert (part[:, 0].astype(np.float64) == rows * v).all() and (part[:, 1].astype(np.float64) == rows * v * v).all()
        assert (o['mean'] == v).all() and (o['var_raw'] == 0).all()
        assert (np.abs(o['invstd'] - 1 / np.sqrt(eps)) <= o['bar_invstd']).all()
    elif kind == 'offset':
        assert (np.abs(o['mean']) * o['invstd'] >= 100).all()
        # a dropped tile still shows: it moves the mean by ~300 / T, the bar is half an ulp of 300
        assert (np.abs(part[-1, 0].astype(np.float64)) / M >= 100 * o['bar_mean']).all()


@pytest.mark.parametrize('T,Cc,kind', FIN_CASES)
def test_partials_hold_what_they_claim(T, Cc, kind):
    _claims(kind, T, Cc)


def _pro_cases(NT):
    """(C, tiles, kind) of the prologue tests: producer partials at every tile count, cancelling ones from the second on."""
    out = []
    for Cc in PRO_C:
        for i, T in enumerate(PRO_TILES[(Cc, NT)]):
            out.append((Cc, T, 'producer'))
            if i > 0:
                out.append((Cc, T, 'cancelling'))
    return out


@pytest.mark.parametrize('NT', [256, 512])
def test_prologue_premise_table(NT):
    """PRO_PREMISE / PRO_TILES from the host mirror of bn_pro_sums' index arithmetic: the mapping of every channel count, every
    element of the partial buffer read exactly once (nothing behind `tiles`), one trip / two or more trips of the load batch in
    every chunk, the entries' limit reached."""
    for Cc in PRO_C:
        chunks = R.pro_mapping(Cc, NT)
        assert chunks == PRO_PREMISE[(Cc, NT)]
        one, second, most = PRO_TILES[(Cc, NT)]
        assert one == 1 and second == 16 * max(L for _, L, _ in chunks) + 1 and most == 16384 // Cc and second <= most
        assert (most + 1) * Cc > 16384
        for T, lo in ((one, 1), (second, 2), (most, 2)):
            cnt, trips = R.pro_reads(T, Cc, NT)
            assert (cnt == 1).all()
            assert all(t == 1 for t in trips) if lo == 1 else all(t >= 2 for t in trips)
    assert [c for c, _, _ in PRO_PREMISE[(160, 256)]][0] > 160 > 0                 # the statistic boundary lies inside chunk 0
    for Cc, T, kind in _pro_cases(NT):
        _claims(kind, T, Cc, small_M=(NT == 256))


def test_finalize_bound_refuses_the_frozen_flag():
    """dsnt_bn_bwd_finalize_bound with DSNT_BN_FROZEN: DSNT_ERR_ARG before anything is launched (a frozen BatchNorm has no folded
    apply; the flag used to reach the kernel as `accumulate`).  Host-side check: the pointers are never followed."""
    from dsnt import _lib
    fake = [C.c_void_p(0x1000 * (i + 1)) for i in range(7)]
    for flags in (R.BN_FROZEN, R.BN_FROZEN | 1):
        rc = _lib.fn('dsnt_bn_bwd_finalize_bound')(fake[0], 3, 100, 20, fake[1], fake[2], flags, fake[3], fake[4], fake[5], fake[6], None)
        assert rc == ERR_ARG and b'DSNT_BN_FROZEN' in _lib.fn('dsnt_last_error')()


# ================================================================ device side: helpers
def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(DEV)


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def call(name, *args):
    from dsnt._lib import call as c, ptr
    c(name, *[ptr(a) if isinstance(a, torch.Tensor) else a for a in args])


def padded(n, init=None):
    """n elements (+ PAD sentinels) on the device: NaN where the launch must write, `init` where it reads first."""
    t = torch.full((n + PAD,), SENT, device=DEV)
    t[:n] = float('nan') if init is None else dev(np.asarray(init, dtype=np.float32))
    return t


def take(t, n):
    """The first n elements on the host; the sentinels behind them must be intact."""
    h = host(t)
    assert (h[n:] == SENT).all(), 'wrote behind element %d: %s' % (n, h[n:])
    return h[:n].copy()


def dev_partial(part):
    """The partial buffer with one tile row of NaN behind it."""
    T, _, Cc = part.shape
    return dev(np.concatenate([part, np.full((1, 2, Cc), np.nan, np.float32)]))


def within(got, want, bar, what):
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - want)
    bad = ~(err <= bar)                                           # (a NaN is bad)
    assert not bad.any(), '%s: channel %d got %r want %r: err %.3e bar %.3e (%d channels)' % (
        what, np.flatnonzero(bad)[0], got[bad][0], np.asarray(want)[bad][0], err[bad][0], np.asarray(bar)[bad][0], bad.sum())


def affine(Cc, seed):
    r = np.random.default_rng(seed)
    return (r.uniform(-1, 1, Cc) + 0.25).astype(np.float32), (r.standard_normal(Cc) * 0.2).astype(np.float32)     # gamma of both signs


def check_forward(launch, M, Cc, sums, gamma, beta, running, calls=1, training=1):
    """launch(gamma, beta, rm, rv, mean, invstd, scale, shift) (device tensors or None) `calls` times on the same buffers; after
    each, the four vectors and the running pair against the oracle fed with what the launch found.  Returns the last call's
    device vectors (mean, invstd, scale, shift)."""
    g, b = (None if v is None else dev(v) for v in (gamma, beta))
    r = np.random.default_rng(Cc)
    rm, rv = (padded(Cc, r.standard_normal(Cc) * 0.3), padded(Cc, r.uniform(0.5, 2.0, Cc))) if running else (None, None)
    for _ in range(calls):
        rm0, rv0 = (take(rm, Cc), take(rv, Cc)) if running else (None, None)
        outs = [padded(Cc) for _ in range(4)]
        launch(g, b, rm, rv, *outs)
        torch.cuda.synchronize()
        o = R.bn_finalize(None, M, gamma, beta, rm0, rv0, MOM, EPS, training, sums=sums)
        mu, is_, sc, sh = (take(t, Cc) for t in outs)
        within(mu, o['mean'], o['bar_mean'], 'mean')
        within(is_, o['invstd'], o['bar_invstd'], 'invstd')
        assert np.array_equal(bits(sc), bits(R.scale_bits(gamma, is_))), 'scale != fl32(gamma * invstd) as bits'
        ok = R.shift_ok(beta, mu, sc, sh)
        assert ok.all(), 'shift: channel %d is neither beta - fl(mean scale) nor the fused value' % np.flatnonzero(~ok)[0]
        if running and training:
            within(take(rm, Cc), o['running_mean'], o['bar_running_mean'], 'running_mean')
            within(take(rv, Cc), o['running_var'], o['bar_running_var'], 'running_var')
            assert not np.array_equal(take(rm, Cc), rm0)
        elif running:
            assert np.array_equal(bits(take(rm, Cc)), bits(rm0)) and np.array_equal(bits(take(rv, Cc)), bits(rv0))
            assert np.array_equal(bits(mu), bits(rm0)), 'eval mode: mean is the running mean, as bits'
    return outs


def check_backward(launch, M, Cc, sums, flags, with_dg, with_db, form='fin'):
    """launch(dgamma, dbeta, flags, coef) once: coef [2][C], dgamma, dbeta against R.bn_bwd_finalize.  Returns coef."""
    r = np.random.default_rng(7 * Cc + flags)
    dg0, db0 = r.standard_normal(Cc).astype(np.float32) * 50, r.standard_normal(Cc).astype(np.float32) * 50
    dg, db = padded(Cc, dg0) if with_dg else None, padded(Cc, db0) if with_db else None
    coef = padded(2 * Cc)
    launch(dg, db, flags, coef)
    torch.cuda.synchronize()
    o = R.bn_bwd_finalize(None, M, flags, dg0 if with_dg else None, db0 if with_db else None, sums=sums)
    cf = take(coef, 2 * Cc).reshape(2, Cc)
    if flags & R.BN_FROZEN:
        assert (np.abs(cf) == 0).all(), 'DSNT_BN_FROZEN: both coefficient rows are zero'
    else:
        within(cf[0], o['coef'][0], o['bar_coef'][0], 'coef0 (%s flags %d)' % (form, flags))
        within(cf[1], o['coef'][1], o['bar_coef'][1], 'coef1 (%s flags %d)' % (form, flags))
    if with_dg:
        within(take(dg, Cc), o['dgamma'], o['bar_dgamma'], 'dgamma (%s flags %d)' % (form, flags))
    if with_db:
        within(take(db, Cc), o['dbeta'], o['bar_dbeta'], 'dbeta (%s flags %d)' % (form, flags))
    return cf


# ================================================================ the stand-alone kernels
@gpu
@pytest.mark.parametrize('T,Cc,kind', FIN_CASES)
def test_bn_finalize(T, Cc, kind):
    """dsnt_bn_finalize, training: everything given (two consecutive calls: the running statistics move twice, each within
    its bar), nothing given, gamma alone, beta and the running pair alone."""
    part, M, sums = _case(kind, T, Cc)
    _claims(kind, T, Cc)
    pd = dev_partial(part)
    gamma, beta = affine(Cc, T)

    def launch(g, b, rm, rv, mu, is_, sc, sh):
        call('dsnt_bn_finalize', pd, T, M, Cc, g, b, rm, rv, MOM, EPS, 1, mu, is_, sc, sh)
    check_forward(launch, M, Cc, sums, gamma, beta, True, calls=2)
    check_forward(launch, M, Cc, sums, None, None, False)
    check_forward(launch, M, Cc, sums, gamma, None, False)
    check_forward(launch, M, Cc, sums, None, beta, True)


@gpu
@pytest.mark.parametrize('Cc', [4, 20, 272])
def test_bn_finalize_single_row_and_eval_mode(Cc):
    """M == 1 (unbias = 1: the running variance moves towards 0, not towards a division by zero); and training = 0 with
    partial = NULL: mean is the running mean as bits, invstd within half an ulp of the fp64 value, nothing moves."""
    part, M, _ = R.partial_producer(1, Cc, 5, rows=1)
    assert M == 1
    pd = dev_partial(part)
    gamma, beta = affine(Cc, 1)
    sums = (R.exact_tile_sums(part), 1)

    def launch(g, b, rm, rv, mu, is_, sc, sh):
        call('dsnt_bn_finalize', pd, 1, 1, Cc, g, b, rm, rv, MOM, EPS, 1, mu, is_, sc, sh)
    check_forward(launch, 1, Cc, sums, gamma, beta, True, calls=2)

    def launch_eval(g, b, rm, rv, mu, is_, sc, sh):
        call('dsnt_bn_finalize', None, 0, 77, Cc, g, b, rm, rv, MOM, EPS, 0, mu, is_, sc, sh)
    check_forward(launch_eval, 77, Cc, None, gamma, beta, True, training=0)
    check_forward(launch_eval, 77, Cc, None, None, None, True, training=0)


@gpu
@pytest.mark.parametrize('T,Cc,kind', FIN_CASES)
def test_bn_bwd_finalize(T, Cc, kind):
    """dsnt_bn_bwd_finalize on the same partials read as (sum dz, sum dz xhat): flags 0, 1, DSNT_BN_FROZEN, DSNT_BN_FROZEN | 1,
    each with dgamma and / or dbeta NULL."""
    part, M, sums = _case(kind, T, Cc)
    pd = dev_partial(part)

    def launch(dg, db, flags, coef):
        call('dsnt_bn_bwd_finalize', pd, T, M, Cc, dg, db, flags, coef)
    for flags in (0, 1, 2, 3):
        for with_dg, with_db in ((True, True), (False, True), (True, False), (False, False)):
            check_backward(launch, M, Cc, sums, flags, with_dg, with_db)


@gpu
@pytest.mark.parametrize('T,Cc,kind', [(64, 4, 'cancelling'), (2, 20, 'producer'), (65, 272, 'cancelling'), (257, 1040, 'producer'),
                                       (1027, 1040, 'cancelling')])
def test_bn_bwd_finalize_bound(T, Cc, kind):
    """dsnt_bn_bwd_finalize_bound: coef / dgamma / dbeta as dsnt_bn_bwd_finalize leaves them, and slot s of bound_out = the maximum
    over the 16-channel blocks vb = s (mod 64) of |scale_c| (max dz_amax + |coef0_c| + |coef1_c| sqrtf(M)) on the device's own
    coef, within gamma(5), never below what the slot held; dz_amax has its maximum in slot 63.  Two launches, the pre-load
    moved between them, so that every populated slot — slot 0 included — is compared with the oracle's value in one of them:
      flags 0: slot 0 zero (as the caller leaves it), slot 1 above every bound, slot 2 far below;
      flags 1: slot 0 above every bound, slot 1 far below, the rest zero.
    The slots no block maps to hold 5.0 and keep their bits.  At C = 1040 slot 0 takes blocks 0 and 64, and block 64 (scale
    times 8) decides it: the first launch fails on a kernel that leaves block 64 out, the one-block case on a wrong block 0.
    With the frozen flag the entry refuses and writes nothing."""
    part, M, sums = _case(kind, T, Cc)
    pd = dev_partial(part)
    r = np.random.default_rng(Cc + T)
    scale = (r.uniform(0.2, 2.0, Cc) * np.where(r.integers(0, 2, Cc) > 0, 1, -1)).astype(np.float32)
    if Cc == 1040:
        scale[1024:] *= 8                                       # block 64 decides slot 0, not block 0
    dz = r.uniform(0.0, 1.0, 64).astype(np.float32)
    dz[63] = 3.0
    nblocks = (Cc + 15) // 16
    pop = min(nblocks, 64)                                      # populated slots
    sd, dzd = dev(scale), dev(dz)
    for flags in (0, 1):
        prev = np.zeros(64, np.float32)
        prev[pop:] = 5.0
        if flags == 0:
            prev[1], prev[2] = 1e30, 1e-30
        else:
            prev[0], prev[1] = 1e30, 1e-30
        bound = padded(64, prev)

        def launch(dg, db, fl, coef):
            call('dsnt_bn_bwd_finalize_bound', pd, T, M, Cc, dg, db, fl, coef, sd, dzd, bound)
        cf = check_backward(launch, M, Cc, sums, flags, True, flags == 0, form='bound')
        o = R.bn_bwd_finalize(None, M, flags, None, None, scale=scale, dz_amax=dz, sums=sums)
        want = o['bound'](cf)
        got32 = take(bound, 64)
        got = got32.astype(np.float64)
        assert (want[:pop] > 0.5).all() and (want[:pop] < 1e29).all() and not want[pop:].any()       # (|scale| >= 0.2, max dz = 3)
        assert (got >= prev).all(), 'a slot was lowered'
        assert np.array_equal(bits(got32[pop:]), bits(prev[pop:])), 'a slot no block maps to was written'
        high = prev == np.float32(1e30)
        assert np.array_equal(bits(got32[high]), bits(prev[high])), 'a slot above the bound was changed'
        final = np.maximum(prev.astype(np.float64), want)
        within(got, final, o['bar_bound_rel'] * want, 'bound slot (flags %d)' % flags)
        # which slots that held the device to the oracle's value: all populated ones but the high one
        held = np.flatnonzero((final == want) & (want > 0))
        assert held.tolist() == [s_ for s_ in range(pop) if not high[s_]]
        if flags == 0:
            assert 0 in held                                    # block 0 (and at C = 1040 block 64) against the oracle
            if Cc == 1040:
                c64 = np.abs(cf[:, 1024:].astype(np.float64))
                blk64 = (np.abs(scale[1024:].astype(np.float64)) * (3.0 + c64[0] + c64[1] * float(np.sqrt(np.float32(M))))).max()
                c0 = np.abs(cf[:, :16].astype(np.float64))
                blk0 = (np.abs(scale[:16].astype(np.float64)) * (3.0 + c0[0] + c0[1] * float(np.sqrt(np.float32(M))))).max()
                assert want[0] == blk64 and blk64 > 2 * blk0        # without block 64 the device would sit at blk0: far outside gamma(5)
    from dsnt import _lib
    from dsnt._lib import ptr
    coef, dg = padded(2 * Cc), padded(Cc, np.zeros(Cc))
    before = take(bound, 64)
    rc = _lib.fn('dsnt_bn_bwd_finalize_bound')(ptr(pd), T, M, Cc, ptr(dg), None, R.BN_FROZEN, ptr(coef), ptr(sd), ptr(dzd), ptr(bound), None)
    torch.cuda.synchronize()
    assert rc == ERR_ARG and np.isnan(take(coef, 2 * Cc)).all() and not take(dg, Cc).any() and np.array_equal(take(bound, 64), before)


# ================================================================ the prologue forms
def _geom(N, H, W, Cin, Cout):
    from dsnt._lib import ConvGeom
    return ConvGeom(N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, 1)


@gpu
@pytest.mark.parametrize('Cc,T,kind', _pro_cases(512))
def test_conv_prologue_finalises_to_the_oracle(Cc, T, kind):
    """bn_pro_forward<512> inside dsnt_conv_fwd_pro.  The prologue's tiles and M have nothing to do with the convolution's
    geometry (only C == Cin is checked), so the partials are the hand-made ones and the convolution a 1 x 1 one:
      C -> 4 channels on 16 rows (one workgroup) and on 289 rows (three): dsnt_conv_fwd_bm says 128 for both — the tiled
        kernel; the larger stays for more than one workgroup writing the vectors (the running statistics at a grid that
        can tell a second move: the next test);
      C -> 128 channels on 16 rows: dsnt_conv_fwd_bm says 32, and conv_fwd_impl then takes conv_ksplit_kernel when
        Cin % 8 == 0 and rows <= 2048 (its default ksplit_rows) — C = 64, 128, 160, 256, four workgroups — and the 32-row
        tiling conv_fwd_kernel<1, 4, 1, 1> otherwise (C = 4, 20, one workgroup).  The ABI does not report the kernel; the
        condition is restated here (KSPLIT) and the channel counts that meet it are asserted.
    The four vectors and the running pair against the oracle (everything given, and nothing given), and the output ==
    dsnt_conv_fwd_ex on the vectors the prologue left, within the 1e-6 of the existing prologue test."""
    from dsnt import _lib
    from dsnt._lib import BnPrologue, ptr
    part, M, sums = _case(kind, T, Cc)
    pd = dev_partial(part)
    gamma, beta = affine(Cc, T)
    r = np.random.default_rng(T + Cc)
    # (rows = hw * hw, Cout, dsnt_conv_fwd_bm, K-split?)  K-split: bm == 32 and rows <= 2048 and Cin % 8 == 0 (conv_fwd_impl)
    for rows_hw, Cout, bm_want, ksplit_want in ((4, 4, 128, False), (17, 4, 128, False), (4, 128, 32, Cc in (64, 128, 160, 256))):
        g = _geom(1, rows_hw, rows_hw, Cc, Cout)
        rows = rows_hw * rows_hw
        assert _lib.fn('dsnt_conv_fwd_pro_ok')(C.byref(g), T, Cc) == 1
        bm = _lib.fn('dsnt_conv_fwd_bm')(C.byref(g))
        assert bm == bm_want and (bm == 32 and rows <= 2048 and Cc % 8 == 0) == ksplit_want
        x = dev(r.standard_normal((rows, Cc)).astype(np.float32))
        w = dev((r.standard_normal((Cout, Cc)) * 0.1).astype(np.float32))
        bias = dev(r.standard_normal(Cout).astype(np.float32))
        y = torch.full((rows, Cout), float('nan'), device=DEV)

        def launch(g_, b_, rm, rv, mu, is_, sc, sh):
            pro = BnPrologue(ptr(pd), T, Cc, M, ptr(g_), ptr(b_), ptr(rm), ptr(rv), MOM, EPS, ptr(mu), ptr(is_), ptr(sc), ptr(sh))
            call('dsnt_conv_fwd_pro', x, w, bias, y, C.byref(pro), 1, None, None, None, C.byref(g), None)
        for gm, bt, running in ((gamma, beta, True), (None, None, False)):
            _, _, sc, sh = check_forward(launch, M, Cc, sums, gm, bt, running, calls=2 if running else 1)
            y_ref = torch.full((rows, Cout), float('nan'), device=DEV)
            call('dsnt_conv_fwd_ex', x, w, bias, y_ref, sc, sh, 1, None, None, None, C.byref(g), None, None)
            torch.cuda.synchronize()
            assert torch.isfinite(y_ref).all()
            assert (y - y_ref).abs().max().item() <= 1e-6 * y_ref.abs().max().item()


@gpu
@pytest.mark.parametrize('kernel,Cc,T,H,W,Cout', [('tiled', 4, 1025, 512, 512, 4), ('ksplit', 64, 65, 32, 64, 1024)])
def test_conv_prologue_moves_the_running_statistics_once_at_a_full_grid(kernel, Cc, T, H, W, Cout):
    """Every workgroup of dsnt_conv_fwd_pro finalises for itself, workgroup 0 alone moves the running statistics.  With a
    handful of workgroups a kernel that let ALL of them move the pair would still pass: they start together, read the old
    pair together and store the same value.  So here the grid is 2048 workgroups of 512 threads — more than the chip holds
    at once (256 CUs x 32 waves: at most 1024) —, the later ones start when workgroup 0 has long stored, and a second move
    would show as m (1 - m) (old - mean), far outside the bar.  Both fp32 kernels: the 128-row tiling (C -> 4 channels on
    512 x 512 rows) and the K-split (64 -> 1024 channels on 2048 rows: bm = 32, Cin % 8 == 0, rows <= 2048)."""
    from dsnt import _lib
    from dsnt._lib import BnPrologue, ptr
    part, M, sums = _case('producer', T, Cc)
    pd = dev_partial(part)
    gamma, beta = affine(Cc, T)
    g = _geom(1, H, W, Cc, Cout)
    rows = H * W
    bm = _lib.fn('dsnt_conv_fwd_bm')(C.byref(g))
    is_ksplit = bm == 32 and rows <= 2048 and Cc % 8 == 0
    grid = (rows + 31) // 32 * ((Cout + 31) // 32) if is_ksplit else (rows + bm - 1) // bm * ((Cout + 31) // 32 if bm == 128 and Cout <= 32 else -1)
    assert is_ksplit == (kernel == 'ksplit') and bm == (32 if is_ksplit else 128) and grid == 2048 > 1024
    assert _lib.fn('dsnt_conv_fwd_pro_ok')(C.byref(g), T, Cc) == 1
    r = np.random.default_rng(Cc)
    x = dev(r.standard_normal((rows, Cc)).astype(np.float32))
    w = dev((r.standard_normal((Cout, Cc)) * 0.1).astype(np.float32))
    y = torch.empty((rows, Cout), device=DEV)

    def launch(g_, b_, rm, rv, mu, is_, sc, sh):
        pro = BnPrologue(ptr(pd), T, Cc, M, ptr(g_), ptr(b_), ptr(rm), ptr(rv), MOM, EPS, ptr(mu), ptr(is_), ptr(sc), ptr(sh))
        call('dsnt_conv_fwd_pro', x, w, None, y, C.byref(pro), 1, None, None, None, C.byref(g), None)
    check_forward(launch, M, Cc, sums, gamma, beta, True, calls=2)
    assert torch.isfinite(y).all()


@gpu
@pytest.mark.parametrize('Cc,T,kind', _pro_cases(256))
def test_apply_prologue_finalises_to_the_oracle(Cc, T, kind):
    """bn_pro_backward<256> inside dsnt_bn_act_bwd_apply_pro and _pro_base: coef / dgamma / dbeta against the oracle with
    accumulate_params 0 and 1 (dx itself is held element by element in test_elementwise_edges_gpu.py).  The apply runs on the
    partials' own M rows (about 2 T here)."""
    part, M, sums = _case(kind, T, Cc, small_M=True)
    pd = dev_partial(part)
    x, gamma, beta, da = R.bn_case(M, Cc, seed=T)
    mu, is_, sc, sh = (dev(v) for v in R.bn_vectors(x, gamma, beta))
    xd, dad = dev(x), dev(da)
    base = dev(np.random.default_rng(T).standard_normal((M, Cc)).astype(np.float32))
    for form in ('dsnt_bn_act_bwd_apply_pro', 'dsnt_bn_act_bwd_apply_pro_base'):
        for accp in (0, 1):
            dx = torch.full((M * Cc + PAD,), SENT, device=DEV)

            def launch(dg, db, flags, coef):
                if form.endswith('_base'):
                    call(form, dad, xd, sc, sh, mu, is_, pd, T, dg, db, flags, coef, 1, base, dx, M, Cc, None)
                else:
                    call(form, dad, xd, sc, sh, mu, is_, pd, T, dg, db, flags, coef, 1, dx, 0, M, Cc, None)
            check_backward(launch, M, Cc, sums, accp, True, True, form=form)
            h = host(dx)
            assert np.isfinite(h[:M * Cc]).all() and (h[M * Cc:] == SENT).all()
        # dgamma / dbeta NULL, one and the other: coef alone (both entries)
        check_backward(launch, M, Cc, sums, 0, False, False, form=form)
        check_backward(launch, M, Cc, sums, 1, True, False, form=form)
        check_backward(launch, M, Cc, sums, 1, False, True, form=form)


# ================================================================ what the one-pass tile sums cost (measured, not gated)
GROUPS = [('mean 0', 0.0, 1.0), ('mean / spread 3', 3.0, 1.0), ('30', 30.0, 1.0), ('300', 300.0, 1.0), ('3000', 3000.0, 1.0),
          ('spread 1e-3 at 1e4', 1e4, 1e-3), ('constant', 7.25, 0.0)]


def offset_input(M=4133, Cc=64, seed=11):
    r = np.random.default_rng(seed)
    x = np.empty((M, Cc), dtype=np.float32)
    for c in range(Cc):
        _, mean, spread = GROUPS[c % len(GROUPS)]
        x[:, c] = (mean + spread * r.standard_normal(M)).astype(np.float32)
    return x


@gpu
def test_one_pass_sums_end_to_end_on_offset_channels(capsys):
    """dsnt_bn_stats -> dsnt_bn_finalize on M = 4133, C = 64, channels in seven groups from mean 0 to mean / spread 1e7 and
    constant.  Bar: the oracle on the exact fp64 tile sums of the same fp32 x, e_k = the propagated a-priori bound of the
    design as it stands, gamma(tile_sum_ops(M, C)) sum |term| for the fp32 tile sums (+ the fp64 combine's).  On the centred
    channels that is a real bar (a dropped row misses it); on the offset channels it is a sanity bound — var - dv reaches 0
    there and the interval runs up to 1 / sqrt(eps).  Printed per group, for DESIGN.md: the relative invstd error of the device
    and of torch's fp32 batch norm on the CPU against fp64, and the bar.  No threshold on their ratio is asserted."""
    M, Cc = 4133, 64
    x = offset_input(M, Cc)
    s1, s2, a1, a2 = R.tile_sums(x, M, Cc)
    T = s1.shape[0]
    n = R.tile_sum_ops(M, Cc)
    A0, A1 = a1.sum(0), a2.sum(0)
    err = ((R.gamma(n) + R.gamma64(T)) * A0, (R.gamma(n) + R.gamma64(T)) * A1)
    o = R.bn_finalize(np.stack([s1, s2], 1), M, None, None, None, None, MOM, EPS, 1, sum_err=err)
    pd = torch.full((T + 1, 2, Cc), float('nan'), device=DEV)
    outs = [padded(Cc) for _ in range(4)]
    call('dsnt_bn_stats', dev(x), pd, M, Cc)
    call('dsnt_bn_finalize', pd, T, M, Cc, None, None, None, None, MOM, EPS, 1, *outs)
    torch.cuda.synchronize()
    assert torch.isnan(pd[T]).all()
    mu, is_ = take(outs[0], Cc), take(outs[1], Cc)
    _, tmean, tis = torch.native_batch_norm(torch.from_numpy(x), None, None, None, None, True, 0.1, float(np.float32(EPS)))
    rel_dev, rel_ref = (np.abs(v.astype(np.float64) - o['invstd']) / o['invstd'] for v in (is_, tis.numpy()))
    with capsys.disabled():
        print('\ngroup                 |mean| invstd   device    torch fp32 CPU   a-priori bar   (max over the group, relative to fp64)')
        for gi, (name, _, _) in enumerate(GROUPS):
            ch = np.arange(gi, Cc, len(GROUPS))
            print('%-20s %10.3g   %10.2e   %10.2e   %10.2e' % (name, (np.abs(o['mean']) * o['invstd'])[ch].max(), rel_dev[ch].max(),
                                                                rel_ref[ch].max(), (o['bar_invstd'] / o['invstd'])[ch].max()))
    within(mu, o['mean'], o['bar_mean'], 'mean')
    within(is_, o['invstd'], o['bar_invstd'], 'invstd')
    # the bar bites where the channel is centred: the oracle itself, fed the sums without the last row (M kept: the row counts
    # as zeros), misses it wherever that row moves var, by x (x - 2 mean) / M, by more than a tenth of var / M
    centred = np.arange(0, Cc, len(GROUPS))
    d1, d2, _, _ = R.tile_sums(x[:-1], M - 1, Cc)
    drop = R.bn_finalize(np.stack([d1, d2], 1), M, None, None, None, None, MOM, EPS, 1)
    last = x[-1, centred].astype(np.float64)
    tell = centred[np.abs(last * (last - 2 * o['mean'][centred])) > 0.1 * o['var'][centred]]
    assert tell.size >= 5 and (np.abs(drop['invstd'] - o['invstd'])[tell] > o['bar_invstd'][tell]).all()
