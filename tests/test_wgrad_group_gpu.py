"""The grouped weight-gradient launch (dsnt_conv_wgrad_group) on fp16x3 descriptors and ragged maps, the table-driven slab
reduction (dsnt_wgrad_reduce_all) and the table-driven eval-mode BatchNorm vectors (dsnt_bn_eval_prep), through the C ABI.

Every weight gradient of the 16x16 ... 4x4 hourglass levels runs through ONE dsnt_conv_wgrad_group launch over a table of
dsnt_conv_wgrad_desc_f16x3 descriptors (convop.py ConvOp.wgrad_slab): wgrad6_body<true, true> of csrc/wgrad_gemm.hip, picked per
workgroup from the descriptor's a_bound.  Here that launch is held to an fp64 reference case by case (tests/wgrad_group_ref.py:
single, odd and short steps, maps smaller than a step, image boundaries that move inside the step, masked tiles), its slabs are
checked for bounds, for independence of the grid's padding and of the table order, and against the per-convolution launches of
the same body.  All bars are the ones of test_conv_gpu.py test_wgrad_f16x3 (with the CPU float32 reference as the fp32 error) or
derived bounds; nothing here is measured."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import wgrad_group_ref as R

pytestmark = pytest.mark.gpu

CANARY = -7.25
IDS = ['x'.join(map(str, c)) for c, _ in R.CASES]


def _geom(case):
    from dsnt._lib import ConvGeom
    N, H, W, Cin, Cout, k, stride, pad, dil = case
    Ho, Wo = R.out_hw(case)
    return ConvGeom(N, H, W, Cin, Ho, Wo, Cout, k, k, stride, pad, dil)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


class Guarded:
    """A workspace of exactly n floats, NaN-filled, inside a larger buffer with 256 canary floats on each side."""

    def __init__(self, n, dev):
        self.n = n
        self.buf = torch.full((256 + n + 256,), CANARY, device=dev)
        self.ws = self.buf[256:256 + n]
        assert self.ws.data_ptr() % 16 == 0
        self.refill()

    def refill(self):
        self.ws.fill_(float('nan'))

    def snapshot(self):
        return self.buf.clone()


class Case:
    pass


def _check_why(c):
    """The property a case is in the table for, from the library's own plan — asserted before anything is launched."""
    from dsnt import _lib
    why, g, case = c.why, c.g, c.case
    assert g.Wo % 4 == 0 and _lib.fn('dsnt_conv_wgrad_bf16x6_ok')(C.byref(g)) == 1
    assert c.M == why['M'] and g.Ho * g.Wo == why['HoWo']
    assert _lib.fn('dsnt_conv_f16x3_route')(C.byref(g), 1) == why['route']
    ktiles, ntiles, splits, rows = R.plan(case)
    assert _lib.fn('dsnt_conv_wgrad_splits')(C.byref(g)) == splits == why['splits']
    assert c.nblk == ktiles * ntiles * splits
    assert R.split_steps(case) == why['steps']
    if 'last_rows' in why:
        assert c.M - (c.M - 1) // 16 * 16 == why['last_rows']
    if 'ktiles' in why:
        assert (ktiles, ntiles) == (why['ktiles'], why['ntiles']) and c.K < 128 and 128 < g.Cout < 256
    # the workspace (sized for ANY weight-gradient entry point on the geometry) holds this plan's slabs
    assert c.used <= c.nws


def _table(descs, dev):
    return torch.frombuffer(bytearray(b''.join(descs)), dtype=torch.uint8).to(dev)


def _build(raw):
    """All cases in one table, one dsnt_conv_wgrad_group launch, one dsnt_wgrad_reduce_all; then the launch again with a padded
    grid and in reversed table order, the mixed fp16x3 / bf16x6 table and the per-convolution launches.  Snapshots of the
    guarded workspaces after every launch are what the tests compare."""
    from dsnt import _lib
    from dsnt._lib import ptr, call
    dev = torch.device('cuda:0')
    nbytes = _lib.fn('dsnt_conv_wgrad_desc_bytes')()
    assert nbytes > 0
    cases = []
    for ci, (case, why) in enumerate(R.CASES):
        c = Case()
        c.ci, c.case, c.why = ci, case, why
        N, H, W, Cin, Cout, k, stride, pad, dil = case
        c.g = g = _geom(case)
        c.M, c.K, c.Cout, c.k, c.Cin = N * g.Ho * g.Wo, k * k * Cin, Cout, k, Cin
        x, sc, sh, c.relu, gy = R.operands(ci, case, raw)
        act = R.activation(x, sc, sh, c.relu)
        if raw:
            assert bool((act < 0).any()) and torch.equal(act, x)
        c.dw64, c.dw32, c.db64 = R.references(case, act, gy)
        c.x, c.gy, c.sc, c.sh = _nhwc(x).to(dev), _nhwc(gy).to(dev), sc.to(dev), sh.to(dev)
        c.ab = torch.full((64,), act.abs().max().item() * 16.0, device=dev)
        c.gb = torch.zeros(64, device=dev)
        call('dsnt_amax', ptr(c.gy), c.gy.numel(), ptr(c.gb))
        c.splits = _lib.fn('dsnt_conv_wgrad_splits')(C.byref(g))
        c.nws = _lib.fn('dsnt_conv_wgrad_ws_floats')(C.byref(g))
        c.used = c.splits * Cout * c.K + c.splits * Cout
        c.w = Guarded(c.nws, dev)
        desc = C.create_string_buffer(nbytes)
        c.nblk = _lib.fn('dsnt_conv_wgrad_desc_f16x3')(ptr(c.x), ptr(c.sc), ptr(c.sh), c.relu, ptr(c.gy), ptr(c.w.ws), ptr(c.ab),
                                                       ptr(c.gb), C.byref(g), desc)
        assert c.nblk > 0, _lib.fn('dsnt_last_error')()
        c.desc = desc.raw
        _check_why(c)
        cases.append(c)
    assert float(torch.stack([c.gb.max() for c in cases]).min()) > 0
    top = max(c.nblk for c in cases)

    def launch(descs, max_blocks):
        t = _table(descs, dev)
        call('dsnt_conv_wgrad_group', ptr(t), len(descs), max_blocks)
        torch.cuda.synchronize()

    # 1. the engine's launch (max_blocks rounded up to a multiple of 8) and the one reduction
    launch([c.desc for c in cases], (top + 7) // 8 * 8)
    rows = []
    for c in cases:
        c.snap = c.w.snapshot()
        c.dw = torch.full((c.Cout, c.k, c.k, c.Cin), float('nan'), device=dev)
        c.db = torch.full((c.Cout,), float('nan'), device=dev)
        rows.append([c.w.ws.data_ptr(), c.dw.data_ptr(), c.db.data_ptr(), c.splits, c.Cout * c.K, c.Cout, 0])
    t = torch.tensor(rows, dtype=torch.int64).to(dev)
    call('dsnt_wgrad_reduce_all', ptr(t), len(rows), max((r[4] // 4 + (r[5] + 3) // 4 + 63) // 64 for r in rows))
    torch.cuda.synchronize()
    if raw:
        # the raw operand un-grouped is the launch WITHOUT a prologue: the identity prologue has to give the same bits
        for c in cases:
            if c.why['route'] == 0:
                c.w.refill()
                call('dsnt_conv_wgrad_f16x3', ptr(c.x), None, None, 0, ptr(c.gy), ptr(c.w.ws), None, None, 0, ptr(c.ab),
                     ptr(c.gb), C.byref(c.g))
                c.snap_single = c.w.snapshot()
        torch.cuda.synchronize()
        return cases
    # 2. 64 padding workgroups per table row more; 3. the table in reversed order
    for c in cases:
        c.w.refill()
    launch([c.desc for c in cases], top + 64)
    for c in cases:
        c.snap_padded = c.w.snapshot()
        c.w.refill()
    launch([c.desc for c in reversed(cases)], (top + 7) // 8 * 8)
    for c in cases:
        c.snap_reversed = c.w.snapshot()
        c.w.refill()
    # 4. the mixed table: fp16x3 and bf16x6 descriptors alternate, every case of R.MIXED both ways
    descs = []
    for ci in R.MIXED:
        c = cases[ci]
        c.w6 = Guarded(c.nws, dev)
        desc = C.create_string_buffer(nbytes)
        n = _lib.fn('dsnt_conv_wgrad_desc')(ptr(c.x), ptr(c.sc), ptr(c.sh), c.relu, ptr(c.gy), ptr(c.w6.ws), C.byref(c.g), desc)
        assert n == c.nblk
        descs += [c.desc, desc.raw]
    launch(descs, (top + 7) // 8 * 8)
    rows = []
    for ci in R.MIXED:
        c = cases[ci]
        c.snap_mixed, c.snap_mixed6 = c.w.snapshot(), c.w6.snapshot()
        c.dw6 = torch.full((c.Cout, c.k, c.k, c.Cin), float('nan'), device=dev)
        c.db6 = torch.full((c.Cout,), float('nan'), device=dev)
        rows.append([c.w6.ws.data_ptr(), c.dw6.data_ptr(), c.db6.data_ptr(), c.splits, c.Cout * c.K, c.Cout, 0])
    t = torch.tensor(rows, dtype=torch.int64).to(dev)
    call('dsnt_wgrad_reduce_all', ptr(t), len(rows), max((r[4] // 4 + (r[5] + 3) // 4 + 63) // 64 for r in rows))
    torch.cuda.synchronize()
    # 5. the per-convolution launches: the same body un-grouped (route 0), the halo kernel (route 2), bf16x6
    for c in cases:
        c.w.refill()
        if c.why['route'] == 0:
            call('dsnt_conv_wgrad_f16x3', ptr(c.x), ptr(c.sc), ptr(c.sh), c.relu, ptr(c.gy), ptr(c.w.ws), None, None, 0,
                 ptr(c.ab), ptr(c.gb), C.byref(c.g))
            c.snap_single = c.w.snapshot()
        else:
            assert _lib.fn('dsnt_conv_wgrad_f16x3_ws_floats')(C.byref(c.g), 0) <= c.nws
            c.dw_halo = torch.full((c.Cout, c.k, c.k, c.Cin), float('nan'), device=dev)
            c.db_halo = torch.full((c.Cout,), float('nan'), device=dev)
            call('dsnt_conv_wgrad_f16x3', ptr(c.x), ptr(c.sc), ptr(c.sh), c.relu, ptr(c.gy), ptr(c.w.ws), ptr(c.dw_halo),
                 ptr(c.db_halo), 0, ptr(c.ab), ptr(c.gb), C.byref(c.g))
            c.snap_halo = c.w.snapshot()
    for ci in R.MIXED:
        c = cases[ci]
        c.w6.refill()
        call('dsnt_conv_wgrad_bf16x6', ptr(c.x), ptr(c.sc), ptr(c.sh), c.relu, ptr(c.gy), ptr(c.w6.ws), None, None, 0,
             C.byref(c.g))
        c.snap_single6 = c.w6.snapshot()
    torch.cuda.synchronize()
    return cases


@pytest.fixture(scope='module')
def grouped():
    return _build(raw=False)


@pytest.fixture(scope='module')
def grouped_raw():
    return _build(raw=True)


def _assert_slab_bounds(c, snap):
    lo, ws, hi = snap[:256], snap[256:256 + c.nws], snap[256 + c.nws:]
    assert bool((lo == CANARY).all()) and bool((hi == CANARY).all()), 'a canary around the workspace was overwritten'
    assert bool(torch.isfinite(ws[:c.used]).all()), 'a slab or bias-partial element was never written'
    assert bool(torch.isnan(ws[c.used:]).all()), 'the launch wrote past its own plan of slabs'


def _assert_values(c, dw, db):
    ok, e16, e32, scale = R.bars(dw, c.dw64, c.dw32)
    print('case %s: e16 %.3g  e32(cpu) %.3g  scale %.3g  e16/scale %.3g' % (c.case, e16, e32, scale, e16 / scale))
    assert ok, (e16, e32, scale)
    eb = (db.double().cpu() - c.db64).abs().max().item()
    assert eb <= 3e-5 * c.db64.abs().max().item(), (eb, c.db64.abs().max().item())


@pytest.mark.parametrize('ci', range(len(R.CASES)), ids=IDS)
def test_grouped_f16x3_against_fp64(grouped, ci):
    """The fp16x3 branch of the grouped launch + dsnt_wgrad_reduce_all vs torch.nn.grad.conv2d_weight in float64: e16 <= 3e-5 scale
    and e16 <= max(4 e32, 2e-6 scale), scale = max|dw64|, e32 the error of the CPU float32 reference; bias gradient within
    3e-5 max|db64|.  Every slab element of the plan is written, nothing around it is."""
    c = grouped[ci]
    _assert_slab_bounds(c, c.snap)
    _assert_values(c, c.dw, c.db)


@pytest.mark.parametrize('ci', range(len(R.CASES)), ids=IDS)
def test_grouped_f16x3_raw_operand(grouped_raw, ci):
    """The identity prologue (scale 1, shift 0, no ReLU) on an operand with negative values — conv1 of a BasicBlock: the
    clamp's lower end is -inf, padding rows stay zero.  Same bars; where the un-grouped call runs the same body, its launch
    WITHOUT a prologue writes the same bits."""
    c = grouped_raw[ci]
    _assert_slab_bounds(c, c.snap)
    _assert_values(c, c.dw, c.db)
    if c.why['route'] == 0:
        _assert_slab_bounds(c, c.snap_single)
        assert _same_bits(c.snap, c.snap_single)


def test_padding_workgroups_and_table_order_change_no_bit(grouped):
    """max_blocks 64 above the largest block count, and the same descriptors in reversed table order: the same slabs."""
    for c in grouped:
        _assert_slab_bounds(c, c.snap_padded)
        _assert_slab_bounds(c, c.snap_reversed)
        assert _same_bits(c.snap, c.snap_padded), c.case
        assert _same_bits(c.snap, c.snap_reversed), c.case


def test_grouped_slabs_equal_the_per_convolution_launch(grouped):
    """Route 0: dsnt_conv_wgrad_f16x3(dw = NULL) runs the same body — the same slabs bit for bit.  Route 2 (the 16x16 level):
    the halo kernel is another summation order; both meet the fp64 bars."""
    seen = set()
    for c in grouped:
        seen.add(c.why['route'])
        if c.why['route'] == 0:
            _assert_slab_bounds(c, c.snap_single)
            assert _same_bits(c.snap, c.snap_single), c.case
        else:
            lo, hi = c.snap_halo[:256], c.snap_halo[256 + c.nws:]
            assert bool((lo == CANARY).all()) and bool((hi == CANARY).all())
            _assert_values(c, c.dw_halo, c.db_halo)
            _assert_values(c, c.dw, c.db)
    assert seen == {0, 2}


def test_mixed_f16x3_and_bf16x6_table(grouped):
    """fp16x3 and bf16x6 descriptors alternating in one table (the branch is uniform per table row): every bf16x6 slab equals
    dsnt_conv_wgrad_bf16x6(dw = NULL), every fp16x3 slab the all-fp16x3 launch, bit for bit; the bf16x6 gradients meet the fp64
    bars (bf16x6 splits are relative, so the gradient-sized dy is held to the bars at scale = max|dw64| like fp16x3)."""
    for ci in R.MIXED:
        c = grouped[ci]
        _assert_slab_bounds(c, c.snap_mixed)
        _assert_slab_bounds(c, c.snap_mixed6)
        _assert_slab_bounds(c, c.snap_single6)
        assert _same_bits(c.snap_mixed, c.snap), c.case
        assert _same_bits(c.snap_mixed6, c.snap_single6), c.case
        assert not _same_bits(c.snap_mixed6, c.snap_mixed), 'the two precisions wrote identical slabs: one branch only?'
        _assert_values(c, c.dw6, c.db6)


def test_refusals_launch_nothing():
    from dsnt import _lib
    from dsnt._lib import ptr
    dev = torch.device('cuda:0')
    case = R.CASES[1][0]
    g = _geom(case)
    N, H, W, Cin, Cout = case[:5]
    x, gy = torch.zeros(N, H, W, Cin, device=dev), torch.zeros(N, g.Ho, g.Wo, Cout, device=dev)
    sc, sh, b = torch.ones(Cin, device=dev), torch.zeros(Cin, device=dev), torch.ones(64, device=dev)
    ws = torch.zeros(_lib.fn('dsnt_conv_wgrad_ws_floats')(C.byref(g)) + 4, device=dev)
    desc = C.create_string_buffer(_lib.fn('dsnt_conv_wgrad_desc_bytes')())
    f = _lib.fn('dsnt_conv_wgrad_desc_f16x3')
    assert f(ptr(x), ptr(sc), ptr(sh), 1, ptr(gy), ptr(ws), ptr(b), ptr(b), C.byref(g), desc) > 0
    assert f(ptr(x), ptr(sc), ptr(sh), 1, ptr(gy), ptr(ws), None, ptr(b), C.byref(g), desc) < 0        # null a_bound
    assert f(ptr(x), ptr(sc), ptr(sh), 1, ptr(gy), ptr(ws), ptr(b), None, C.byref(g), desc) < 0        # null g_bound
    assert f(ptr(x), None, None, 1, ptr(gy), ptr(ws), ptr(b), ptr(b), C.byref(g), desc) < 0            # null BN vectors
    assert f(ptr(x), ptr(sc), None, 1, ptr(gy), ptr(ws), ptr(b), ptr(b), C.byref(g), desc) < 0
    assert f(ptr(x), ptr(sc), ptr(sh), 1, ptr(gy), ws.data_ptr() + 4, ptr(b), ptr(b), C.byref(g), desc) < 0    # mis-aligned ws
    g7 = _geom((1, 5, 7, 64, 128, 3, 1, 1, 1))                                                          # Wo = 7
    assert g7.Wo % 4 != 0
    big = torch.zeros(1 << 16, device=dev)
    assert f(ptr(big), ptr(sc), ptr(sh), 1, ptr(big), ptr(big), ptr(b), ptr(b), C.byref(g7), desc) < 0
    t = torch.zeros(len(desc.raw), dtype=torch.uint8, device=dev)
    grp = _lib.fn('dsnt_conv_wgrad_group')
    assert grp(ptr(t), 0, 8, None) != 0
    assert grp(ptr(t), 1, 0, None) != 0
    assert grp(None, 1, 8, None) != 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- dsnt_wgrad_reduce_all alone
SPLITS = [1, 7, 8, 9, 56, 57, 64, 65, 71]
# (CK, Cout): CK / 4 = 180 is no multiple of the 32 columns of a workgroup (the last one holds slab AND bias columns);
# (24, 6): the bias tail with Cout % 4 != 0
SHAPES = [(720, 20), (24, 6)]


def _reduce_blocks(CK, Cout):
    return (CK // 4 + (Cout + 3) // 4 + 63) // 64


def _synthetic_slabs(splits, CK, Cout, dev):
    ws = R.synthetic.tensor('red%d_%d_%d' % (splits, CK, Cout), (splits * CK + splits * Cout,), seed=21)
    return ws, ws.to(dev)


def _reduce_rows(rows, dev, blocks=None):
    from dsnt._lib import ptr, call
    t = torch.tensor(rows, dtype=torch.int64).to(dev)
    call('dsnt_wgrad_reduce_all', ptr(t), len(rows), blocks or max(_reduce_blocks(r[4], r[5]) for r in rows))
    torch.cuda.synchronize()


@pytest.mark.parametrize('CK,Cout', SHAPES)
@pytest.mark.parametrize('splits', SPLITS)
def test_reduce_all_against_fp64_column_sums(splits, CK, Cout):
    """Synthetic slabs, no convolution.  fp32 summation of n terms in any order errs by at most (n - 1) 2^-24 sum|terms|:
    |got - ref64| <= splits 2^-24 sum|terms| per element.  splits > 56 takes the eight-deep unrolled loop, 57 ... 71 its tail.
    With the accumulate column set, the result is old + (the result without) to one fp32 rounding, and exactly it where old
    is zero."""
    dev = torch.device('cuda:0')
    ws, wsd = _synthetic_slabs(splits, CK, Cout, dev)
    slabs, bias = ws[:splits * CK].view(splits, CK).double(), ws[splits * CK:].view(splits, Cout).double()
    dw, db = torch.full((CK,), float('nan'), device=dev), torch.full((Cout + 2,), CANARY, device=dev)
    _reduce_rows([[wsd.data_ptr(), dw.data_ptr(), db.data_ptr(), splits, CK, Cout, 0]], dev)
    bound = splits * 2.0 ** -24
    assert bool(((dw.cpu().double() - slabs.sum(0)).abs() <= bound * slabs.abs().sum(0)).all())
    assert bool(((db[:Cout].cpu().double() - bias.sum(0)).abs() <= bound * bias.abs().sum(0)).all())
    assert bool((db[Cout:] == CANARY).all()), 'the bias tail wrote past Cout'
    # accumulate: onto `old` (zero in every other element)
    old_w = R.synthetic.tensor('redow%d_%d' % (splits, CK), (CK,), seed=22)
    old_b = R.synthetic.tensor('redob%d_%d' % (splits, Cout), (Cout + 2,), seed=22)
    old_w[::2] = 0.0
    old_b[::2] = 0.0
    dw2, db2 = old_w.to(dev), old_b.to(dev)
    _reduce_rows([[wsd.data_ptr(), dw2.data_ptr(), db2.data_ptr(), splits, CK, Cout, 1]], dev)
    for got, plain, old in ((dw2, dw, old_w), (db2[:Cout], db[:Cout], old_b[:Cout])):
        got, want = got.cpu().double(), old.double() + plain.cpu().double()
        assert bool(((got - want).abs() <= 2.0 ** -24 * want.abs()).all())
        zero = old == 0
        assert torch.equal(got[zero], plain.cpu().double()[zero])
    assert torch.equal(db2[Cout:].cpu(), old_b[Cout:])


def test_reduce_all_rows_are_independent():
    """Several rows of different splits and CK in one launch (max_blocks = the largest row's count, one row without dbias):
    each row equals its own single-row launch bit for bit, the row without dbias leaves its bias alone."""
    dev = torch.device('cuda:0')
    shapes = [(9, 720, 20), (65, 24, 6), (57, 4608, 64), (1, 2048, 16), (8, 720, 20)]
    no_bias = 2
    keep, rows, single = [], [], []
    for i, (splits, CK, Cout) in enumerate(shapes):
        _, wsd = _synthetic_slabs(splits, CK, Cout, dev)
        dw, db = torch.full((CK,), float('nan'), device=dev), torch.full((Cout,), CANARY, device=dev)
        dw1, db1 = torch.full((CK,), float('nan'), device=dev), torch.full((Cout,), CANARY, device=dev)
        rows.append([wsd.data_ptr(), dw.data_ptr(), 0 if i == no_bias else db.data_ptr(), splits, CK, Cout, 0])
        _reduce_rows([[wsd.data_ptr(), dw1.data_ptr(), db1.data_ptr(), splits, CK, Cout, 0]], dev)
        keep.append(wsd)
        single.append((dw, db, dw1, db1))
    assert len({_reduce_blocks(CK, Cout) for _, CK, Cout in shapes}) > 2
    _reduce_rows(rows, dev)
    for i, (dw, db, dw1, db1) in enumerate(single):
        assert bool(torch.isfinite(dw1).all()) and _same_bits(dw, dw1), shapes[i]
        if i == no_bias:
            assert bool((db == CANARY).all()) and bool(torch.isfinite(db1).all()) and not bool((db1 == CANARY).any())
        else:
            assert _same_bits(db, db1), shapes[i]


# ------------------------------------------------------------------------------- dsnt_bn_eval_prep vs dsnt_bn_finalize(training = 0)
def test_bn_eval_prep_against_finalize_and_fp64():
    """Four table rows (C = 16, 256, 300: the second trip of the 256-thread loop, 10: no multiple of 4; one row without gamma and
    beta; running variances that include 0 and 1e-12; eps = 1e-5): mean, invstd, scale and shift of the one launch are
    bit-identical to the per-layer dsnt_bn_finalize(training = 0), and both lie within 1 ulp (fp32) of 1 / sqrt(var + eps) in
    float64, scale and shift within 2 ulp of gamma invstd and beta - mean gamma invstd in float64.

    An ulp bound on a DIFFERENCE of two fp32 quantities only means something where they do not cancel, so the running means
    carry the sign that makes beta and -mean scale add (gamma > 0)."""
    from dsnt._lib import ptr, call
    dev = torch.device('cuda:0')
    eps = np.float32(1e-5)
    eps_bits = struct.unpack('<I', struct.pack('<f', float(eps)))[0]
    Cs, bare = [16, 256, 300, 10], 2
    rows, layers = [], []
    for i, Cc in enumerate(Cs):
        gamma = synthetic_uniform('evg%d' % i, Cc) + 1.5
        beta = R.synthetic.tensor('evb%d' % i, (Cc,), seed=31, scale=0.2)
        rv = synthetic_uniform('evv%d' % i, Cc).abs() * 2.0 + 1e-3
        rv[0], rv[1], rv[Cc - 1] = 0.0, 1e-12, 1e-12
        rm = R.synthetic.tensor('evm%d' % i, (Cc,), seed=31).abs() * -torch.sign(beta)
        if i == bare:
            gamma = beta = None
        assert gamma is None or bool((gamma > 0).all())
        dv = [None if t is None else t.to(dev) for t in (gamma, beta, rm, rv)]
        out = [torch.full((Cc + 2,), CANARY, device=dev) for _ in range(4)]
        fin = [torch.full((Cc + 2,), CANARY, device=dev) for _ in range(4)]
        rows.append([0 if t is None else t.data_ptr() for t in dv] + [t.data_ptr() for t in out] + [Cc, eps_bits])
        call('dsnt_bn_finalize', None, 0, 1, Cc, ptr(dv[0]), ptr(dv[1]), ptr(dv[2]), ptr(dv[3]), 0.1, float(eps), 0,
             ptr(fin[0]), ptr(fin[1]), ptr(fin[2]), ptr(fin[3]))
        layers.append((Cc, gamma, beta, rm, rv, dv, out, fin))
    t = torch.tensor(rows, dtype=torch.int64).to(dev)
    call('dsnt_bn_eval_prep', ptr(t), len(rows))
    torch.cuda.synchronize()
    names = ('mean', 'invstd', 'scale', 'shift')
    for Cc, gamma, beta, rm, rv, dv, out, fin in layers:
        assert torch.equal(dv[2].cpu(), rm) and torch.equal(dv[3].cpu(), rv)         # eval mode leaves the running statistics
        is64 = 1.0 / np.sqrt(rv.double().numpy() + np.float64(eps))
        g64 = np.ones(Cc) if gamma is None else gamma.double().numpy()
        b64 = np.zeros(Cc) if beta is None else beta.double().numpy()
        sc64 = g64 * is64
        ref = (rm.double().numpy(), is64, sc64, b64 - rm.double().numpy() * sc64)
        for name, ulps, r64, a, b in zip(names, (0, 1, 2, 2), ref, out, fin):
            assert bool((a[Cc:] == CANARY).all()) and bool((b[Cc:] == CANARY).all()), name + ': wrote past C'
            for who, got in (('dsnt_bn_eval_prep', a), ('dsnt_bn_finalize', b)):
                err = np.abs(got[:Cc].cpu().double().numpy() - r64) / R.ulp32(r64)
                print('C %d %s %s: worst %.3f ulp' % (Cc, who, name, err.max()))
                assert bool((err <= ulps).all()), (Cc, who, name, float(err.max()))
            assert _same_bits(a, b), (Cc, name)


def synthetic_uniform(tag, n):
    return R.synthetic.tensor(tag, (n,), seed=31, kind='uniform')
