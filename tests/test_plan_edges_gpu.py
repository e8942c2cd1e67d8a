"""The fp16x3 streaming convolution kernels at the edges of what their host plans accept (tests/plan_edge_cases.py): slabs of 9 /
13 / 17 stages and short last slabs (wgrad1), persistent workgroups that run a second, ragged iteration (gemm1), one-stage
workgroups and one-stage tails (fwd1, bwd1), odd / tiny / non-power-of-two heights and three strips (wgrad3), 27 K-step pairs and a
one-patch-row image (conv3s), non-square stem tiles (stem4).

Every test first holds tests/plan_ref.py — the plans restated in Python — to what the C ABI reports on this device, then asserts
the edge from the restatement (the edges are stated for 256 CUs: on another device the assertion names the premise that moved),
then runs the comparison of tests/test_conv_gpu.py / tests/test_bwd1_gpu.py for that kernel (tests/conv_checks.py: the same code,
the same bars against fp64)."""
import ctypes as C

import pytest
import torch

import conv_checks as K
import plan_edge_cases as E
import plan_ref as P

pytestmark = pytest.mark.gpu

SHARE = 2           # DSNT_CONV_SHARE_CHIP == DSNT_WGRAD_SHARE_CHIP
NARROW = 4          # DSNT_WGRAD_NARROW


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _abi(name, *args):
    from dsnt import _lib
    return _lib.fn(name)(*args)


def _g1(case):
    return K.geom(*case, 1, 1, 1, 0, 1)


def _g3(case):
    return K.geom(*case, 3, 3, 1, 1, 1)


def _report(family, case, what, figs):
    print('plan-edge %s %s %s: %s' % (family, case, what, ' '.join(
        '%s=%.3g' % kv if isinstance(kv[1], float) else '%s=%s' % kv for kv in sorted(figs.items()))))


def _edge(ok, family, case, **numbers):
    assert ok, 'the %s edge of %s is stated for 256 CUs; on this device (%d CUs) the plan gives %s' % (family, case, _cus(), numbers)


@pytest.mark.parametrize('case', E.WGRAD1)
def test_wgrad1_slabs_of_every_length(case):
    g, cus = _g1(case), _cus()
    N, H, W, Cin, Cout = case
    pl, sh = P.wgrad1(case, cus), P.wgrad1(case, cus, share=True)
    assert _abi('dsnt_conv_f16x3_route', C.byref(g), 1) == P.route(case, 1, True) == 3
    for flags, p in ((0, pl), (SHARE, sh)):
        assert _abi('dsnt_conv_wgrad_f16x3_splits', C.byref(g), flags) == p['nsplits'], (case, flags, p)
        assert _abi('dsnt_conv_wgrad_f16x3_ws_floats', C.byref(g), flags) == p['nsplits'] * Cout * (Cin + 1), (case, flags, p)
    edges = {
        (1, 25, 656, 128, 128): pl['nstages'] % 3 == 0 and pl['last_stages'] == 8,
        (1, 79, 208, 128, 128): pl['last_stages'] == 1,
        (1, 257, 64, 128, 128): pl['last_stages'] == 2,
        (1, 41, 400, 64, 256): pl['nchunks'] == 2 and (sh['nstages'], sh['last_stages']) == (17, 5),
        (1, 129, 128, 192, 64): pl['kchunks'] == 3 and pl['nstages'] % 3 == 1 and pl['last_stages'] == 5,
        (1, 130, 128, 256, 64): (pl['ck'], pl['cn'], pl['kchunks']) == (128, 64, 2) and sh['last_stages'] == 3,
    }
    _edge(edges[case], 'wgrad1', case, plain=pl, share=sh)
    for pro, relu in ((True, 1), (False, 0)):
        _report('wgrad1', case, 'pro=%d' % pro, K.wgrad_1x1_f16x3(case, pro, relu))


@pytest.mark.parametrize('case,share', E.GEMM1)
def test_gemm1_grid_stride_loop(case, share):
    g, cus = _g1(case), _cus()
    pl = P.gemm1(case, cus, share)
    assert _abi('dsnt_conv_f16x3_route', C.byref(g), 0) == P.route(case, 1, False) == 1
    _edge(pl['niter'] > pl['grid'] and (pl['niter'] % pl['grid'] != 0 or case[4] == 512), 'gemm1', case, **pl)
    want = {(131, 16, 32, 64, 256): (4, 2), (129, 16, 32, 128, 512): (8, 2), (66, 32, 32, 128, 192): (2, 3)}.get(case, (8, 1))
    assert (pl['ntw'], pl['chunks']) == want, (case, pl)
    flags = SHARE if share else 0
    # bias + residual + the M / 128-row statistics partial in both; the BatchNorm prologue under a 64x loose operand bound
    _report('gemm1', case, 'plain', K.conv_f16x3_vs_fp32_accuracy(case + (1, 1, 0, 1), False, 1.0, flags))
    _report('gemm1', case, 'pro', K.conv_f16x3_vs_fp32_accuracy(case + (1, 1, 0, 1), True, 64.0, flags))


FWD1 = E.FWD1_ONE_STAGE + E.FWD1_SHORT_LAST_SHARE + E.FWD1_SHORT_LAST


@pytest.mark.parametrize('case', FWD1)
def test_fwd1_one_stage_workgroups_and_tails(case):
    g, cus = _g1(case), _cus()
    pl, sh = P.fwd1(case, cus), P.fwd1(case, cus, share=True)
    assert _abi('dsnt_conv1x1_fwd_ok', C.byref(g)) == 1
    assert _abi('dsnt_conv1x1_fwd_stats_rows', C.byref(g), 0) == pl['nwg'], (case, pl)
    assert _abi('dsnt_conv1x1_fwd_stats_rows', C.byref(g), SHARE) == sh['nwg'], (case, sh)
    if case in E.FWD1_ONE_STAGE:
        _edge(pl['spw'] == 1, 'fwd1', case, **pl)
    elif case in E.FWD1_SHORT_LAST:
        _edge((pl['spw'], pl['last']) == (2, 1), 'fwd1', case, **pl)
    else:       # 129 stages: one each; under the share flag (which the comparison also runs) the eight-wave pair has two and a last of one
        _edge(pl['spw'] == 1 and ((sh['spw'], sh['last']) == (2, 1) or pl['waves'] == 4), 'fwd1', case, plain=pl, share=sh)
    for pro, res in ((True, True), (True, False), (False, True), (False, False)):
        _report('fwd1', case, 'pro=%d res=%d' % (pro, res), K.conv1x1_forward_lds_staged(case, pro, res))


def test_fwd1_fused_shortcut_launch_at_129_stages():
    """dsnt_conv1x1_fwd_ds_f16x3 (conv3 + projection shortcut in one launch, 128 -> 256) on 129 stages — one per workgroup, and under
    the share flag two per workgroup with a last of one: bit for bit the pair of launches, and the per-channel fp32 bar against fp64
    (the checks of tests/test_shortcut_fused_gpu.py)."""
    import f16x3_util as U
    import shortcut_fused_util as S
    Cin, Cout, M = 128, 256, 32 * E.FWD1_DS_STAGES
    case, cus = (1, M // 32, 32, Cin, Cout), _cus()
    pl, sh = P.fwd1(case, cus), P.fwd1(case, cus, share=True)
    assert (Cin, Cout) in P.FWD1_DS_PAIRS
    _edge(pl['spw'] == 1 and (sh['spw'], sh['last']) == (2, 1), 'fwd1 (fused shortcut)', case, plain=pl, share=sh)
    r64, r32 = S.forward_refs(Cin, Cout, M)
    for flags, p in ((0, pl), (SHARE, sh)):
        pair, fused, rows = S.forward(Cin, Cout, M, flags)
        assert rows == p['nwg'], (flags, rows, p)
        assert bool(torch.isfinite(fused['out']).all()) and bool(torch.isfinite(fused['stats']).all())
        for k in ('out', 'stats', 'amax', 'amax_bn'):
            assert torch.equal(pair[k], fused[k]), (flags, k)
        fails = U.per_channel('fwd_ds %d->%d flags %d' % (Cin, Cout, flags), fused['out'], r64, r32, -1)
        assert not fails, fails
        s = fused['stats'].double().sum(0).cpu()
        assert ((s[0] - r64.sum(0)).abs() <= 1e-5 * r64.abs().sum(0)).all()
        assert ((s[1] - (r64 * r64).sum(0)).abs() <= 1e-5 * (r64 * r64).sum(0)).all()


@pytest.mark.parametrize('case', E.BWD1_ONE_STAGE + E.BWD1_SHORT_LAST)
def test_bwd1_one_stage_workgroups_and_tails(case):
    g, cus = _g1(case), _cus()
    pl, sh = P.bwd1(case, cus), P.bwd1(case, cus, share=True)
    assert _abi('dsnt_conv1x1_bwd_ok', C.byref(g)) == 1
    assert _abi('dsnt_conv1x1_bwd_splits', C.byref(g), 0) == pl['nwg'], (case, pl)
    assert _abi('dsnt_conv1x1_bwd_splits', C.byref(g), SHARE) == sh['nwg'], (case, sh)
    if case in E.BWD1_ONE_STAGE:
        _edge(pl['waves'] == 4 and pl['spw'] == 1, 'bwd1', case, **pl)
    elif pl['waves'] == 8:
        _edge((pl['spw'], pl['last']) == (3, 1), 'bwd1', case, **pl)
    else:
        _edge((pl['spw'], pl['nwg'], pl['last']) == (2, 257, 2), 'bwd1', case, **pl)
    for mode, relu in (('apply', 1), ('given', 1), ('apply', 0), ('raw', 0), ('raw_acc', 0)):
        _report('bwd1', case, '%s relu=%d' % (mode, relu), K.conv1x1_backward_in_one_pass(case, mode, relu))


@pytest.mark.parametrize('case', E.WGRAD3)
def test_wgrad3_heights_strips_and_chunks(case):
    g, cus = _g3(case), _cus()
    N, H, W, Cin, Cout = case
    assert _abi('dsnt_conv_wgrad_halo_ok', C.byref(g)) == 1
    assert _abi('dsnt_conv_f16x3_route', C.byref(g), 1) == P.route(case, 3, True) == 2
    for flags, share in ((0, 0), (SHARE, 1), (SHARE | NARROW, 2)):
        p = P.wgrad3(case, cus, share)
        assert _abi('dsnt_conv_wgrad_f16x3_splits', C.byref(g), flags) == p['nslabs'], (case, flags, p)
        assert _abi('dsnt_conv_wgrad_f16x3_ws_floats', C.byref(g), flags) == p['nslabs'] * Cout * (9 * Cin + 1), (case, flags, p)
    pl = P.wgrad3(case, cus)
    edges = {
        (1, 24, 64, 64, 128): pl['rps'] == 12, (1, 40, 64, 64, 64): pl['rps'] == 10,
        (2, 5, 16, 64, 64): (pl['rps'], pl['hsplits']) == (5, 1), (1, 3, 64, 128, 64): (pl['rps'], pl['hsplits']) == (3, 1),
        (1, 1, 32, 64, 128): pl['rps'] == 1, (1, 2, 16, 64, 64): pl['rps'] == 2,
        (1, 16, 192, 64, 192): (pl['strips'], pl['nchunks'], pl['cfg']) == (3, 3, 1),
        (1, 48, 32, 192, 128): (pl['kchunks'], pl['rps']) == (3, 24),
    }
    _edge(edges[case], 'wgrad3', case, **pl)
    for pro, relu in ((True, 1), (True, 0), (False, 0)):
        _report('wgrad3', case, 'pro=%d relu=%d' % (pro, relu), K.wgrad_halo_f16x3(case, pro, relu))


STREAM_MODES = ['plain', 'pro', 'pro_res', 'res', 'bnb', 'pro_norelu', 'bnb_norelu']


@pytest.mark.parametrize('case', E.CONV3S_CIN96 + [E.CONV3S_ONE_ROW])
def test_conv3s_27_pairs_and_one_patch_row(case):
    g, cus = _g3(case), _cus()
    assert _abi('dsnt_conv_fwd_stream_ok', C.byref(g)) == 1
    assert _abi('dsnt_conv_f16x3_route', C.byref(g), 0) == P.route(case, 3, False)
    forms = {}
    for mode in (0, 1, 3, 4):
        forms[mode] = P.conv3s(case, cus, mode)['form']
        assert _abi('dsnt_conv_fwd_stream_form', C.byref(g), mode) == forms[mode], (case, mode, forms)
    pl = P.conv3s(case, cus)
    print('plan-edge conv3s %s forms (mode: form) %s, %d patches' % (case, forms, pl['ntiles']))
    if case == E.CONV3S_ONE_ROW:
        assert pl['patch_rows'] == 1 and forms[0] == 0
    else:
        assert pl['kpairs'] == 27
        want = {(2, 8, 32, 96, 64): (0, 0, 0), (1, 8, 16, 96, 128): (5, 5, 4), (3, 16, 32, 96, 128): (1, 1, 0)}[case]
        _edge((forms[0], forms[3], forms[4]) == want, 'conv3s', case, forms=forms, patches=pl['ntiles'])
    for mode in STREAM_MODES:           # MODE 0 / 1 (plain, pro; res, pro_res) and MODE 3 (bnb)
        _report('conv3s', case, mode, K.conv3_stream_kernel(case, mode))
    if case in E.CONV3S_CIN96:          # MODE 4: the 27-pair path through the two-slot ring, BatchNorm backward folded in
        for relu, big_mean in ((1, False), (0, False), (1, True)):
            _report('conv3s', case, 'dgrad_apply relu=%d big_mean=%d' % (relu, big_mean), K.conv3_stream_dgrad_apply(case, relu, big_mean))


@pytest.mark.parametrize('N,Ho,Wo', E.STEM4)
def test_stem4_tiles_of_a_non_square_image(N, Ho, Wo):
    from dsnt._lib import ConvGeom
    cus = _cus()
    g = ConvGeom(N, Ho + 1, Wo + 1, 16, Ho, Wo, 64, 4, 4, 1, 1, 1)
    pl = P.stem4((N, Ho, Wo), cus)
    assert _abi('dsnt_stem4_fwd_ok', C.byref(g)) == 1
    assert _abi('dsnt_stem4_fwd_stats_rows', C.byref(g)) == pl['grid'], pl
    assert _abi('dsnt_conv_wgrad_f16x3_splits', C.byref(g), 0) == pl['wgrad_grid'], pl
    assert _abi('dsnt_conv_wgrad_f16x3_ws_floats', C.byref(g), 0) == pl['wgrad_grid'] * (64 * 256 + 64), pl
    assert _abi('dsnt_conv_f16x3_route', C.byref(g), 1) == P.route((N, Ho, Wo), 4, True, stem=True) == 1
    assert Ho != Wo and pl['tiles'] == N * pl['tile_rows'] * pl['tile_cols'], pl
    for with_bias in (True, False):
        _report('stem4 fwd', (N, Ho, Wo), 'bias=%d' % with_bias, K.stem_forward_on_its_halo_kernel(N, Ho, Wo, with_bias))
    _report('stem4 wgrad', (N, Ho, Wo), '', K.stem_weight_gradient_on_its_own_kernel(N, Ho, Wo))


def test_refusals_at_the_borders_of_the_plans():
    """What lies just outside the families above is refused: 0 from the `_ok`, a plan of 0 rows / the generic route from the
    queries, and an error (no launch) from the entry point."""
    from dsnt import _lib
    from dsnt._lib import ConvGeom
    fwd_ok = _lib.fn('dsnt_conv1x1_fwd_ok')
    assert fwd_ok(C.byref(_g1((1, 64, 64, 128, 256))))                    # 4096 rows: the smallest
    bad = [_g1((1, 127, 32, 128, 256)),                                   # 4064 rows
           _g1((1, 129, 48, 128, 256)),                                   # 6192 rows: not whole 32-row stages
           _g1((1, 64, 64, 128, 192)),                                    # a channel pair without a configuration
           _g3((1, 64, 64, 128, 256))]                                    # 3x3
    for g in bad:
        assert not fwd_ok(C.byref(g)) and (g.R == 3 or P.fwd1((g.N, g.H, g.W, g.Cin, g.Cout)) is None)
        assert _lib.fn('dsnt_conv1x1_fwd_stats_rows')(C.byref(g), 0) == 0
    X = C.c_void_p(4096)                       # never followed: refused before a launch
    rc = _lib.fn('dsnt_conv1x1_fwd_f16x3')(X, X, 8192, X, X, X, X, None, None, 0, None, None, C.byref(bad[0]), None, None)
    assert rc == 1 and b'dsnt_conv1x1_fwd_f16x3' in _lib.load().dsnt_last_error()
    # the streaming 1x1 kernel and the 1x1 / halo weight gradients: the route falls back to the tiled / generic kernel
    route = _lib.fn('dsnt_conv_f16x3_route')
    for case in [(255, 16, 16, 128, 256), (257, 16, 16, 64, 128), (259, 16, 16, 128, 96), (259, 16, 16, 192, 256)]:
        assert P.gemm1(case) is None and route(C.byref(_g1(case)), 0) == 0, case
    for case in [(1, 127, 128, 128, 128), (1, 129, 136, 128, 128), (1, 128, 128, 96, 128)]:
        assert P.wgrad1(case) is None and route(C.byref(_g1(case)), 1) == 0, case
    for case in [(1, 16, 48, 64, 64), (1, 16, 160, 64, 64), (1, 16, 64, 96, 64), (1, 16, 8, 64, 64)]:
        assert P.wgrad3(case) is None and _lib.fn('dsnt_conv_wgrad_halo_ok')(C.byref(_g3(case))) == 0, case
        assert route(C.byref(_g3(case)), 1) == 0, case
    # the stem: Ho % 4, Wo % 32
    for N, Ho, Wo in [(1, 6, 32), (1, 4, 48), (1, 2, 32)]:
        g = ConvGeom(N, Ho + 1, Wo + 1, 16, Ho, Wo, 64, 4, 4, 1, 1, 1)
        assert P.stem4((N, Ho, Wo)) is None and _lib.fn('dsnt_stem4_fwd_ok')(C.byref(g)) == 0
        assert _lib.fn('dsnt_stem4_fwd_stats_rows')(C.byref(g)) == 0
        assert _lib.fn('dsnt_stem4_fwd_f16x3')(X, X, 64 * 256, X, X, None, X, None, C.byref(g), None, None) == 1
