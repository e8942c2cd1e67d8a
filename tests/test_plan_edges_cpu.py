"""The cases of tests/test_plan_edges_gpu.py hold what they claim: on 256 CUs each one hits the plan edge it is listed for
(tests/plan_ref.py restates the host plans of the fp16x3 streaming kernels), and the case lists of tests/test_conv_gpu.py never
reached those edges — every 1x1 weight-gradient slab there is eight equal stages, every streaming 1x1 workgroup runs one
iteration.  No GPU: tests/test_plan_edges_gpu.py holds plan_ref itself to the C ABI on the device.

The same for the fp32 family of csrc/conv_f32.hip (plan_ref.conv_f32, plan_edge_cases.CONV_F32, run by
tests/test_conv_f32_edges_gpu.py): which tile shape, loader, K-step count and K-split chunk counts each case lands on, and
that the fp32 launches of tests/test_conv_gpu.py reach none of them.

And for the tiled split-precision kernels of csrc/conv_split6.hip (plan_ref.conv_split, plan_edge_cases.CONV_SPLIT, run by
tests/test_conv_split_edges_gpu.py): kernel, tile width, K-steps or chunks, LDS request and prologue trips of each case, and
which of those edges BF16X6_CASES of tests/test_conv_gpu.py did and did not reach."""
import ast
import os

import plan_ref as P
import plan_edge_cases as E

CUS = 256


def _literal(path, name):
    """A module-level list literal of a test module, read without importing it (the module needs torch and a GPU marker)."""
    tree = ast.parse(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), path)).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], 'id', None) == name:
            if isinstance(node.value, ast.BinOp):             # BF16X6_CASES = [comprehension over CASES] + [literal]
                return ast.literal_eval(node.value.right)
            return ast.literal_eval(node.value)
    raise KeyError(name)


def test_the_existing_wgrad1_cases_only_ever_planned_eight_equal_stages():
    cases = _literal('test_conv_gpu.py', 'W1_CASES')
    assert len(cases) == 8 and (5, 64, 64, 128, 256) in cases
    for case in cases:
        pl = P.wgrad1(case, CUS)
        assert pl['rows_per_split'] == 128 and pl['nstages'] == 8 and pl['last_rows'] == 128, (case, pl)     # 8 = 2 (mod 3), no short slab
        assert pl['nchunks'] == 1 and pl['kchunks'] <= 2, (case, pl)
        sh = P.wgrad1(case, CUS, share=True)
        assert sh['last_rows'] == sh['rows_per_split'] and sh['nstages'] in (8, 10, 16), (case, sh)          # 2, 1, 1 (mod 3): never 0
    assert P.wgrad1((5, 64, 64, 128, 256), CUS)['nsplits'] == 160


def test_the_existing_gemm1_cases_run_one_iteration_per_workgroup():
    cases = [c[:5] for c in _literal('test_conv_gpu.py', 'BF16X6_CASES') if c[5] == 1 and P.gemm1(c[:5], CUS)]
    assert len(cases) == 7
    for case in cases:
        pl = P.gemm1(case, CUS)
        assert pl['niter'] == pl['grid'] and pl['chunks'] <= 2, (case, pl)
        assert not (case[3] == 64 and pl['chunks'] == 2) and not (case[3] == 128 and case[4] == 512)


def test_the_existing_stage_kernels_cases_never_ran_a_one_stage_workgroup():
    for case in _literal('test_bwd1_gpu.py', 'FWD_CASES'):
        pl = P.fwd1(case, CUS)
        assert pl['spw'] in (2, 3, 4) and not (pl['spw'] == 2 and pl['last'] == 1), (case, pl)
    for case in _literal('test_bwd1_gpu.py', 'CASES'):
        assert P.bwd1(case, CUS)['spw'] >= 2, case


def test_the_existing_halo_and_stream_and_stem_cases_miss_the_new_edges():
    for case in _literal('test_conv_gpu.py', 'HALO_CASES'):
        pl = P.wgrad3(case, CUS)
        assert case[1] in (8, 16, 32, 64, 128) and pl['rps'] & (pl['rps'] - 1) == 0 and pl['strips'] <= 2 and pl['kchunks'] != 3
        assert not (pl['cfg'] == 1 and pl['nchunks'] == 3)
    for case in _literal('test_conv_gpu.py', 'STREAM_CASES'):
        assert case[3] != 96 and not (case[1] == 4 and case[4] == 64 and case[3] == 64)
    assert all(len(c) == 2 for c in _literal('test_bwd1_gpu.py', 'STEM_CASES'))           # (N, Ho): square


def test_wgrad1_cases_hit_their_edges():
    want = {
        (1, 25, 656, 128, 128): dict(nsplits=114, nstages=9, last_stages=8),               # 9 = 0 (mod 3)
        (1, 79, 208, 128, 128): dict(last_stages=1),
        (1, 257, 64, 128, 128): dict(last_stages=2),
        (1, 41, 400, 64, 256): dict(nchunks=2),
        (1, 129, 128, 192, 64): dict(kchunks=3, nstages=13, last_stages=5),                # 13 = 1 (mod 3)
        (1, 130, 128, 256, 64): dict(ck=128, cn=64, kchunks=2),
    }
    share = {
        (1, 41, 400, 64, 256): dict(nsplits=61, nstages=17, last_stages=5),
        (1, 130, 128, 256, 64): dict(last_stages=3),                                       # the loop once, no tail
    }
    assert sorted(want) == sorted(E.WGRAD1)
    for case in E.WGRAD1:
        pl = P.wgrad1(case, CUS)
        assert pl and all(pl[k] == v for k, v in want[case].items()), (case, pl)
        assert pl['last_rows'] < pl['rows_per_split'] or case in share, (case, pl)
        if case in share:
            sh = P.wgrad1(case, CUS, share=True)
            assert all(sh[k] == v for k, v in share[case].items()), (case, sh)
    assert {P.wgrad1(c, CUS)['nstages'] % 3 for c in E.WGRAD1} | {P.wgrad1(c, CUS, True)['nstages'] % 3 for c in share} == {0, 1, 2}


def test_gemm1_cases_hit_their_edges():
    want = {
        (259, 16, 16, 128, 256): (dict(niter=259, grid=256, chunks=1), False),             # three workgroups run a second iteration
        (131, 16, 32, 64, 256): (dict(niter=131, grid=128, chunks=2, ntw=4), False),
        (129, 16, 32, 128, 512): (dict(niter=258, grid=128, chunks=2, ntw=8), False),
        (66, 32, 32, 128, 192): (dict(niter=66, grid=42, chunks=3, ntw=2), True),
    }
    assert sorted((c, s) for c, (_, s) in want.items()) == sorted(E.GEMM1)
    for case, (figs, share) in want.items():
        pl = P.gemm1(case, CUS, share)
        assert pl and all(pl[k] == v for k, v in figs.items()), (case, pl)
        assert pl['niter'] > pl['grid'] and (pl['niter'] % pl['grid'] != 0 or case[4] == 512), (case, pl)
        assert case[0] * case[1] * case[2] <= 67 * 1024
    assert P.gemm1((66, 32, 32, 128, 192), CUS)['grid'] == 66                               # (without the share flag: one iteration each)


def test_fwd1_and_bwd1_cases_hit_their_edges():
    assert sorted(c[3:] for c in E.FWD1_ONE_STAGE) == sorted(c[:2] for c in P.F1_CFGS)
    for case in E.FWD1_ONE_STAGE:
        pl = P.fwd1(case, CUS)
        assert pl['spw'] == 1 and pl['nstages'] == 128 and pl['nwg'] == 128, (case, pl)
    assert P.fwd1((1, 64, 64, 256, 256), CUS)['chunks'] == 2
    for case in E.FWD1_SHORT_LAST_SHARE:
        pl, sh = P.fwd1(case, CUS), P.fwd1(case, CUS, share=True)
        assert pl['nstages'] == 129 and pl['spw'] == 1, (case, pl)
        if pl['waves'] == 8:
            assert (sh['spw'], sh['nwg'], sh['last']) == (2, 65, 1), (case, sh)
        else:               # 64 -> 64 runs four-wave workgroups, two per CU: 256 of them under the share flag too, one stage each
            assert (sh['spw'], sh['nwg']) == (1, 129), (case, sh)
    for case in E.FWD1_SHORT_LAST:
        pl = P.fwd1(case, CUS)
        assert (pl['nstages'], pl['spw'], pl['nwg'], pl['last']) == (257, 2, 129, 1), (case, pl)
    for case in E.BWD1_ONE_STAGE:
        pl = P.bwd1(case, CUS)
        assert pl['waves'] == 4 and pl['nstages'] == 512 and pl['spw'] == 1, (case, pl)
    want = {(1, 257, 64, 256, 128): (3, 172, 1), (1, 257, 64, 64, 64): (2, 257, 2)}
    assert sorted(want) == sorted(E.BWD1_SHORT_LAST)
    for case, figs in want.items():
        pl = P.bwd1(case, CUS)
        assert pl['nstages'] == 514 and (pl['spw'], pl['nwg'], pl['last']) == figs, (case, pl)


def test_wgrad3_cases_hit_their_edges():
    want = {
        (1, 24, 64, 64, 128): dict(rps=12), (1, 40, 64, 64, 64): dict(rps=10),
        (2, 5, 16, 64, 64): dict(rps=5, hsplits=1), (1, 3, 64, 128, 64): dict(rps=3, hsplits=1),
        (1, 1, 32, 64, 128): dict(rps=1), (1, 2, 16, 64, 64): dict(rps=2),
        (1, 16, 192, 64, 192): dict(strips=3, nchunks=3, cfg=1),
        (1, 48, 32, 192, 128): dict(kchunks=3, rps=24),
    }
    assert sorted(want) == sorted(E.WGRAD3)
    for case, figs in want.items():
        pl = P.wgrad3(case, CUS)
        assert pl and all(pl[k] == v for k, v in figs.items()), (case, pl)
        assert pl['rps'] * pl['hsplits'] == case[1]
    assert sum(1 for c in E.WGRAD3 if c[1] < 3) == 2 and sum(1 for c in E.WGRAD3 if c[1] % 2) == 3


def test_conv3s_and_stem_cases_hit_their_edges():
    forms = {}
    for case in E.CONV3S_CIN96:
        pl = P.conv3s(case, CUS)
        assert pl and pl['kpairs'] == 27 and case[3] == 96, (case, pl)
        forms[case] = tuple(P.conv3s(case, CUS, m)['form'] for m in (0, 3, 4))
    # forward / BatchNorm-backward epilogue / folded BatchNorm backward: 4 x 32 patches; 8 x 16 patches split into column halves (the
    # folded form never splits); 4 x 32 patches, 128 columns — split into halves on its 12 patches, whole in the folded form
    assert forms == {(2, 8, 32, 96, 64): (0, 0, 0), (1, 8, 16, 96, 128): (5, 5, 4), (3, 16, 32, 96, 128): (1, 1, 0)}
    pl = P.conv3s(E.CONV3S_ONE_ROW, CUS)
    assert pl['patch_rows'] == 1 and pl['form'] == 0 and E.CONV3S_ONE_ROW[1] == 4
    for case in E.STEM4:
        pl = P.stem4(case, CUS)
        assert pl and case[1] != case[2], (case, pl)
    assert P.stem4((1, 4, 32), CUS)['tiles'] == 1
    assert {c[1] > c[2] for c in E.STEM4} == {True, False}                                               # a tall image and wide ones
    assert {(P.stem4(c)['tile_rows'] > P.stem4(c)['tile_cols']) for c in E.STEM4} == {True, False}      # ... in tiles too


def _parametrized(path, func, argnames):
    """The literal list of the `pytest.mark.parametrize(argnames, [...])` decorator of a test function, read like _literal."""
    tree = ast.parse(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), path)).read())
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == func:
            for dec in node.decorator_list:
                if isinstance(dec, ast.Call) and dec.args and ast.literal_eval(dec.args[0]) == argnames:
                    return ast.literal_eval(dec.args[1])
    raise KeyError((func, argnames))


def _existing_f32_launches():
    """Every dsnt_conv_fwd / _ex / _pro launch on the fp32 path that tests/test_conv_gpu.py holds to a reference of its own, as
    (what, case, pro, amax) with case = (N, H, W, Cin, Cout, k, stride, pad, dil) of the LAUNCH: test_conv_fwd_wgrad_dgrad (CASES,
    both `pro`, and the data gradient of the stride-1 ones), test_bn_backward_epilogue_with_relu_vs_autograd on path f32 (BNB_CASES
    as data gradients, without and with amax), test_epilogue_leaves_the_bound_of_its_output (its shapes are written in its body:
    restated here, the parameters read) and test_batchnorm_finalised_in_the_consumers_prologue."""
    out = []
    for c in _literal('test_conv_gpu.py', 'CASES'):
        N, H, W, Cin, Cout, k, stride, pad, dil = c
        out += [('fwd', c, False, False), ('fwd', c, True, False)]
        if stride == 1:
            Ho, Wo = H + 2 * pad - dil * (k - 1), W + 2 * pad - dil * (k - 1)
            out.append(('dgrad', (N, Ho, Wo, Cout, Cin, k, 1, dil * (k - 1) - pad, dil), False, False))
    for N, H, W, Cin, Cout, k in _literal('test_conv_gpu.py', 'BNB_CASES'):
        out += [('bnb', (N, H, W, Cout, Cin, k, 1, k // 2, 1), False, amax) for amax in (False, True)]
    for k, _, N in _parametrized('test_conv_gpu.py', 'test_epilogue_leaves_the_bound_of_its_output', 'k,with_res,N'):
        out += [('bound', (N, 32, 32, 64, 128, k, 1, k // 2, 1), False, True), ('bound', (1, 8, 8, 64, 128, k, 1, k // 2, 1), False, True)]
    for N, H, W, Cin, Cout, k in _parametrized('test_conv_gpu.py', 'test_batchnorm_finalised_in_the_consumers_prologue', 'shape'):
        out.append(('pro', (N, H, W, Cin, Cout, k, 1, k // 2, 1), True, False))
    return out


def test_the_existing_fp32_launches_never_reached_the_edges_of_the_family():
    """What tests/test_conv_f32_edges_gpu.py is for, as assertions on the lists it complements.  (tests/test_bn_finalize_gpu.py also
    launches 1x1 convolutions of one K-step on the general loaders, but holds them to the same kernel with separately finalised
    vectors, not to a reference of the convolution.)"""
    launches = _existing_f32_launches()
    assert len(launches) == 11 * 2 + 9 + 7 * 2 + 3 * 2 + 4
    plans = [(what, case, pro, P.conv_f32(case, pro, amax)) for what, case, pro, amax in launches]
    assert all(pl is not None for _, _, _, pl in plans)
    ks = [(w, c, pro, pl) for w, c, pro, pl in plans if pl['kernel'].startswith('ksplit')]
    tiled = [(w, c, pro, pl) for w, c, pro, pl in plans if pl['kernel'].startswith('t')]
    # ---- the K-split kernel: chunk width 16 only, whole 32-column tiles, no dilation, and of the chunk counts per wave only these
    assert ks and all(pl['kernel'] == 'ksplit16' and not pl['ragged_n'] and c[8] == 1 for _, c, _, pl in ks)
    assert sorted(set(tuple(sorted(pl['chunks'])) for _, _, _, pl in ks)) == [(0, 1), (1,), (2,), (4, 5), (9,)]
    assert max(pl['M'] for _, _, _, pl in ks) == 1024                                      # the row limit (2048): never approached
    past = [pl['M'] for (_, case, pro, pl), (_, _, _, amax) in zip(plans, launches) if pl['kernel'] == 't32x128' and not amax]
    assert past and min(past) == 16384                                                     # ... from either side
    assert max(c[3] for _, c, pro, _ in plans if pro) == 256                               # ... nor the prologue's Cin <= 4096
    # ---- 128 x 128: 1x1, FAST, whole tiles, never a prologue, bias, residual or plain statistics (bnb / bound launches only)
    t128 = [(w, c, pro, pl) for w, c, pro, pl in tiled if pl['kernel'] == 't128x128']
    assert t128 and all(w in ('bnb', 'bound') and c[5] == 1 and pl['fast'] and not pro and not pl['ragged_m'] and not pl['ragged_n']
                        for w, c, pro, pl in t128)
    # ---- the general loader: only the stem (128 x 64, Cin = 4); never on 32 x 128, 128 x 32 or 128 x 128, never with Cin % 32 == 0
    general = [(c, pl) for _, c, _, pl in tiled if not pl['fast']]
    assert general and all(pl['kernel'] == 't128x64' and c[3] == 4 and pl['nsteps'] == 7 for c, pl in general)
    # ---- K-steps: never one, never an odd count on a FAST loader; a FAST loader never with stride > 1
    assert sorted(set(pl['nsteps'] for _, _, _, pl in tiled)) == [2, 4, 7, 8, 18, 36]
    assert all(pl['nsteps'] % 2 == 0 and c[6] == 1 for _, c, _, pl in tiled if pl['fast'])
    # ---- a second N tile never exists with its last columns masked
    assert all(not (pl['ntiles'] > 1 and pl['ragged_n']) for _, _, _, pl in plans)
    # (res2 is None, bnb.relu is 1 and amax_relu is 1 in every launch of that file: written in the test bodies, not in the lists)


# case -> (without a dsnt_out_bounds, without / with a prologue; the plan with one, where it differs)
CONV_F32_WANT = {
    (1, 6, 6, 24, 128, 3, 1, 1, 1): dict(kernel='ksplit8', chunks={3, 4}, ragged_m=True, ragged_n=False, mtiles=2, ntiles=4),
    (2, 5, 5, 8, 144, 1, 1, 0, 1): dict(kernel='ksplit8', chunks={0, 1}, ragged_m=True, ragged_n=True, mtiles=2, ntiles=5),
    (1, 8, 8, 48, 176, 3, 2, 1, 1): dict(kernel='ksplit16', chunks={3, 4}, ragged_m=True, ragged_n=True, mtiles=1, ntiles=6),
    (1, 9, 9, 32, 128, 3, 1, 2, 2): dict(kernel='ksplit16', chunks={2, 3}, ragged_m=True, ragged_n=False, mtiles=3, ntiles=4),
    (1, 4, 4, 384, 128, 1, 1, 0, 1): dict(kernel='ksplit16', chunks={3}, ragged_m=True, ragged_n=False, M=16, mtiles=1, ntiles=4),
    (1, 4, 8, 4096, 128, 1, 1, 0, 1): dict(kernel='ksplit16', chunks={32}, ragged_m=False, ragged_n=False, mtiles=1, ntiles=4),
    (1, 4, 8, 4104, 128, 1, 1, 0, 1): dict(kernel='ksplit8', chunks={64, 65}, ragged_m=False, ragged_n=False, mtiles=1, ntiles=4),
    (2, 32, 32, 32, 128, 1, 1, 0, 1): dict(kernel='ksplit16', chunks={0, 1}, M=2048, ragged_m=False, ragged_n=False, mtiles=64, ntiles=4),
    (1, 2049, 1, 32, 128, 1, 1, 0, 1): dict(kernel='t32x128', fast=True, nsteps=1, ktail=False, M=2049, ragged_m=True, ragged_n=False,
                                            mtiles=65, ntiles=1),
    (2, 9, 9, 32, 96, 3, 1, 1, 1): dict(kernel='t128x128', fast=True, nsteps=9, ktail=False, ragged_m=True, ragged_n=True, mtiles=2, ntiles=1),
    (1, 10, 10, 12, 72, 5, 1, 2, 1): dict(kernel='t128x128', fast=False, nsteps=10, ktail=True, ragged_m=True, ragged_n=True, mtiles=1,
                                          ntiles=1),
    (1, 128, 128, 32, 160, 1, 1, 0, 1): dict(kernel='t128x128', fast=True, nsteps=1, ktail=False, ragged_m=False, ragged_n=True, mtiles=128,
                                             ntiles=2),
    (2, 17, 15, 32, 64, 3, 2, 1, 1): dict(kernel='t128x64', fast=True, nsteps=9, ktail=False, ragged_m=True, ragged_n=False, mtiles=2, ntiles=1),
    (2, 7, 9, 16, 48, 1, 1, 0, 1): dict(kernel='t128x64', fast=False, nsteps=1, ktail=True, ragged_m=True, ragged_n=True, mtiles=1, ntiles=1),
    (1, 12, 12, 32, 64, 5, 1, 2, 1): dict(kernel='t128x64', fast=False, nsteps=25, ktail=False, ragged_m=True, ragged_n=False, mtiles=2,
                                          ntiles=1),
    (1, 11, 13, 20, 16, 3, 1, 1, 1): dict(kernel='t128x32', fast=False, nsteps=6, ktail=True, ragged_m=True, ragged_n=True, mtiles=2, ntiles=1),
    (1, 7, 5, 96, 32, 1, 1, 0, 1): dict(kernel='t128x32', fast=True, nsteps=3, ktail=False, ragged_m=True, ragged_n=False, mtiles=1, ntiles=1),
    (1, 64, 64, 16, 256, 1, 1, 0, 1): dict(kernel='t32x128', fast=False, nsteps=1, ktail=True, ragged_m=False, ragged_n=False, mtiles=128,
                                           ntiles=2),
    (1, 6, 7, 12, 128, 3, 1, 1, 1): dict(kernel='t32x128', fast=False, nsteps=4, ktail=True, ragged_m=True, ragged_n=False, mtiles=2, ntiles=1),
    (3, 30, 30, 32, 144, 3, 1, 1, 1): dict(kernel='t32x128', fast=True, nsteps=9, ktail=False, ragged_m=True, ragged_n=True, mtiles=85,
                                           ntiles=2),
}
# the K-split cases under a dsnt_out_bounds (amax / amax_bn): the 32 x 128 tiling, (fast, K-steps, K tail, N tiles)
CONV_F32_WANT_AMAX = {
    (1, 6, 6, 24, 128, 3, 1, 1, 1): (False, 7, True, 1), (2, 5, 5, 8, 144, 1, 1, 0, 1): (False, 1, True, 2),
    (1, 8, 8, 48, 176, 3, 2, 1, 1): (False, 14, True, 2), (1, 9, 9, 32, 128, 3, 1, 2, 2): (True, 9, False, 1),
    (1, 4, 4, 384, 128, 1, 1, 0, 1): (True, 12, False, 1), (1, 4, 8, 4096, 128, 1, 1, 0, 1): (True, 128, False, 1),
    (1, 4, 8, 4104, 128, 1, 1, 0, 1): (False, 129, True, 1), (2, 32, 32, 32, 128, 1, 1, 0, 1): (True, 1, False, 1),
}


def test_conv_f32_cases_hit_their_edges():
    assert sorted(CONV_F32_WANT) == sorted(E.CONV_F32) and len(set(E.CONV_F32)) == 20
    for case in E.CONV_F32:
        pl = P.conv_f32(case)
        assert pl and all(pl[k] == v for k, v in CONV_F32_WANT[case].items()), (case, pl)
        # a prologue moves one case only: Cin = 4104 is past the K-split's limit of 4096 input channels
        pro = P.conv_f32(case, pro=True)
        if case[3] == 4104:
            assert (pro['kernel'], pro['fast'], pro['nsteps'], pro['ktail']) == ('t32x128', False, 129, True), pro
        else:
            assert pro == pl, (case, pro)
        am = P.conv_f32(case, amax=True)
        if pl['kernel'].startswith('ksplit'):
            assert (am['kernel'], am['bm']) == ('t32x128', 32), (case, am)
            assert (am['fast'], am['nsteps'], am['ktail'], am['ntiles']) == CONV_F32_WANT_AMAX[case], (case, am)
            assert am['mtiles'] == pl['mtiles'] and P.conv_f32(case, pro=True, amax=True) == am
        else:
            assert am == pl, (case, am)
    assert sorted(CONV_F32_WANT_AMAX) == sorted(c for c in E.CONV_F32 if P.conv_f32(c)['kernel'].startswith('ksplit'))
    plans = {c: P.conv_f32(c) for c in E.CONV_F32}
    # every kernel form: four tile shapes x both loaders, both K-split widths
    forms = {(pl['kernel'], pl.get('fast')) for pl in plans.values()}
    assert forms == {('ksplit16', None), ('ksplit8', None)} | {(t, f) for t in ('t128x128', 't128x64', 't128x32', 't32x128') for f in (True, False)}
    # the K-split rotation: three register sets, so the chunk counts mod 3 and the short ones all occur; the limits from both sides
    counts = set().union(*[pl['chunks'] for pl in plans.values() if 'chunks' in pl])
    assert {0, 1, 2, 3, 4, 32, 64, 65} <= counts and {c % 3 for c in counts if c} == {0, 1, 2}
    assert plans[(1, 4, 8, 4096, 128, 1, 1, 0, 1)] == P.conv_f32((1, 4, 8, 4096, 128, 1, 1, 0, 1), pro=True) and 2 * 4096 <= 8 * 32 * 33
    assert {plans[c]['M'] for c in plans} >= {2048, 2049}
    # tiled: one K-step on every tile shape but 128 x 32 (FAST and general), odd counts on FAST loaders, stride 2 on a FAST loader
    one = {(pl['kernel'], pl['fast']) for pl in plans.values() if pl.get('nsteps') == 1}
    assert one == {('t32x128', True), ('t32x128', False), ('t128x128', True), ('t128x64', False)}
    assert {pl['kernel'] for pl in plans.values() if pl.get('fast') and pl['nsteps'] % 2 == 1 and pl['nsteps'] > 1} == \
        {'t128x128', 't128x64', 't128x32', 't32x128'}
    assert plans[(2, 17, 15, 32, 64, 3, 2, 1, 1)]['fast'] and plans[(1, 12, 12, 32, 64, 5, 1, 2, 1)]['fast'] is False
    assert (85 * 2) % 8 != 0 and 128 * 2 == 256


def test_plan_ref_refuses_what_the_plans_refuse():
    assert P.wgrad1((1, 127, 128, 128, 128)) is None and P.wgrad1((1, 129, 136, 128, 128)) is None      # < 16384 rows; not whole 16-row stages
    assert P.fwd1((1, 127, 32, 128, 256)) is None and P.fwd1((1, 64, 64, 128, 192)) is None
    assert P.bwd1((1, 127, 128, 64, 64)) is None and P.gemm1((255, 16, 16, 128, 256)) is None
    assert P.gemm1((257, 16, 16, 64, 128)) is None                                                      # 65792 rows: not whole 512-row iterations
    assert P.wgrad3((1, 16, 48, 64, 64)) is None and P.wgrad3((1, 16, 160, 64, 64)) is None
    assert P.conv3s((2, 4, 16, 64, 64)) is None and P.conv3s((2, 8, 32, 160, 64)) is None
    assert P.stem4((1, 6, 32)) is None and P.stem4((1, 4, 48)) is None
    assert P.conv_split((1, 8, 8, 24, 16, 1, 1, 1, 0, 1)) is None and P.conv_split((1, 8, 8, 16, 16, 4, 5, 1, 1, 1)) is None
    assert P.conv_split((16, 64, 64, 128, 128, 1, 1, 1, 0, 1), 'f16x3') is None         # the streaming 1x1 kernel's
    assert P.conv_split((16, 64, 64, 128, 128, 1, 1, 1, 0, 1))['bn'] == 128


# ---------------------------------------------------------------- the tiled split-precision kernels (csrc/conv_split6.hip)

def _existing_split_cases():
    """BF16X6_CASES of tests/test_conv_gpu.py — the geometries its bf16x6 test and tests/test_f16x3_range_gpu.py run through
    these kernels — as 10-tuples with R and S apart."""
    cases = [c for c in _literal('test_conv_gpu.py', 'CASES') if c[3] % 16 == 0 and c[4] % 4 == 0] + _literal('test_conv_gpu.py', 'BF16X6_CASES')
    return [c[:5] + (c[5],) + c[5:] for c in cases]


def test_the_existing_split_precision_cases_never_reached_the_edges_of_the_tiled_kernels():
    """What tests/test_conv_split_edges_gpu.py is for, as assertions on the list it complements.  One K-step IS in that list —
    the score_ launch (3, 8, 8, 16, 256), 192 rows on four full 64-wide tiles, once with a prologue — so the assertions below are
    about where it is not: on a 128-wide tile, on a ragged N tile, with a filter."""
    cases = _existing_split_cases()
    assert len(cases) == 10 + 11
    plans = [(c, P.conv_split(c)) for c in cases]
    assert all(pl is not None for _, pl in plans)
    gemm = [(c, pl) for c, pl in plans if pl['kernel'] == 'gemm']
    halo = [(c, pl) for c, pl in plans if pl['kernel'] == 'halo']
    assert len(gemm) == 15 and len(halo) == 6
    # ---- K-steps: one only on (3, 8, 8, 16, 256) 1x1; otherwise even
    one = [c for c, pl in gemm if pl['nsteps'] == 1]
    assert one == [(3, 8, 8, 16, 256, 1, 1, 1, 0, 1)] and P.conv_split(one[0])['bn'] == 64 and not P.conv_split(one[0])['ragged_n']
    assert all(pl['nsteps'] % 2 == 0 for c, pl in gemm if c not in one)
    # ---- the tap never changes at every K-step away from the 1x1 filter (Cin == 16 under a filter); R == S; at most 9 taps
    assert all(c[5] == c[6] and c[5] * c[6] <= 9 for c in cases)
    assert not [c for c in cases if c[3] == 16 and c[5] * c[6] > 1]
    # ---- Ho <= H; one trip of the prologue's copy; the vectors never push the LDS request past the epilogue's tile
    assert all((c[1] + 2 * c[8] - c[9] * (c[5] - 1) - 1) // c[7] + 1 <= c[1] for c in cases)
    assert max(c[3] for c in cases) == 256 and all(pl['trips'] == 1 for _, pl in gemm)
    # ---- N tiles: Cout is 16, 64, 128, 160 or 256 — never a multiple of 4 that is no multiple of 16, never a lone float4 column
    assert sorted(set(c[4] for c in cases)) == [16, 64, 128, 160, 256] and all(c[4] % 16 == 0 for c in cases)
    assert [c for c, pl in plans if pl['ragged_n'] and pl['ntiles'] > 1] == [(1, 24, 48, 32, 160, 3, 3, 1, 1, 1)]      # 32 of 128 columns: halo
    assert all(pl['bn'] - (-c[4]) % pl['bn'] >= 16 for c, pl in plans)
    # ---- the 64 / 128-column threshold (8192 rows): where it decides (Cout % 64 == 0, above 64), 512 rows at the most or 65536
    rows = sorted(set(pl['M'] for c, pl in gemm if c[4] > 64 and c[4] % 64 == 0))
    assert rows == [35, 128, 192, 512, 65536]
    # ---- row tiles: the only ragged ones hold 35 and 32 (of 288) and 64 (of 192) rows — never one row; at most two images in a tile
    assert sorted(set(pl['M'] % 128 for _, pl in gemm if pl['ragged_m'])) == [32, 35, 64]
    assert all(c[0] == 1 or c[1] * c[2] >= 64 for c in cases)
    # ---- the halo kernel: TN = 1 only on whole tiles; at most six chunks; several images only of one tile COLUMN or more
    assert all(not (pl['bn'] == 64 and pl['ragged_n']) and pl['nchunks'] <= 8 for _, pl in halo)
    assert not [c for c, _ in halo if c[0] > 1 and c[1] == 8 and c[2] == 16]
    assert not [c for c, _ in halo if c[1] == 16 and c[2] == 32]


# case -> what plan_ref.conv_split must say of it (every path), and the LDS request per path (bf16x6, f16x3)
CONV_SPLIT_WANT = {
    (1, 3, 5, 16, 4, 1, 1, 1, 0, 1): (dict(kernel='gemm', bn=64, M=15, nsteps=1, mtiles=1, ntiles=1, trips=1), (55424, 36992)),
    (1, 8, 16, 32, 64, 1, 1, 1, 0, 1): (dict(kernel='gemm', bn=64, M=128, nsteps=2, mtiles=1, ntiles=1, ragged_m=False, ragged_n=False),
                                        (55552, 37120)),
    (1, 3, 43, 48, 68, 1, 1, 1, 0, 1): (dict(kernel='gemm', bn=128, M=129, nsteps=3, mtiles=2, ntiles=1, ragged_n=True), (74112, 67584)),
    (2, 7, 9, 16, 132, 3, 3, 1, 1, 1): (dict(kernel='gemm', bn=128, M=126, nsteps=9, mtiles=1, ntiles=2, ragged_n=True), (73856, 67584)),
    (3, 5, 7, 16, 64, 3, 3, 1, 1, 1): (dict(kernel='gemm', bn=64, M=105, nsteps=9, mtiles=1, ntiles=1), (55424, 36992)),
    (1, 9, 11, 32, 192, 1, 3, 1, 1, 1): (dict(kernel='gemm', bn=64, M=121, nsteps=6, mtiles=1, ntiles=3, ragged_n=False), (55552, 37120)),
    (1, 12, 10, 16, 8, 4, 4, 2, 1, 1): (dict(kernel='gemm', bn=64, M=30, nsteps=16, mtiles=1, ntiles=1), (55424, 36992)),
    (1, 15, 13, 48, 128, 3, 3, 2, 1, 1): (dict(kernel='gemm', bn=64, M=56, nsteps=27, mtiles=1, ntiles=2, ragged_n=False), (55680, 37248)),
    (1, 11, 14, 32, 96, 3, 2, 2, 2, 2): (dict(kernel='gemm', bn=128, M=48, nsteps=12, mtiles=1, ntiles=1, ragged_n=True), (73984, 67584)),
    (1, 4, 8, 528, 72, 1, 1, 1, 0, 1): (dict(kernel='gemm', bn=128, M=32, nsteps=33, mtiles=1, ntiles=1, trips=3), (77952, 67584)),
    (2, 64, 64, 16, 128, 1, 1, 1, 0, 1): (dict(kernel='gemm', bn=64, M=8192, nsteps=1, mtiles=64, ntiles=2), (55424, 36992)),
    (1, 65, 128, 16, 128, 1, 1, 1, 0, 1): (dict(kernel='gemm', bn=128, M=8320, nsteps=1, mtiles=65, ntiles=1), (73856, 67584)),
    (1, 8, 16, 32, 4, 3, 3, 1, 1, 1): (dict(kernel='halo', bn=64, nchunks=2, mtiles=1, ntiles=1, ragged_n=True), (46080, 49152)),
    (2, 8, 48, 64, 36, 3, 3, 1, 1, 1): (dict(kernel='halo', bn=64, nchunks=4, mtiles=6, ntiles=1, ragged_n=True), (46080, 49152)),
    (1, 24, 16, 96, 64, 3, 3, 1, 1, 1): (dict(kernel='halo', bn=64, nchunks=6, mtiles=3, ntiles=1, ragged_n=False), (46080, 49152)),
    (1, 16, 32, 160, 132, 3, 3, 1, 1, 1): (dict(kernel='halo', bn=128, nchunks=10, mtiles=4, ntiles=2, ragged_n=True), (67584, 67584)),
    (3, 8, 16, 32, 128, 3, 3, 1, 1, 1): (dict(kernel='halo', bn=128, nchunks=2, mtiles=3, ntiles=1, ragged_n=False), (67584, 67584)),
}


def test_conv_split_cases_hit_their_edges():
    assert list(CONV_SPLIT_WANT) == E.CONV_SPLIT and len(set(E.CONV_SPLIT)) == 17
    plans = {}
    for case in E.CONV_SPLIT:
        figs, lds = CONV_SPLIT_WANT[case]
        for path, want_lds in zip(('bf16x6', 'f16x3'), lds):
            pl = P.conv_split(case, path)
            assert pl and all(pl[k] == v for k, v in figs.items()) and pl['lds'] == want_lds, (case, path, pl)
        assert {k: v for k, v in P.conv_split(case, 'f16x3').items() if k != 'lds'} == {k: v for k, v in P.conv_split(case).items() if k != 'lds'}
        plans[case] = P.conv_split(case)
    # all four (kernel, tile width) cells
    assert {(pl['kernel'], pl['bn']) for pl in plans.values()} == {('gemm', 64), ('gemm', 128), ('halo', 64), ('halo', 128)}
    gemm = {c: pl for c, pl in plans.items() if pl['kernel'] == 'gemm'}
    halo = {c: pl for c, pl in plans.items() if pl['kernel'] == 'halo'}
    assert len(gemm) == 12 and len(halo) == 5
    # K-steps: one on both tile widths, odd counts past one on both, even ones; the tap of a filter changing at every K-step
    assert {pl['bn'] for pl in gemm.values() if pl['nsteps'] == 1} == {64, 128}
    assert {pl['bn'] for pl in gemm.values() if pl['nsteps'] % 2 == 1 and pl['nsteps'] > 1} == {64, 128}
    assert {pl['nsteps'] for pl in gemm.values()} == {1, 2, 3, 6, 9, 12, 16, 27, 33}
    assert sum(1 for c in gemm if c[3] == 16 and c[5] * c[6] > 1) == 3
    # R != S (both orders of magnitude: 1 x 3, 3 x 2); 16 taps at stride 2: bit 2 * 15 + 1 of the loader's tap mask
    assert {(c[5], c[6]) for c in gemm if c[5] != c[6]} == {(1, 3), (3, 2)}
    assert [c for c in gemm if c[5] * c[6] == 16 and c[7] == 2] == [(1, 12, 10, 16, 8, 4, 4, 2, 1, 1)] and 15 * 2 + 1 == 31
    # output rows that see padding only: pad = 1 under a filter of ONE row
    c = (1, 9, 11, 32, 192, 1, 3, 1, 1, 1)
    assert c[5] == 1 and c[8] == 1 and 9 + 2 * 1 - (1 - 1) == 11 > c[1]
    # the prologue's copy: three trips, the last of 16 channels; the bf16x6 request above 64 KB BECAUSE of the vectors behind the tiles
    c = (1, 4, 8, 528, 72, 1, 1, 1, 0, 1)
    assert plans[c]['trips'] == 3 and 528 - 2 * 256 == 16 and plans[c]['lds'] == 2 * 3 * 256 * 48 + 2 * 528 * 4 > 128 * 132 * 4 > 65536
    assert all(pl['trips'] == 1 for k, pl in gemm.items() if k != c)
    # the row threshold from both sides, the same channels
    lo, hi = (2, 64, 64, 16, 128, 1, 1, 1, 0, 1), (1, 65, 128, 16, 128, 1, 1, 1, 0, 1)
    assert lo[3:] == hi[3:] and plans[lo]['M'] == P.FWD6_BN64_ROWS and plans[hi]['M'] == P.FWD6_BN64_ROWS + 128
    assert (plans[lo]['bn'], plans[hi]['bn']) == (64, 128) and plans[hi]['mtiles'] % 8 != 0
    # ragged N: one float4 column (both kernels), a second tile of four columns (both), 60 and 32 of 128 columns masked
    assert {pl['kernel'] for c, pl in plans.items() if c[4] == 4} == {'gemm', 'halo'}
    assert {pl['kernel'] for c, pl in plans.items() if c[4] == 132 and pl['ntiles'] == 2} == {'gemm', 'halo'}
    assert {c[4] for c, pl in gemm.items() if pl['bn'] == 128} == {68, 72, 96, 128, 132} and {c[4] for c, pl in halo.items() if pl['bn'] == 64} == {4, 36, 64}
    # ragged M: one valid row in the last tile; two and three images inside one tile
    assert plans[(1, 3, 43, 48, 68, 1, 1, 1, 0, 1)]['M'] % 128 == 1
    assert {c[0] for c, pl in gemm.items() if pl['mtiles'] == 1 and c[0] > 1} == {2, 3}
    # the halo kernel: chunk-pair loop once, twice, three and five times; tiles side by side, stacked, 2 x 2, one per image
    assert sorted(pl['nchunks'] // 2 for pl in halo.values()) == [1, 1, 2, 3, 5]
    assert {(c[0], c[1] // 8, c[2] // 16) for c in halo} == {(1, 1, 1), (2, 1, 3), (1, 3, 1), (1, 2, 2), (3, 1, 1)}
