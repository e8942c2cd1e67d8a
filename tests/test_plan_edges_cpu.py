"""The cases of tests/test_plan_edges_gpu.py hold what they claim: on 256 CUs each one hits the plan edge it is listed for
(tests/plan_ref.py restates the host plans of the fp16x3 streaming kernels), and the case lists of tests/test_conv_gpu.py never
reached those edges — every 1x1 weight-gradient slab there is eight equal stages, every streaming 1x1 workgroup runs one
iteration.  No GPU: tests/test_plan_edges_gpu.py holds plan_ref itself to the C ABI on the device."""
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


def test_plan_ref_refuses_what_the_plans_refuse():
    assert P.wgrad1((1, 127, 128, 128, 128)) is None and P.wgrad1((1, 129, 136, 128, 128)) is None      # < 16384 rows; not whole 16-row stages
    assert P.fwd1((1, 127, 32, 128, 256)) is None and P.fwd1((1, 64, 64, 128, 192)) is None
    assert P.bwd1((1, 127, 128, 64, 64)) is None and P.gemm1((255, 16, 16, 128, 256)) is None
    assert P.gemm1((257, 16, 16, 64, 128)) is None                                                      # 65792 rows: not whole 512-row iterations
    assert P.wgrad3((1, 16, 48, 64, 64)) is None and P.wgrad3((1, 16, 160, 64, 64)) is None
    assert P.conv3s((2, 4, 16, 64, 64)) is None and P.conv3s((2, 8, 32, 160, 64)) is None
    assert P.stem4((1, 6, 32)) is None and P.stem4((1, 4, 48)) is None
