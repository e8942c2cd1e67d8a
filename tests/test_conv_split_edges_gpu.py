"""The tiled split-precision convolutions (csrc/conv_split6.hip through csrc/conv_epilogue.h) at the edges of their host plan, on
both paths (bf16x6, fp16x3): the implicit GEMM on 128 x 64 and 128 x 128 tiles with one, two, odd and many K-steps, a filter tap
that changes at every K-step, R != S, 16 taps at stride 2, output rows of padding only, a prologue whose vectors take three trips
into LDS, both sides of the 8192-row tile-width threshold, ragged N tiles down to one float4 column, a row tile of one row and
three images in one tile; the LDS halo-tile kernel with TN = 1 and 2, ragged Cout, two to ten chunks and tiles side by side,
stacked, 2 x 2 and one per image (tests/plan_edge_cases.py CONV_SPLIT; what each case lands on is asserted without a GPU by
tests/test_plan_edges_cpu.py).  Cases at an odd index pass their weight planes further apart than the weights are long.

Every epilogue mode runs on every case (tests/conv_checks.py conv_split_edge): bias + two residuals + statistics per tile, the
operand bounds (amax, amax_bn with amax_relu 1 and 0), the BatchNorm prologue with and without ReLU, the in-place accumulation,
the BatchNorm-backward mask and sums with relu 1 and 0.  The reference is torch's fp64 convolution on the CPU; the bars are the
project's.  The tile WIDTH is not visible through the ABI: plan_ref.conv_split restates it."""
import ctypes as C
import os

import pytest
import torch

import conv_checks as K
import plan_edge_cases as E
import plan_ref as P
import test_plan_edges_cpu as T

pytestmark = pytest.mark.gpu

TRIPLES = [(case, path, mode) for case in E.CONV_SPLIT for path in K.CONV_SPLIT_PATHS for mode in K.CONV_F32_MODES]


def test_plan_ref_agrees_with_what_the_library_shows_of_the_plan():
    """dsnt_conv_f16x3_route is 2 exactly for the halo kernel and 0 for the implicit GEMM, dsnt_conv_bf16x6_ok accepts every case,
    the statistics rows are ceil(M / 128) (that many are written, and no more: conv_split_edge); for the cases here and for the
    split-precision cases of tests/test_conv_gpu.py below the streaming 1x1 kernel."""
    from dsnt import _lib
    assert 'DSNT_X_FWD6_BN64_ROWS' not in os.environ            # plan_ref.FWD6_BN64_ROWS is the library's default
    cases = list(E.CONV_SPLIT) + [c for c in T._existing_split_cases() if P.conv_split(c, 'f16x3')]
    assert len(cases) == 17 + 14
    for case in cases:
        g = K.geom(*case)
        pl = P.conv_split(case, 'f16x3')
        assert _lib.fn('dsnt_conv_bf16x6_ok')(C.byref(g)) == 1, case
        assert _lib.fn('dsnt_conv_f16x3_route')(C.byref(g), 0) == (2 if pl['kernel'] == 'halo' else 0), case
        assert pl['mtiles'] == (g.N * g.Ho * g.Wo + 127) // 128 and pl['M'] == g.N * g.Ho * g.Wo
    for case in T._existing_split_cases():
        if P.conv_split(case, 'f16x3') is None:
            assert _lib.fn('dsnt_conv_f16x3_route')(C.byref(K.geom(*case)), 0) == 1, case


@pytest.mark.parametrize('case,path,mode', TRIPLES, ids=['%s-%s-%s' % ('x'.join(map(str, c)), p, m) for c, p, m in TRIPLES])
def test_conv_split_at_its_plan_edges(case, path, mode):
    pl = P.conv_split(case, path)
    figs = K.conv_split_edge(case, path, mode)
    print('plan-edge conv_split %s %s %s on %s x%d: %s' % (case, path, mode, pl['kernel'], pl['bn'],
                                                            ' '.join('%s=%.3g' % kv for kv in sorted(figs.items()))))


def _operands(case, path, dev):
    o = K._f32_operands(case)
    xd = K.nhwc(o['x']).to(dev)
    wd = o['w'].permute(0, 2, 3, 1).contiguous().to(dev)
    planes, stride, wb = K.split_weight_planes(wd, path, 0, dev)
    ab = torch.zeros(64, device=dev)
    ab[K.A_SLOT] = 4.0 * float(o['x'].abs().max()) * float(o['sc'].abs().max() + o['sh'].abs().max() + 1)
    return o, xd, planes, stride, wb, ab


@pytest.mark.parametrize('case', [(1, 3, 43, 48, 68, 1, 1, 1, 0, 1), (2, 8, 48, 64, 36, 3, 3, 1, 1, 1)], ids=['gemm', 'halo'])
def test_share_chip_flag_changes_no_bit_on_the_tiled_kernels(case):
    """DSNT_CONV_SHARE_CHIP (bit 1 of in_relu on the fp16x3 entry) asks the streaming kernels for fewer workgroups; the tiled ones
    have no such form and must not read the bit as part of in_relu — with ReLU off it would turn it on."""
    dev = torch.device('cuda:0')
    o, xd, planes, stride, wb, ab = _operands(case, 'f16x3', dev)
    M, Cout, tiles = o['M'], case[4], (o['M'] + 127) // 128
    scd, shd, bd = o['sc'].to(dev), o['sh'].to(dev), o['b'].to(dev)
    for in_relu in (0, 1):
        outs = []
        for flag in (0, 2):
            y, st = K.Guarded(M, Cout, dev), K.Guarded(tiles * 2, Cout, dev, guard_rows=4)
            K.split_launch('f16x3', xd, planes, stride, wb, ab, bd, y.t, scd, shd, in_relu | flag, None, None, st.t, o['g'])
            torch.cuda.synchronize()
            outs.append((y, st))
        assert K._f32_same(outs[0], outs[1]), (case, in_relu)
        assert bool((outs[0][0].t != K.SENT).all())
        if in_relu == 0:
            assert float(outs[0][0].t.min()) < 0
    ref = K._f32_conv64(o, case, o['sc'], o['sh'], 1) + o['b'].double()
    assert float((outs[0][0].t.cpu().double() - ref).abs().max()) <= K.F32_BAR * float(ref.abs().max())


def test_the_entry_points_refuse_what_the_kernels_cannot_run():
    """Each call returns non-zero, leaves its message in dsnt_last_error and does not touch y."""
    from dsnt import _lib
    from dsnt._lib import BnBwdEpilogue
    dev = torch.device('cuda:0')
    case = (1, 8, 16, 32, 64, 1, 1, 1, 0, 1)
    err = _lib.fn('dsnt_last_error')
    for path in K.CONV_SPLIT_PATHS:
        o, xd, planes, stride, wb, ab = _operands(case, path, dev)
        g, M, Cout = o['g'], o['M'], case[4]
        n = 64 * 32
        y, st = K.Guarded(M, Cout, dev), K.Guarded(2, Cout, dev, guard_rows=4)
        bd = o['b'].to(dev)
        xin, vec = torch.zeros(M, Cout, device=dev), torch.ones(Cout, device=dev)
        bnb = BnBwdEpilogue(xin.data_ptr(), vec.data_ptr(), vec.data_ptr(), vec.data_ptr(), vec.data_ptr(), 1)
        am = torch.zeros(64, device=dev)
        tail_bn = K._out_bounds(1, am, am, vec, vec)

        def refused(what, geom=g, stride=stride, bias=None, bnb=None, tail=None, ab=ab):
            rc = K.split_launch(path, xd, planes, stride, wb, ab, bias, y.t, None, None, 0, None, None, st.t, geom, bnb, tail, check=False)
            torch.cuda.synchronize()
            msg = err()
            assert rc != 0 and what in msg, (path, what, rc, msg)
            assert bool((y.buf == K.SENT).all()) and bool((st.buf == K.SENT).all()), (path, what)

        name = b'dsnt_conv_fwd_bf16x6'            # both entry points check through conv_fill under this name
        refused(name + b': geometry not supported', geom=K.geom(1, 8, 16, 24, 64, 1, 1, 1, 0, 1))                # Cin = 24
        refused(name + b': geometry not supported', geom=K.geom(1, 8, 16, 32, 64, 4, 5, 1, 2, 1))                # 20 taps
        refused(name + b': bad plane stride %d' % (n + 4), stride=n + 4)
        refused(name + b': bad plane stride %d' % (n - 8), stride=n - 8)
        refused(name + b'_ex: the batch-norm-backward epilogue', bias=bd, bnb=bnb)
        refused(name + b'_ex: dsnt_out_bounds.amax_bn excludes', bnb=bnb, tail=tail_bn)
        if path == 'f16x3':
            refused(b'dsnt_conv_fwd_f16x3_ex: the operand bounds', ab=None)
        # and the same buffers take a launch that is in order
        assert K.split_launch(path, xd, planes, stride, wb, ab, bd, y.t, None, None, 0, None, None, st.t, g) == 0
        torch.cuda.synchronize()
        assert y.intact() and st.intact() and bool((y.t != K.SENT).all())
