"""The fp32 convolution family (csrc/conv_f32.hip through csrc/conv_epilogue.h) at the edges of its host plan: every tile shape
(128x128, 128x64, 128x32, 32x128) on the FAST and on the general loader, with one, odd and tail-ended counts of K-steps, ragged M
and N, a masked second N tile, stride 2 and dilation; the K-split kernel at both chunk widths, with 0 ... 4, 32 and 64 / 65 chunks
per wave, ragged Cout, and on both sides of its row and input-channel limits (tests/plan_edge_cases.py CONV_F32; what each case
lands on is asserted without a GPU by tests/test_plan_edges_cpu.py).

Every epilogue mode runs on every case (tests/conv_checks.py conv_f32_edge): bias + two residuals + statistics, the operand bounds
(amax, amax_bn with amax_relu 1 and 0), the BatchNorm prologue with and without ReLU and finalised in the launch itself, the
in-place accumulation, the BatchNorm-backward mask and sums with relu 1 and 0.  The reference is torch's fp64 convolution on the
CPU; the bars are the project's (2e-5 of the output scale, 1e-5 of a column's sum of absolute values), masks, amax, the fused
prologue and repeated launches are exact."""
import ctypes as C

import pytest

import conv_checks as K
import plan_edge_cases as E
import plan_ref as P
import test_plan_edges_cpu as T

pytestmark = pytest.mark.gpu

# in-place accumulation is the data gradient's: stride 1
PAIRS = [(case, mode) for case in E.CONV_F32 for mode in K.CONV_F32_MODES if not (mode == 'inplace' and case[6] != 1)]


def test_plan_ref_reports_the_tile_rows_of_the_library():
    """tests/plan_ref.py conv_f32 against what the ABI exposes of the plan — dsnt_conv_fwd_bm, the rows per statistics tile — for
    every case here and every fp32 launch of tests/test_conv_gpu.py."""
    from dsnt import _lib
    cases = list(E.CONV_F32) + [case for _, case, _, _ in T._existing_f32_launches()]
    assert len(cases) == 20 + 55
    for case in cases:
        g = K.geom(*case[:5], case[5], *case[5:])
        for pro in (False, True):
            for amax in (False, True):
                assert _lib.fn('dsnt_conv_fwd_bm')(C.byref(g)) == P.conv_f32(case, pro, amax)['bm'], case


@pytest.mark.parametrize('case,mode', PAIRS, ids=['%s-%s' % ('x'.join(map(str, c)), m) for c, m in PAIRS])
def test_conv_f32_at_its_plan_edges(case, mode):
    from dsnt import _lib
    g = K.geom(*case[:5], case[5], *case[5:])
    pl = P.conv_f32(case, pro=mode.startswith('pro'))
    assert _lib.fn('dsnt_conv_fwd_bm')(C.byref(g)) == pl['bm']
    assert all(pl[k] == v for k, v in T.CONV_F32_WANT[case].items()) or (case[3] == 4104 and mode.startswith('pro')), (case, pl)
    figs = K.conv_f32_edge(case, mode)
    print('plan-edge conv_f32 %s %s on %s: %s' % (case, mode, pl['kernel'], ' '.join('%s=%.3g' % kv for kv in sorted(figs.items()))))
