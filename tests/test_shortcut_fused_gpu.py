"""conv3 of a Bottleneck with a projection shortcut and that shortcut in ONE forward launch (csrc/fwd1.hip DS form:
dsnt_conv1x1_fwd_ds_f16x3), through the C ABI, at the two sites of the stem (64 -> 128 and 128 -> 256 channels): bit for bit what
the pair of existing launches leaves on the same operands and bounds, and within the per-channel fp32 bar of the fp64 result
(tests/f16x3_util.py: A bounds 2^8 loose).

Rows: M = 32 (2 W + 1) with W the workgroups a launch of the shape takes — every workgroup runs two stages or more and the last
range is short; M = 32 (W - 1) is the edge where the plan has fewer ranges than the chip has workgroup slots."""
import ctypes as C

import pytest
import torch

import f16x3_util as U
import shortcut_fused_util as S

pytestmark = pytest.mark.gpu


def _rows(Cin, Cout, edge=False):
    W = S.workgroups(Cin, Cout)
    assert 0 < W <= 512
    return 32 * (W - 1) if edge else 32 * (2 * W + 1)


@pytest.mark.parametrize('Cin,Cout', S.SITES)
@pytest.mark.parametrize('edge', [False, True])
def test_fused_forward_is_the_two_launches_bit_for_bit(Cin, Cout, edge):
    M = _rows(Cin, Cout, edge)
    pair, fused, rows = S.forward(Cin, Cout, M)
    assert bool(torch.isfinite(fused['out']).all()) and bool(torch.isfinite(fused['stats']).all())
    for k in ('out', 'stats', 'amax', 'amax_bn'):
        assert torch.equal(pair[k], fused[k]), k
    assert float(fused['amax'].max()) == float(fused['out'].abs().max())


@pytest.mark.parametrize('Cin,Cout', S.SITES)
def test_fused_forward_meets_the_fp32_bar_per_channel(Cin, Cout):
    M = _rows(Cin, Cout)
    _, fused, rows = S.forward(Cin, Cout, M)
    r64, r32 = S.forward_refs(Cin, Cout, M)
    fails = U.per_channel('fwd_ds %d->%d' % (Cin, Cout), fused['out'], r64, r32, -1)
    assert not fails, fails
    s = fused['stats'].double().sum(0).cpu()
    assert ((s[0] - r64.sum(0)).abs() <= 1e-5 * r64.abs().sum(0)).all()
    assert ((s[1] - (r64 * r64).sum(0)).abs() <= 1e-5 * (r64 * r64).sum(0)).all()


def test_fused_entry_point_refuses_what_its_neighbour_refuses():
    from dsnt import _lib
    fwd = _lib.fn('dsnt_conv1x1_fwd_ds_f16x3')
    X, Y = C.c_void_p(4096), C.c_void_p(4096 + 4)          # never followed: every call below is refused before a launch
    M = 32 * 1024
    g, half, other = S.geom(M, 64, 128), S.geom(M, 128, 128), S.geom(M, 256, 128)
    gp = lambda q: C.byref(q)
    f_args = lambda x=X, ab=X, g1=g, g2=g: (x, X, X, X, 8192, X, X, ab, X, X, X, X, X, X, 1, X, gp(g1), gp(g2), None, None)
    assert fwd(*f_args(ab=None)) == 3                       # a null bound
    assert fwd(*f_args(g2=half)) == 1                       # unequal halves
    assert fwd(*f_args(g1=other, g2=other)) == 1            # a shape without a shortcut form
    assert fwd(*f_args(x=Y)) == 2                           # a misaligned pointer
    assert b'dsnt_conv1x1_fwd_ds_f16x3' in _lib.load().dsnt_last_error()
