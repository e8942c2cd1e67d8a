"""The one-pass backward of a 1x1 convolution (csrc/bwd1.hip, dsnt_conv1x1_bwd_f16x3) against fp64: what autograd runs as
backward-data + backward-filter of /root/reference/src/dsnt/hourglass.py:20,25 (conv1 / conv3 of a Bottleneck) and, in
the `apply` mode, the BatchNorm backward of the layer behind (hourglass.py:21,36-37), through the C ABI.  The comparisons
themselves live in tests/conv_checks.py, shared with tests/test_plan_edges_gpu.py."""
import ctypes as C

import pytest

import conv_checks as K

pytestmark = pytest.mark.gpu

CASES = [
    # N, H, W, Cin, Cout
    (4, 64, 64, 256, 128),     # conv1 of a Bottleneck (n = 128, two 16-column tiles per wave)
    (4, 64, 64, 128, 256),     # conv3 (n = 256, one tile per wave)
    (4, 64, 64, 128, 128),     # conv1 of a 128-wide Bottleneck
    (5, 64, 64, 256, 128),     # 640 stages over 214 workgroups: the last one is short
    (16, 32, 32, 128, 256),
    (2, 128, 128, 64, 64),     # the 128 x 128 level: four-wave workgroups, two per CU
    (2, 128, 128, 64, 128),
    (4, 64, 64, 256, 256),     # the `fc` convolutions: two column chunks (gridDim.y) filling one slab
]


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('mode,relu', [('apply', 1), ('given', 1), ('apply', 0), ('raw', 0), ('raw_acc', 0)])
def test_conv1x1_backward_in_one_pass(case, mode, relu):
    K.conv1x1_backward_in_one_pass(case, mode, relu)


def test_conv1x1_backward_refusals():
    from dsnt import _lib
    from dsnt._lib import ConvGeom
    ok = _lib.fn('dsnt_conv1x1_bwd_ok')
    assert not ok(C.byref(ConvGeom(4, 64, 64, 256, 64, 64, 16, 1, 1, 1, 0, 1)))       # 256 -> 16 (score): not built
    assert not ok(C.byref(ConvGeom(4, 64, 64, 128, 64, 64, 128, 3, 3, 1, 1, 1)))      # 3x3
    assert not ok(C.byref(ConvGeom(2, 16, 16, 256, 16, 16, 128, 1, 1, 1, 0, 1)))      # 512 rows
    assert not ok(C.byref(ConvGeom(1, 127, 128, 64, 127, 128, 64, 1, 1, 1, 0, 1)))    # 16256 rows: one 32-row stage short of 16384
    assert not ok(C.byref(ConvGeom(1, 257, 80, 64, 257, 80, 64, 1, 1, 1, 0, 1)))      # 20560 rows: not whole 32-row stages
    g = ConvGeom(2, 16, 16, 256, 16, 16, 128, 1, 1, 1, 0, 1)
    rc = _lib.fn('dsnt_conv1x1_bwd_f16x3')(None, None, None, None, 0, None, None, None, None, None, None, None,
                                           0, C.byref(g), None)
    assert rc == 3


FWD_CASES = [
    # N, H, W, Cin, Cout
    (4, 64, 64, 256, 128),     # conv1 of a Bottleneck
    (4, 64, 64, 128, 256),     # conv3 (+ residual)
    (4, 64, 64, 128, 128),
    (2, 128, 128, 64, 64),     # four-wave workgroups
    (2, 128, 128, 64, 128),
    (4, 64, 64, 256, 256),     # two column chunks
    (5, 64, 64, 128, 256),     # 640 stages over 214 workgroups: the last one is short
]


@pytest.mark.parametrize('case', FWD_CASES)
@pytest.mark.parametrize('pro,res', [(True, True), (True, False), (False, True), (False, False)])
def test_conv1x1_forward_on_the_lds_staged_streaming_kernel(case, pro, res):
    """dsnt_conv1x1_fwd_f16x3 (csrc/fwd1.hip: conv1 / conv3 / shortcut / `fc` forward, hourglass.py:20,25,44-48,146-153) against
    fp64 and against dsnt_conv_fwd_f16x3_ex (the first streaming kernel) on the same operands: output, the one-row-per-workgroup
    statistics (summed: the same two sums), both operand-bound outputs, bit-reproducible; DSNT_CONV_SHARE_CHIP changes no value."""
    K.conv1x1_forward_lds_staged(case, pro, res)


STEM_CASES = [
    # N, Ho (= Wo): the space-to-depth image is [N][Ho + 1][Wo + 1][16]
    (2, 128),      # the 256-pixel input of every BASELINE configuration: 256 tiles
    (3, 64),       # the 128-pixel goldens
    (9, 128),      # 1152 tiles on 512 persistent workgroups: 2-3 tiles each, ragged
    (1, 32),       # 8 tiles
]


@pytest.mark.parametrize('N,Ho', STEM_CASES)
@pytest.mark.parametrize('with_bias', [True, False])
def test_stem_forward_on_its_halo_kernel(N, Ho, with_bias):
    """dsnt_stem4_fwd_f16x3 (csrc/stem4.hip): the stem of /root/reference/src/dsnt/hourglass.py:157 (`conv1`, 7x7 / stride 2 / pad 3)
    in its space-to-depth form — a 4x4 / stride 1 / pad 1 convolution of the 16-channel image, 64 output channels — against the
    tiled fp16x3 kernel on the same operands (same K order, same products: bit-identical outputs), against torch in fp64 (the fp32
    bar), with its statistics (one row per workgroup: the column sums of y and y^2) and the bound of its output."""
    K.stem_forward_on_its_halo_kernel(N, Ho, Ho, with_bias)


@pytest.mark.parametrize('N,Ho', STEM_CASES)
def test_stem_weight_gradient_on_its_own_kernel(N, Ho):
    """The weight gradient of the same convolution (csrc/stem4.hip: stem4_wgrad_kernel, reached through dsnt_conv_wgrad_f16x3): both
    operands read transposed from pixel-major LDS images, one slab and one bias partial per workgroup — against torch in fp64 (the
    weight-gradient bar of the other fp16x3 kernels), with and without the in-call reduction, accumulating, and the refusal of a
    BatchNorm prologue (the stem's operand is the raw image)."""
    K.stem_weight_gradient_on_its_own_kernel(N, Ho, Ho)
