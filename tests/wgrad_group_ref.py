"""Cases, the restated slab plan and the CPU references of tests/test_wgrad_group_gpu.py (the grouped weight-gradient launch).

Nothing here touches the device: the plan is csrc/wgrad_gemm.hip `dsnt_wgg_plan` as read, the references are
torch.nn.grad.conv2d_weight on the CPU in float64 and float32 over the BatchNorm+ReLU'd operand."""
import numpy as np
import torch
import torch.nn.functional as F

from dsnt import synthetic

# (N, H, W, Cin, Cout, k, stride, pad, dil) and what the case is in the table for: the expected dsnt_conv_f16x3_route(g, 1),
# M = N Ho Wo, the number of splits and of 16-row steps per split, and Ho Wo.  The test asserts all of it before it launches.
CASES = [
    # the production 16x16 level: the halo kernel un-grouped (route 2), so only the group reaches the generic fp16x3 body
    ((2, 16, 16, 128, 128, 3, 1, 1, 1), dict(route=2, M=512, splits=2, steps=[16, 16], HoWo=256)),
    # the production 8x8 and 4x4 levels
    ((2, 8, 8, 128, 128, 3, 1, 1, 1), dict(route=0, M=128, splits=1, steps=[8], HoWo=64)),
    ((2, 4, 4, 128, 128, 3, 1, 1, 1), dict(route=0, M=32, splits=1, steps=[2], HoWo=16)),
    # conv1 and conv3 of a low-resolution Bottleneck
    ((2, 8, 8, 256, 128, 1, 1, 0, 1), dict(route=0, M=128, splits=1, steps=[8], HoWo=64)),
    ((2, 8, 8, 128, 256, 1, 1, 0, 1), dict(route=0, M=128, splits=1, steps=[8], HoWo=64)),
    # a single step, three steps, nine steps (an odd training batch at the 4x4 level): the odd ending of the double-buffered loop
    ((1, 4, 4, 64, 64, 3, 1, 1, 1), dict(route=0, M=16, splits=1, steps=[1], HoWo=16)),
    ((3, 4, 4, 64, 64, 3, 1, 1, 1), dict(route=0, M=48, splits=1, steps=[3], HoWo=16)),
    ((9, 4, 4, 128, 128, 3, 1, 1, 1), dict(route=0, M=144, splits=1, steps=[9], HoWo=16)),
    # several splits, the last one short: 5 x 224 rows and 176 (11 steps)
    ((9, 12, 12, 64, 64, 3, 1, 1, 1), dict(route=0, M=1296, splits=6, steps=[14, 14, 14, 14, 14, 11], HoWo=144)),
    # Ho Wo = 12 < 16: the tiny-map loop; the last step has 4 rows
    ((3, 3, 4, 64, 64, 3, 1, 1, 1), dict(route=0, M=36, splits=1, steps=[3], HoWo=12, last_rows=4)),
    # Ho Wo = 8: two image boundaries per step
    ((5, 1, 8, 32, 64, 1, 1, 0, 1), dict(route=0, M=40, splits=1, steps=[3], HoWo=8, last_rows=8)),
    ((4, 2, 4, 64, 32, 3, 1, 1, 1), dict(route=0, M=32, splits=1, steps=[2], HoWo=8)),
    # Ho Wo = 20 and 24: the image boundary moves inside the 16-row step from step to step
    ((3, 5, 4, 64, 64, 3, 1, 1, 1), dict(route=0, M=60, splits=1, steps=[4], HoWo=20, last_rows=12)),
    ((2, 6, 4, 64, 64, 3, 1, 1, 1), dict(route=0, M=48, splits=1, steps=[3], HoWo=24)),
    # stride 2 into a 4x4 map, dilation 2
    ((2, 8, 8, 64, 128, 3, 2, 1, 1), dict(route=0, M=32, splits=1, steps=[2], HoWo=16)),
    ((2, 8, 8, 64, 64, 3, 1, 2, 2), dict(route=0, M=128, splits=1, steps=[8], HoWo=64)),
    # K = 108 < 128: one masked k-tile; Cout = 160: the second n-tile is masked
    ((2, 8, 8, 12, 160, 3, 1, 1, 1), dict(route=0, M=128, splits=1, steps=[8], HoWo=64, ktiles=1, ntiles=2)),
    # Cout = 16
    ((3, 8, 8, 256, 16, 1, 1, 0, 1), dict(route=0, M=192, splits=1, steps=[12], HoWo=64)),
]

# the cases of the mixed fp16x3 / bf16x6 table: the 16x16 level, a 1x1, nine steps, six splits, the tiny map, the moving boundary,
# the masked tiles
MIXED = [0, 3, 7, 8, 9, 12, 16]


def out_hw(case):
    N, H, W, Cin, Cout, k, stride, pad, dil = case
    return (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1


def plan(case):
    """csrc/wgrad_gemm.hip dsnt_wgg_plan: (ktiles, ntiles, splits, rows_per_split)."""
    N, H, W, Cin, Cout, k, stride, pad, dil = case
    Ho, Wo = out_hw(case)
    M, K = N * Ho * Wo, k * k * Cin
    ktiles, ntiles = (K + 127) // 128, (Cout + 127) // 128
    want = max(1, 256 // (ktiles * ntiles))
    max_splits = max(1, (M + 255) // 256)
    sp = min(want, max_splits)
    rows = ((M + sp - 1) // sp + 31) // 32 * 32
    return ktiles, ntiles, (M + rows - 1) // rows, rows


def split_steps(case):
    """16-row steps of every split (the last split may be short)."""
    Ho, Wo = out_hw(case)
    M = case[0] * Ho * Wo
    _, _, splits, rows = plan(case)
    return [(min(M, (s + 1) * rows) - s * rows + 15) // 16 for s in range(splits)]


def operands(ci, case, raw):
    """x [N][Cin][H][W], the prologue (scale, shift, relu) and dy [N][Cout][Ho][Wo] of case `ci`.  raw: the identity prologue
    (scale 1, shift 0, no ReLU) of a BasicBlock's conv1 — the operand keeps its negative values."""
    N, H, W, Cin, Cout, k, stride, pad, dil = case
    Ho, Wo = out_hw(case)
    tag = 'wg%d%s' % (ci, 'r' if raw else '')
    x = synthetic.tensor(tag + 'x', (N, Cin, H, W), seed=11)
    if raw:
        sc, sh, relu = torch.ones(Cin), torch.zeros(Cin), 0
    else:
        sc = synthetic.tensor(tag + 's', (Cin,), seed=11, kind='uniform').abs() + 0.5
        sh = synthetic.tensor(tag + 'h', (Cin,), seed=11, scale=0.3)
        relu = 1 - ci % 2
    gy = synthetic.tensor(tag + 'g', (N, Cout, Ho, Wo), seed=12) * 1e-4
    return x, sc, sh, relu, gy


def activation(x, sc, sh, relu):
    act = x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    return F.relu(act) if relu else act


def references(case, act, gy):
    """dw [Cout][k][k][Cin] in float64 and float32 and db in float64 (torch.nn.grad.conv2d_weight on the CPU)."""
    N, H, W, Cin, Cout, k, stride, pad, dil = case
    size = (Cout, Cin, k, k)
    dw64 = torch.nn.grad.conv2d_weight(act.double(), size, gy.double(), stride=stride, padding=pad, dilation=dil)
    dw32 = torch.nn.grad.conv2d_weight(act.float(), size, gy.float(), stride=stride, padding=pad, dilation=dil)
    assert dw64.dtype == torch.float64 and dw32.dtype == torch.float32
    return (dw64.permute(0, 2, 3, 1).contiguous(), dw32.permute(0, 2, 3, 1).contiguous().double(),
            gy.double().sum(dim=(0, 2, 3)))


def bars(got, dw64, dw32):
    """The bars of test_wgrad_f16x3 with e32 from the CPU float32 reference: (ok, e16, e32, scale)."""
    scale = dw64.abs().max().item()
    e16 = (got.double().cpu() - dw64).abs().max().item()
    e32 = (dw32 - dw64).abs().max().item()
    ok = e16 <= 3e-5 * scale and e16 <= max(4 * e32, 2e-6 * scale)       # (a NaN fails both)
    return ok, e16, e32, scale


def ulp32(v):
    """Spacing of float32 at |v| (v: float64 array)."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)
