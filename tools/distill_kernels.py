"""Launch dsnt_distill_loss_grad and, beside it, dsnt_head_loss_grad (js) on the same rows of 64 x 64 maps, for a kernel
trace: `rocprofv3 --kernel-trace --stats -- python tools/distill_kernels.py KIND ROWS TEACHER_ROWS [REPS]`
(profiles/distill_kernels.txt).  Also prints HIP-event averages of the same launches.  KIND: kl, js or mse."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'dsnt-pose2d_amd'))

import torch  # noqa: E402

from dsnt._lib import call, ptr  # noqa: E402
import dsnt.nn as dn  # noqa: E402


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    kind, rows, trows = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 50
    h = w = 64
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(1)
    student = 3.0 * torch.randn(rows, h * w, device=dev, generator=g)
    teacher = 3.0 * torch.randn(trows, h * w, device=dev, generator=g)
    mask = (torch.rand(rows, device=dev, generator=g) < 0.9).float()
    denom2 = dn.mask_denominator(mask, rows, dev)
    loss_row, g0 = torch.empty(rows, device=dev), torch.empty_like(student)
    k = dn.DISTILL_KINDS[kind]
    t_d = timed(lambda: call('dsnt_distill_loss_grad', ptr(student), ptr(teacher), ptr(mask), ptr(denom2), ptr(loss_row),
                             ptr(g0), rows, trows, h, w, 2.0, k), reps)
    hm = torch.softmax(student, -1)
    coords, target = torch.zeros(rows, 2, device=dev), 0.5 * torch.rand(rows, 2, device=dev, generator=g) - 0.25
    call('dsnt_expect_fwd', ptr(hm), ptr(coords), rows, h, w)
    dist, reg = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    t_h = timed(lambda: call('dsnt_head_loss_grad', ptr(hm), ptr(coords), ptr(target), ptr(mask), ptr(denom2), ptr(dist),
                             ptr(reg), ptr(g0), rows, h, w, 2.0 / w, 0, 1.0), reps)
    S = rows // trows
    mb = (2.0 + 1.0 / S) * rows * h * w * 4 / 1e6
    print('%s rows=%d teacher_rows=%d 64x64 DSNT_OFF=%r: distill_loss_grad %.1f us (%.0f MB, %.2f TB/s), head_loss_grad js %.1f us '
          '(%.0f MB, %.2f TB/s), ratio %.2f (passes %.2f)'
          % (kind, rows, trows, os.environ.get('DSNT_OFF', ''), t_d, mb, mb / t_d, t_h, 2.0 * rows * h * w * 4 / 1e6,
             2.0 * rows * h * w * 4 / 1e6 / t_h, t_d / t_h, (2.0 + 1.0 / S) / 2.0))


if __name__ == '__main__':
    main()
