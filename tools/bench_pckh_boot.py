"""Time the bootstrap accumulator beside the curve it is modelled on:

    python tools/bench_pckh_boot.py [--batch 32] [--replicates 1000,200] [--rounds 11] [--iters 1000]

`PCKhBootstrap.add_normalized` (one `dsnt_pckh_boot` launch: R + 1 copies of a 16 x 2 table) and `PCKhCurve.add_normalized`
(one `dsnt_pckh_hist` launch, the same threshold 0.5) on the same batch of `tests/score_ref.case`, resident on the device
in the dtypes the kernels take.  Two numbers per variant, both in microseconds per call and both means over `iters`
calls in steady state:
- `wall`: a host clock from one synchronisation to the next around the calls, i.e. what a validation loop pays per batch,
  Python and ctypes included;
- `gpu`: HIP events around the same calls enqueued behind a device sleep, so that the host is not in the window.
Before anything is timed the table of each R is compared with `tests/boot_ref.py` on the device's own distances.  Every
variant is warmed up; the rounds alternate the variants and the median over rounds is reported with min and max.  Prints
one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dsnt-pose2d_amd'), os.path.join(ROOT, 'tests')]


def summary(xs):
    xs = sorted(xs)
    return {'median': round(xs[len(xs) // 2], 2), 'min': round(xs[0], 2), 'max': round(xs[-1], 2)}


def wall_us(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def gpu_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(100_000_000)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--replicates', default='1000,200')
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--iters', type=int, default=1000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_pckh_boot times the GPU path: no GPU here'
    import boot_ref
    import score_ref
    from dsnt.evaluator import PCKhBootstrap, PCKhCurve
    B, J, thr, seed = a.batch, 16, score_ref.THR1, 0
    args = score_ref.case(B, J, seed=B * 100 + J)
    pred, target, m, b, mask, head = [torch.from_numpy(x).cuda() for x in args[:6]]
    ids = torch.arange(B, device='cuda')
    curve = PCKhCurve(thresholds=thr)
    dist = curve.add_normalized(pred, target, mask, head, m, b, return_distances=True).cpu().numpy()
    variants = {'curve': lambda: curve.add_normalized(pred, target, mask, head, m, b)}
    for R in map(int, a.replicates.split(',')):
        boot = PCKhBootstrap(replicates=R, thresholds=thr, seed=seed)
        boot.add_normalized(pred, target, mask, head, m, b, ids)
        want = boot_ref.table(score_ref.column(dist, thr), args[4] == 1, np.arange(B), R, seed, J, len(thr))
        assert np.array_equal(boot.counts().numpy(), want), R
        variants['boot_R%d' % R] = lambda boot=boot: boot.add_normalized(pred, target, mask, head, m, b, ids)
    for fn in variants.values():
        wall_us(fn, 100)
    res = {(k, how): [] for k in variants for how in ('wall', 'gpu')}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            res[k, 'wall'].append(wall_us(fn, a.iters))
            res[k, 'gpu'].append(gpu_us(fn, a.iters))
    out = {'metric': 'add_normalized, us per call (mean of %d calls; median, min, max over %d rounds): B = %d, J = %d, T = %d'
                     % (a.iters, a.rounds, B, J, len(thr)), 'device': torch.cuda.get_device_name(0)}
    for k in variants:
        out[k] = {how: summary(res[k, how]) for how in ('wall', 'gpu')}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
