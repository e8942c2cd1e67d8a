"""Time one launch of the two miss-diagnosis kernels beside their nearest neighbours:

    python tools/bench_confusion.py [--batch 1024] [--joints 16] [--size 64] [--iters 21]

`dsnt_joint_confusion` beside `dsnt_pckh_hist` (one threshold), and `dsnt_target_mass` beside `dsnt_heatmap_stats`, all
four in one process on one batch of `tests/confusion_ref.case` and softmax maps of seeded logits.  Isolated launches, a
millisecond of idle between samples, HIP events on the stream the kernel runs on, the median: as `bench.py` times its
dominant kernel.  Before anything is timed the confusion tables are compared with the restatement.  Prints one JSON line,
microseconds per launch.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dsnt-pose2d_amd'), os.path.join(ROOT, 'tests')]


def timed_us(fn, args, stream, iters):
    for _ in range(3):
        assert fn(*args, stream) == 0
    torch.cuda.synchronize()
    samples = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(*args, stream)
        e1.record()
        torch.cuda.synchronize()
        samples.append(e0.elapsed_time(e1) * 1e3)
        time.sleep(1e-3)
    samples.sort()
    return round(samples[len(samples) // 2], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--joints', type=int, default=16)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--iters', type=int, default=21)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_confusion times the GPU path: no GPU here'
    import confusion_ref as ref
    from dsnt import _lib
    from dsnt._lib import ptr
    B, J, S = a.batch, a.joints, a.size
    args = ref.case(B, J, seed=1)
    mirror = ref.mirror_of(J)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in args]
    ptrs = [ptr(t) for t in dev]
    stream = _lib.stream_ptr()
    mir = (C.c_int * J)(*mirror)
    table = torch.zeros(J, J + 1, dtype=torch.int64, device='cuda')
    mutual = torch.zeros(J, dtype=torch.int64, device='cuda')
    assert _lib.fn('dsnt_joint_confusion')(*ptrs, ref.THR, mir, ptr(table), ptr(mutual), B, J, stream) == 0
    want = ref.restate(*args, mirror)
    assert np.array_equal(table.cpu().numpy(), want[0]) and np.array_equal(mutual.cpu().numpy(), want[1])
    hm = torch.softmax(torch.randn(B, J, S * S, device='cuda', generator=torch.Generator('cuda').manual_seed(0)), -1)
    hm = hm.view(B, J, S, S).contiguous()
    target = torch.nan_to_num(dev[1], nan=0.0)                 # the maps' kernels read every counted target
    out = torch.empty(B, J, 2, device='cuda')
    hist = torch.zeros(J, 2, dtype=torch.int64, device='cuda')
    stats = torch.empty(B * J, 7, device='cuda')
    index = torch.empty(B * J, dtype=torch.int32, device='cuda')
    thr = (C.c_double * 1)(ref.f32(ref.THR))
    res = {
        'dsnt_joint_confusion': timed_us(_lib.fn('dsnt_joint_confusion'),
                                         (*ptrs, ref.THR, mir, ptr(table), ptr(mutual), B, J), stream, a.iters),
        'dsnt_pckh_hist': timed_us(_lib.fn('dsnt_pckh_hist'), (*ptrs, thr, 1, ptr(hist), None, B, J), stream, a.iters),
        'dsnt_target_mass': timed_us(_lib.fn('dsnt_target_mass'),
                                     (ptr(hm), ptr(target), *ptrs[2:], ref.THR, mir, ptr(out), B, J, S, S), stream, a.iters),
        'dsnt_heatmap_stats': timed_us(_lib.fn('dsnt_heatmap_stats'), (ptr(hm), B * J, S, S, ptr(stats), ptr(index)), stream,
                                       a.iters),
    }
    print(json.dumps({'metric': 'us per launch (median of %d isolated launches): B = %d, J = %d, maps %d x %d'
                                % (a.iters, B, J, S, S), 'device': torch.cuda.get_device_name(0), **res}))


if __name__ == '__main__':
    main()
