"""Cost of one `ErrorField.add_normalized` call against the host route it replaces.

    python tools/bench_error_field.py [--batches 32,2958] [--joints 16] [--bins 8] [--iters 200] [--host-iters 3]

Inputs are `tests/error_field_ref.spread(B, J)` (about a quarter of the targets outside the frame, a third of the rest
missed), resident on the device as a validation pass leaves them.  Per batch size, one JSON line holds, in us:
  * `call`: HIP events around `iters` back-to-back `add_normalized` calls after a warm-up, three times over;
  * `kernel`: the same with a device sleep queued first, so that every launch is enqueued before the first one starts
    and the events bracket GPU time alone;
  * `issue`: the host clock around issuing those calls, without a synchronise: what the Python thread pays per call;
  * `host_route`: device-to-host copies of the six tensors, then the numpy restatement (`error_field_ref.restate`, the
    per-joint loop a user writes by hand), host clock, `host-iters` times; `copies` is its first part alone.
The device tables are compared with the restatement before anything is timed.
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


def _events(fn, iters, gpu_only=False):
    """(us per call between two HIP events, us per call on the host clock for issuing them)."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if gpu_only:
        torch.cuda._sleep(100_000_000)
    a.record()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    issue = time.perf_counter() - t
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters, issue * 1e6 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='32,2958')
    ap.add_argument('--joints', type=int, default=16)
    ap.add_argument('--bins', type=int, default=8)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--host-iters', type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_error_field times the GPU path: no GPU here'
    import error_field_ref as ref
    from dsnt.evaluator import ErrorField
    for B in [int(v) for v in a.batches.split(',')]:
        args = ref.spread(B, a.joints)
        pred, target, m, b, mask, head = [torch.from_numpy(x).cuda() for x in args]
        ev = ErrorField(bins=a.bins, n_joints=a.joints)
        add = lambda: ev.add_normalized(pred, target, mask, head, m, b)
        add()
        want = ref.restate(*args, ev.threshold, ev.edges)
        counts, sums = ev.tables()
        assert np.array_equal(counts.numpy(), np.stack(want[:3])) and np.array_equal(sums.numpy(), np.stack(want[3:]))
        out = {'metric': 'ErrorField.add_normalized, us per call', 'device': torch.cuda.get_device_name(), 'B': B,
               'J': a.joints, 'bins': a.bins, 'iters': a.iters, 'in_frame': int(want[0].sum()), 'misses': int(want[1].sum())}
        runs = [_events(add, a.iters) for _ in range(3)]
        out['call'] = [round(r[0], 2) for r in runs]
        out['issue'] = [round(r[1], 2) for r in runs]
        out['kernel'] = [round(_events(add, a.iters, gpu_only=True)[0], 2) for _ in range(3)]
        route, copies = [], []
        for _ in range(a.host_iters):
            torch.cuda.synchronize()
            t = time.perf_counter()
            host = [x.cpu().numpy() for x in (pred, target, m, b, mask, head)]
            copies.append(time.perf_counter() - t)
            ref.restate(*host, ev.threshold, ev.edges)
            route.append(time.perf_counter() - t)
        out['host_route'] = [round(v * 1e6, 1) for v in route]
        out['copies'] = [round(v * 1e6, 1) for v in copies]
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
