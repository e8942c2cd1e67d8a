"""Time the ways of feeding a training batch on the GPU (R = 384 uint8 crops -> S = 256 inputs, drawn augmentation):

    python tools/bench_loader.py [--batches 32,256] [--iters 40] [--pool 1024]

- `loader`: `EpochLoader` over a resident `DeviceDataset` of `pool` crops (order + gather + augmentation, 3 launches);
- `weighted`: `WeightedLoader` over the same set with log-uniform row weights (weighted draw + gather + augmentation, 3
  launches); `reweight_us` is one `set_weights` (the CDF build, 5 launches) over the pool's rows and over 25,000 rows;
- `augment`: `DeviceAugment` on one batch already gathered on the device (2 launches), the same batch every time (its
  crops stay in cache); `augment_cold`: the same on a different pre-gathered batch each time, read from HBM as the
  loader's rows are;
- `host_fed`: INTEGRATION.md §1b, the host picks `B` rows of a host crop set, gathers them into one of two pinned
  staging buffers, copies them to the device and runs `DeviceAugment` (the event of a buffer's copy is waited for
  before the buffer is refilled).

Each path is warmed up, then `iters` batches run back to back between a host clock and a device synchronise (the host
work is what differs).  Prints one JSON line with µs per batch and images/s per path and batch size.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dsnt-pose2d_amd')]

R, S, J = 384, 256, 16


def host_set(n):
    """A host training set of n crops (64 distinct random crops, tiled: the content does not change the cost)."""
    r = np.random.default_rng(0)
    crops = np.tile(r.integers(0, 256, (64, R, R, 3), dtype=np.uint8), ((n + 63) // 64, 1, 1, 1))[:n]
    m = np.tile(np.array([[2 / 300, 0, -4.0], [0, 2 / 300, -3.0], [0, 0, 1]]), (n, 1, 1))
    return crops, r.uniform(300, 900, (n, J, 2)), np.ones((n, J), np.float32), m, np.full(n, 80.0)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='32,256')
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--pool', type=int, default=1024)
    a = ap.parse_args()
    from dsnt import synthetic
    from dsnt import _lib
    from dsnt.data import DeviceAugment, DeviceDataset, EpochLoader, ImageSpecs, WeightedLoader
    assert torch.cuda.is_available(), 'bench_loader times the GPU path: no GPU here'
    dev = torch.device('cuda:0')
    host = host_set(a.pool)
    ds = DeviceDataset.from_arrays(*host, device=dev)
    aug = DeviceAugment(ImageSpecs(S, True, False), synthetic.IMAGE_MEAN, (1, 1, 1), seed=0)
    out = {'metric': 'training batch feed R=%d -> S=%d, pool %d' % (R, S, a.pool), 'device': torch.cuda.get_device_name(0)}
    weights = torch.exp2(torch.rand(a.pool, device=dev) * 8 - 4)

    def cdf_build(n):
        w = torch.exp2(torch.rand(n, device=dev) * 8 - 4)
        cdf = torch.empty(n, dtype=torch.int64, device=dev)
        scratch = torch.empty(1 + (n + 1023) // 1024, dtype=torch.int64, device=dev)
        return lambda: _lib.call('dsnt_sample_cdf', _lib.ptr(w), n, _lib.ptr(cdf), _lib.ptr(scratch))
    out['reweight_us'] = {str(n): round(timed(cdf_build(n), a.iters), 1) for n in (a.pool, 25000)}
    for B in [int(b) for b in a.batches.split(',')]:
        res = {}
        ld = EpochLoader(ds, B, aug, drop_last=True)
        state = {'it': iter(ld)}

        def loader():
            try:
                return next(state['it'])
            except StopIteration:
                state['it'] = iter(ld)
                return next(state['it'])
        res['loader'] = timed(loader, a.iters)

        wl = WeightedLoader(ds, B, aug, weights, drop_last=True)
        wstate = {'it': iter(wl)}

        def weighted():
            try:
                return next(wstate['it'])
            except StopIteration:
                wstate['it'] = iter(wl)
                return next(wstate['it'])
        res['weighted'] = timed(weighted, a.iters)

        idx = torch.randperm(a.pool, device=dev)[:B]
        batch = [ds.crops[idx], ds.keypoints[idx], ds.keypoint_mask[idx], ds.matrix[idx], ds.head_lengths[idx]]
        step = [0]

        def augment():
            step[0] += 1
            return aug(*batch, step=step[0])
        res['augment'] = timed(augment, a.iters)

        # the same on a fresh pre-gathered batch each time (pool // B of them, the whole pool): crops come from HBM,
        # as they do for the loader, instead of staying cached between iterations
        order = torch.randperm(a.pool, device=dev)
        cold = [[t[order[i * B:(i + 1) * B]] for t in (ds.crops, ds.keypoints, ds.keypoint_mask, ds.matrix,
                                                        ds.head_lengths)] for i in range(a.pool // B)]

        def augment_cold():
            step[0] += 1
            return aug(*cold[step[0] % len(cold)], step=step[0])
        res['augment_cold'] = timed(augment_cold, a.iters)
        del cold

        stage = [torch.empty(B, R, R, 3, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        done = [None, None]
        rng = np.random.default_rng(1)

        def host_fed():
            k = step[0] % 2
            step[0] += 1
            if done[k] is not None:
                done[k].synchronize()                     # the previous copy out of this buffer has finished
            rows = np.sort(rng.choice(a.pool, B, replace=False))
            np.take(host[0], rows, axis=0, out=stage[k].numpy())
            crops = stage[k].to(dev, non_blocking=True)
            done[k] = torch.cuda.Event()
            done[k].record()
            small = [torch.from_numpy(np.ascontiguousarray(h[rows])).to(dev, non_blocking=True) for h in host[1:]]
            return aug(crops, small[0], small[1], small[2], small[3], step=step[0])
        res['host_fed'] = timed(host_fed, a.iters)
        out[str(B)] = {k: {'us_per_batch': round(v, 1), 'images_per_s': round(B / v * 1e6)} for k, v in res.items()}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
