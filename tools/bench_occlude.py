"""Time dsnt.data.Occlude (csrc/occlude.hip) on the GPU against the copy that moves the same bytes and against the
DeviceAugment call that makes the batch.

    python tools/bench_occlude.py [--batches 32,256] [--iters 300] [--windows 5]

For each batch size, on an S = 256 input batch made by DeviceAugment from R = 384 crops (device-drawn parameters): the
`Occlude` call at p = 1, max_rects = 2, side = (0.1, 0.4), joint-centred, for each fill (`value`, `noise`, `paste`), the
Python call and the allocation of its outputs included, as a training loop pays them; `out.copy_(in)` of the same tensor
into a preallocated one (the floor: one read and one write of the batch); and the `DeviceAugment` call itself.  Every row
is warmed up, then `windows` windows of `iters` back-to-back calls between two device events; the figure is the median
window, with the fastest and slowest beside it.  `covered` is the rectangles' area at step 0 over the batch's pixels
(overlaps counted twice; read back once, outside the timed windows).  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dsnt-pose2d_amd'), os.path.join(ROOT, 'tools')]

from bench_augment import R, S, inputs        # noqa: E402  (the same synthetic crops and keypoints)


def timed(fn, iters, windows):
    for i in range(10):
        fn(i)
    torch.cuda.synchronize()
    us = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / iters * 1e3)
    us.sort()
    return {'us': round(us[len(us) // 2], 2), 'min': round(us[0], 2), 'max': round(us[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='32,256')
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--windows', type=int, default=5)
    a = ap.parse_args()
    from dsnt import synthetic
    from dsnt.data import DeviceAugment, ImageSpecs, Occlude
    assert torch.cuda.is_available(), 'bench_occlude times the GPU path: no GPU here'
    dev = torch.device('cuda:0')
    aug = DeviceAugment(ImageSpecs(S, True, False), synthetic.IMAGE_MEAN, (1, 1, 1), seed=0)
    out = {'metric': 'Occlude on [B, 3, %d, %d] fp32, p=1, max_rects=2, side=(0.1, 0.4), centre=joint' % (S, S),
           'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'windows': a.windows}
    for B in (int(b) for b in a.batches.split(',')):
        args = inputs(B, dev)
        sample = aug(*args, step=0)
        x = sample['input']
        nbytes = 2 * x.numel() * 4
        dst = torch.empty_like(x)
        row = {'bytes': nbytes, 'copy': timed(lambda i: dst.copy_(x), a.iters, a.windows),
               'augment': timed(lambda i: aug(*args, step=i), a.iters, a.windows)}
        for fill in ('value', 'noise', 'paste'):
            occ = Occlude.like(aug, p=1.0, max_rects=2, side=(0.1, 0.4), fill=fill, centre='joint')
            row[fill] = timed(lambda i: occ(sample, i), a.iters, a.windows)
            row[fill]['x_copy'] = round(row[fill]['us'] / row['copy']['us'], 2)
        for k in ('copy', 'value', 'noise', 'paste'):
            row[k]['GB_per_s'] = round(nbytes / row[k]['us'] / 1e3, 1)
        r = occ(sample, 0)['params']['occ_rects'].cpu().long()
        row['covered'] = round(float(sum(((q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1])).sum() for q in r)) / (B * S * S), 4)
        out[str(B)] = row
    print(json.dumps(out))


if __name__ == '__main__':
    main()
