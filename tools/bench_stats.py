"""Time the per-joint heat-map statistics against the launch they ride on and against ATen:

    python tools/bench_stats.py [--batches 32,128] [--hm 64] [--rounds 5] [--iters 100] [--base hg2] [--predict-batch 32]

Per batch size B, with 16 joints and hm x hm maps, in microseconds of GPU time per call (HIP events around `iters`
launches that are all enqueued behind a device sleep, so the Python of each call is not in the window):
- `fused` / `fused_stats`: `dsnt_flip_merge_head` and `dsnt_flip_merge_head_stats`, with the heat-maps stored and not;
- `standalone`: `dsnt_heatmap_stats` on the stored merged heat-maps;
- `aten`: the ATen composition that gives the same seven numbers from the stored merged heat-maps (`max`, `sum`, two
  first moments, three central moments), without the fp64 step.
Bytes are what the algorithm needs: the paired logits read once, the heat-maps written when asked for (the statistics
themselves are 48 bytes per row).  `predict` is a batch of `inference.predict` with flip augmentation end to end (host
clock, synchronised), with and without `return_stats`.

Every measurement is warmed up first; the rounds alternate the variants and the median over rounds is reported with
min and max.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dsnt-pose2d_amd')]


def summary(xs):
    xs = sorted(xs)
    return {'median': round(xs[len(xs) // 2], 2), 'min': round(xs[0], 2), 'max': round(xs[-1], 2)}


def gpu_us(fn, iters):
    """us of GPU time per call: the launches queue up behind a device sleep, the events bracket them."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(50_000_000)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def aten_stats(hm):
    """peak, index, mass, mean and the three central moments of stored heat-maps [B, J, h, w] in ATen."""
    h, w = hm.shape[-2:]
    X = ((2 * torch.arange(w, device=hm.device, dtype=torch.float32) - (w - 1)) / w).view(1, w)
    Y = ((2 * torch.arange(h, device=hm.device, dtype=torch.float32) - (h - 1)) / h).view(h, 1)
    peak, index = hm.flatten(-2).max(-1)
    mass = hm.sum((-2, -1))
    mx, my = (X * hm).sum((-2, -1)), (Y * hm).sum((-2, -1))
    dx, dy = X - mx[..., None, None], Y - my[..., None, None]
    return peak, index, mass, mx, my, (dx * dx * hm).sum((-2, -1)), (dy * dy * hm).sum((-2, -1)), \
        (dx * dy * hm).sum((-2, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='32,128')
    ap.add_argument('--hm', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--base', default='hg2')
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--predict-batch', type=int, default=32)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_stats times the GPU path: no GPU here'
    import dsnt.nn as dn
    from dsnt import inference, synthetic
    from dsnt.model import build_mpii_pose_model
    J, S = 16, a.hm
    batches = [int(b) for b in a.batches.split(',')]
    variants = {}
    for B in batches:
        L = torch.randn(2 * B, J, S, S, device='cuda')
        tm = torch.eye(2, dtype=torch.float64, device='cuda').expand(B, 2, 2).contiguous() * 120
        tb = torch.zeros(B, 1, 2, dtype=torch.float64, device='cuda')
        hm = inference.flip_merge_head(L, tm, tb)[2]

        def fused(store, stats, L=L, tm=tm, tb=tb):
            return lambda: inference.flip_merge_head(L, tm, tb, 'dsnt', 'softmax', heatmaps=store, stats=stats)
        read = L.numel() * 4
        for store in (True, False):
            for stats in (False, True):
                name = 'fused%s_%s' % ('_stats' if stats else '', 'heatmaps' if store else 'coords_only')
                variants[(B, name)] = (fused(store, stats), read + (hm.numel() * 4 if store else 0))
        variants[(B, 'standalone')] = (lambda hm=hm: dn.heatmap_stats(hm), hm.numel() * 4)
        variants[(B, 'aten')] = (lambda hm=hm: aten_stats(hm), None)

    model = build_mpii_pose_model(base=a.base, output_strat='dsnt', reg='js')
    synthetic.fill_state_dict(model, seed=0)
    model.cuda().eval()
    E = a.predict_batch
    x, _, _ = synthetic.batch(E, size=a.size, seed=3, mask_p=1.0)
    x = x.cuda()
    pm = torch.eye(2, dtype=torch.float64, device='cuda').expand(E, 2, 2).contiguous() * 120
    pb = torch.full((E, 1, 2), 80.0, dtype=torch.float64, device='cuda')

    def predict_ms(stats):
        n = max(1, a.iters // 10)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            inference.predict(model, x, pm, pb, return_stats=stats)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    with torch.no_grad():
        for fn, _ in variants.values():
            fn()
        for stats in (False, True):
            inference.predict(model, x, pm, pb, return_stats=stats)
        torch.cuda.synchronize()
        res = {k: [] for k in variants}
        res['predict'], res['predict_stats'] = [], []
        for _ in range(a.rounds):
            for k, (fn, _) in variants.items():
                res[k].append(gpu_us(fn, a.iters))
            res['predict'].append(predict_ms(False))
            res['predict_stats'].append(predict_ms(True))
    out = {'metric': 'heat-map statistics, %d joints, %d x %d maps; predict %s at %d px, batch %d, flip TTA'
                     % (J, S, S, a.base, a.size, E),
           'device': torch.cuda.get_device_name(0), 'rounds': a.rounds, 'iters': a.iters}
    for B in batches:
        row = {}
        for (b, name), (_, nbytes) in variants.items():
            if b != B:
                continue
            us = summary(res[(b, name)])
            row[name] = {'us': us}
            if nbytes:
                row[name].update(bytes=nbytes, GB_per_s=round(nbytes / us['median'] / 1e3, 1))
        out[str(B)] = row
    out['predict_ms'] = summary(res['predict'])
    out['predict_return_stats_ms'] = summary(res['predict_stats'])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
