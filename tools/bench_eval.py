"""Flip-augmented evaluation throughput: the reference-shaped batch-1 loop against the batched device path, and the
fused merge-and-head kernel alone.

    python tools/bench_eval.py [--base hg2] [--size 256] [--batches 8,32,128] [--loop-samples 64] [--iters 10]

Three measurements, one JSON line:
  * `loop`: `inference.generate_predictions(..., use_flipped=True, batch_size=1)` over `loop-samples` synthetic samples
    (CPU tensors, as a DataLoader hands them out): host wall time around the whole call, which ends with the results
    on the host.
  * `predict`: `inference.predict` on device inputs at each batch size, with the pair built inside (`paired=False`,
    ATen flip + cat) and handed over ready-made (`paired=True`, what `DeviceAugment(flip_pair=True)` produces), `iters`
    back-to-back calls between two HIP events after a warm-up.
  * `kernel`: `dsnt_flip_merge_head` alone on the model's heat-map geometry (16 joints), HIP events around 10 x `iters`
    back-to-back launches queued behind a device sleep (GPU time only), with and without the merged heat-maps
    written; bytes = logits read + heat-maps written.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dsnt-pose2d_amd')]


def _model(base, size):
    from dsnt import synthetic
    from dsnt.model import build_mpii_pose_model
    m = build_mpii_pose_model(base=base, output_strat='dsnt', reg='js')
    synthetic.fill_state_dict(m, seed=0)
    m.cuda().train()
    x, _, _ = synthetic.batch(2, size=size, seed=5, mask_p=1.0)
    with torch.no_grad():
        m(x.cuda())                 # running statistics from one train-mode forward
    return m.eval()


def _dataset(n, size):
    from dsnt import synthetic
    x, _, _ = synthetic.batch(n, size=size, seed=3, mask_p=1.0)
    m = torch.eye(2, dtype=torch.float64) * 120.0
    b = torch.full((1, 2), 80.0, dtype=torch.float64)
    return [{'input': x[i], 'transform_m': m, 'transform_b': b} for i in range(n)]


def _events(fn, iters, gpu_only=False):
    """us per call between two HIP events.  gpu_only: a device sleep is queued first, so the launches are all enqueued
    before the first one starts and the events bracket GPU time alone (not the Python call of each launch)."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if gpu_only:
        torch.cuda._sleep(50_000_000)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters         # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--base', default='hg2')
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--batches', default='8,32,128')
    ap.add_argument('--loop-samples', type=int, default=64)
    ap.add_argument('--iters', type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_eval times the GPU path: no GPU here'
    from dsnt import inference
    model = _model(a.base, a.size)
    out = {'metric': 'flip-TTA evaluation, %s + DSNT at %d px' % (a.base, a.size), 'device': torch.cuda.get_device_name()}

    data = _dataset(a.loop_samples, a.size)
    inference.generate_predictions(model, data[:2], use_flipped=True, batch_size=1)        # warm-up
    torch.cuda.synchronize()
    t = time.perf_counter()
    inference.generate_predictions(model, data, use_flipped=True, batch_size=1)
    dt = time.perf_counter() - t
    out['loop'] = {'batch_size': 1, 'samples': a.loop_samples, 'images_per_s': round(a.loop_samples / dt, 1),
                   'ms_per_image': round(dt * 1e3 / a.loop_samples, 3)}

    out['predict'] = {}
    for B in [int(v) for v in a.batches.split(',')]:
        data = _dataset(B, a.size)
        x = torch.stack([d['input'] for d in data]).cuda()
        tm = torch.stack([d['transform_m'] for d in data]).cuda()
        tb = torch.stack([d['transform_b'] for d in data]).cuda()
        pair = torch.cat([x, x.flip(-1)], 0)
        row = {}
        for paired, inp in ((False, x), (True, pair)):
            us = _events(lambda: inference.predict(model, inp, tm, tb, paired=paired), a.iters)
            row['paired' if paired else 'unpaired'] = {'us_per_batch': round(us, 1), 'images_per_s': round(B * 1e6 / us, 1)}
        out['predict'][str(B)] = row

    hm_size = model.heatmaps.shape[-1]
    out['kernel'] = {'heatmap': '%dx%d' % (hm_size, hm_size)}
    for B in [int(v) for v in a.batches.split(',')]:
        L = torch.randn(2 * B, 16, hm_size, hm_size, device='cuda')
        tm = torch.eye(2, dtype=torch.float64, device='cuda').expand(B, 2, 2).contiguous() * 120
        tb = torch.zeros(B, 1, 2, dtype=torch.float64, device='cuda')
        read = L.numel() * 4
        row = {}
        for hm in (True, False):
            us = _events(lambda: inference.flip_merge_head(L, tm, tb, 'dsnt', 'softmax', heatmaps=hm), a.iters * 10, gpu_only=True)
            moved = read + (read // 2 if hm else 0)
            row['with_heatmaps' if hm else 'coords_only'] = {'us': round(us, 2), 'bytes': moved,
                                                             'GB_per_s': round(moved / us / 1e3, 1)}
        out['kernel'][str(B)] = row
    print(json.dumps(out))


if __name__ == '__main__':
    main()
