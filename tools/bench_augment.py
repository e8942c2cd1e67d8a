"""Time DeviceAugment (the batched MPII training transform, csrc/augment.hip) on the GPU, and the same transform on the
CPU with Pillow for context.

    python tools/bench_augment.py [--batches 32,256] [--iters 50] [--cpu-samples 0]

GPU: for each batch size, R = 384 uint8 crops -> S = 256 inputs with device-drawn parameters (rotation, flip, scale,
gains), warmed up, then `iters` back-to-back calls between two events (the Python call included, as a training loop
pays it).  Bytes moved = the source crops read once + the fp32 input written + keypoints in / out (the floor: the
rotation re-reads source pixels, which are served by L2).  --cpu-samples N also times N samples of the Pillow + torch
CPU transform (tests/golden/make_augment_golden.transform_image) on this host's one core.  Prints one JSON line.
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dsnt-pose2d_amd')]

R, S, J = 384, 256, 16


def inputs(B, dev):
    r = np.random.default_rng(B)
    src = torch.from_numpy(r.integers(0, 256, (B, R, R, 3), dtype=np.uint8)).to(dev)
    m = np.tile(np.array([[2 / 300, 0, -4.0], [0, 2 / 300, -3.0], [0, 0, 1]]), (B, 1, 1))
    kp = r.uniform(300, 900, (B, J, 2))
    return (src, torch.from_numpy(kp).to(dev), torch.ones(B, J, device=dev), torch.from_numpy(m).to(dev),
            torch.full((B,), 80.0, dtype=torch.float64, device=dev))


def gpu(batches, iters):
    from dsnt.data import DeviceAugment, ImageSpecs
    from dsnt import synthetic
    assert torch.cuda.is_available(), 'bench_augment times the GPU path: no GPU here'
    dev = torch.device('cuda:0')
    aug = DeviceAugment(ImageSpecs(S, True, False), synthetic.IMAGE_MEAN, (1, 1, 1), seed=0)
    res = {}
    for B in batches:
        args = inputs(B, dev)
        for step in range(5):
            aug(*args, step=step)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for step in range(iters):
            aug(*args, step=step)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / iters * 1e3
        nbytes = B * (R * R * 3 + 3 * S * S * 4 + J * (2 * 8 + 4 + 2 * 4 + 4) + 9 * 8 + 6 * 8 + 3 * 4 + 6 + 8)
        res[B] = {'us_per_batch': round(us, 2), 'GB_per_s': round(nbytes / us / 1e3, 1), 'bytes': nbytes,
                  'us_per_image': round(us / B, 3)}
    return res


def cpu(n):
    spec = importlib.util.spec_from_file_location('gen', os.path.join(ROOT, 'tests', 'golden', 'make_augment_golden.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    torch.set_num_threads(1)
    r = np.random.default_rng(0)
    srcs = [r.integers(0, 256, (R, R, 3), dtype=np.uint8) for _ in range(4)]
    gen.transform_image(srcs[0], 1.1, 20.0, 1, (1.1, 0.9, 1.2), S)
    t0 = time.perf_counter()
    for i in range(n):
        gen.transform_image(srcs[i % 4], float(2 ** r.uniform(-0.5, 0.5)), float(r.uniform(-60, 60)) if i % 5 < 2 else 0.0,
                            i % 2, tuple(r.uniform(0.6, 1.4, 3)), S)
    dt = (time.perf_counter() - t0) / n
    return {'us_per_image': round(dt * 1e6, 1), 'images_per_s_per_core': round(1 / dt, 1), 'samples': n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='32,256')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--cpu-samples', type=int, default=0)
    ap.add_argument('--no-gpu', action='store_true')
    a = ap.parse_args()
    out = {'metric': 'DeviceAugment R=%d -> S=%d' % (R, S)}
    if not a.no_gpu:
        out['gpu'] = gpu([int(b) for b in a.batches.split(',')], a.iters)
        out['device'] = torch.cuda.get_device_name(0)
    if a.cpu_samples:
        out['cpu_pillow'] = cpu(a.cpu_samples)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
