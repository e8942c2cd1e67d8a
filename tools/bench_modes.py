"""Time one launch of the mode-seeking read-out beside its nearest neighbour, and `predict` with and without it:

    python tools/bench_modes.py [--batch 1024] [--joints 16] [--size 64] [--radius 3] [--modes 2] [--iters 21]
                                [--base hg2] [--input 256] [--predict-batch 32] [--rounds 5]

`dsnt_map_modes` beside `dsnt_heatmap_stats` on the same softmax maps of seeded logits, in one process.  Isolated
launches, a millisecond of idle between samples, HIP events on the stream the kernel runs on, the median: as `bench.py`
times its dominant kernel.  Before anything is timed a slice of the result is compared with the restatement
(tests/modes_ref.py), bit for bit.  Bytes are what the algorithm needs: one read of the maps.
`predict_ms`: a batch of `inference.predict` with flip augmentation end to end (host clock, synchronised), rounds
alternating `readout='mean'` (the code path of the commit before the read-out existed, bit for bit) and `readout='mode'`.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

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


def summary(xs):
    xs = sorted(xs)
    return {'median': round(xs[len(xs) // 2], 3), 'min': round(xs[0], 3), 'max': round(xs[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--joints', type=int, default=16)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--radius', type=int, default=3)
    ap.add_argument('--modes', type=int, default=2)
    ap.add_argument('--iters', type=int, default=21)
    ap.add_argument('--base', default='hg2')
    ap.add_argument('--input', type=int, default=256)
    ap.add_argument('--predict-batch', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_modes times the GPU path: no GPU here'
    import numpy as np
    import modes_ref as ref
    from dsnt import _lib, inference, synthetic
    from dsnt._lib import ptr
    from dsnt.model import build_mpii_pose_model
    B, J, S, r, K = a.batch, a.joints, a.size, a.radius, a.modes
    hm = torch.softmax(torch.randn(B, J, S * S, device='cuda', generator=torch.Generator('cuda').manual_seed(0)), -1)
    hm = hm.view(B, J, S, S).contiguous()
    coords = torch.empty(B * J, K, 2, device='cuda')
    mass = torch.empty(B * J, K, device='cuda')
    index = torch.empty(B * J, K, dtype=torch.int32, device='cuda')
    stats = torch.empty(B * J, 7, device='cuda')
    peak_index = torch.empty(B * J, dtype=torch.int32, device='cuda')
    stream = _lib.stream_ptr()
    modes_args = (ptr(hm), B * J, J, S, S, r, K, None, None, ptr(coords), ptr(mass), ptr(index), None)
    assert _lib.fn('dsnt_map_modes')(*modes_args, stream) == 0
    want = ref.modes(hm.view(-1, S, S)[:64].cpu().numpy(), r, K)
    for k, got in (('index', index), ('mass', mass), ('coords', coords)):
        assert np.array_equal(got[:64].cpu().numpy(), want[k], equal_nan=True), k
    res = {
        'dsnt_map_modes': timed_us(_lib.fn('dsnt_map_modes'), modes_args, stream, a.iters),
        'dsnt_heatmap_stats': timed_us(_lib.fn('dsnt_heatmap_stats'), (ptr(hm), B * J, S, S, ptr(stats), ptr(peak_index)),
                                       stream, a.iters),
    }
    nbytes = hm.numel() * 4
    res['GB_per_s'] = {k: round(nbytes / v / 1e3, 1) for k, v in res.items()}

    model = build_mpii_pose_model(base=a.base, output_strat='dsnt', reg='js')
    synthetic.fill_state_dict(model, seed=0)
    model.cuda().eval()
    E = a.predict_batch
    x, _, _ = synthetic.batch(E, size=a.input, seed=3, mask_p=1.0)
    x = x.cuda()
    pm = torch.eye(2, dtype=torch.float64, device='cuda').expand(E, 2, 2).contiguous() * 120
    pb = torch.full((E, 1, 2), 80.0, dtype=torch.float64, device='cuda')

    def predict_ms(readout, n=10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            inference.predict(model, x, pm, pb, readout=readout, mode_radius=r)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    ms = {'mean': [], 'mode': []}
    with torch.no_grad():
        for readout in ms:
            predict_ms(readout, 3)
        for _ in range(a.rounds):
            for readout in ms:
                ms[readout].append(predict_ms(readout))
    print(json.dumps({'metric': 'us per launch (median of %d isolated launches): B = %d, J = %d, maps %d x %d, radius %d, '
                                '%d modes; predict_ms: %s at %d px, batch %d, flip TTA, %d rounds of 10 calls'
                                % (a.iters, B, J, S, S, r, K, a.base, a.input, E, a.rounds),
                      'device': torch.cuda.get_device_name(0), **res,
                      'predict_ms': {'readout_mean': summary(ms['mean']), 'readout_mode': summary(ms['mode'])}}))


if __name__ == '__main__':
    main()
