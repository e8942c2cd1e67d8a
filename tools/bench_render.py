"""Time the device pose renderer (dsnt.vis.render_pose, `dsnt_render_pose`) against the host route it replaces.

Two runs, the profiler in one of its own (profiles/render_b32.txt):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_render.py --replay
    python tools/bench_render.py --trace DIR/*/*_kernel_trace.csv [--out FILE]

For one batch (`--batch 32 --size 256 --hm 64`: model inputs, the two wrist heat-maps with their peaks passed in, the
default skeleton) and five sets of layers (SETS; "off the canvas" moves every joint outside, which leaves the work a
workgroup does before its pixels and no segment), per call:
- `kernel`: the kernel's own time, from the trace of `--replay` (10 warm-up and `--iters` timed calls per set, in the
  order of SETS): median and least End - Start of `render_pose_kernel`'s timed dispatches.  The rate is the bytes the
  launch must move (canvas read, the coloured heat-maps read, picture written) over the median.
- `events, launch only`: device events around `--iters` back-to-back `dsnt_render_pose` calls whose argument list was
  built once (`vis._render_args`); `events, render_pose`: the same around whole `vis.render_pose` calls.  Such a loop
  gives the larger of the device's time and the host's issue time per call, so beside each stands
- `host`: the host clock around the same loop up to its last call's return, without a synchronise: what the host
  needs to issue one call.  Where `events` is not above `host`, the loop was bound by the host.
- `host route`: what the package offered before: the batch copied to the host, `ImageSpecs.unconvert` and Pillow's
  `util.draw_skeleton` per image (no heat-maps: nothing rendered them).  Host wall time per batch.
Needs the GPU.
"""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dsnt-pose2d_amd')]

import torch  # noqa: E402

SETS = ('canvas + heat-maps + skeleton', 'canvas + skeleton', 'canvas + heat-maps', 'canvas + skeleton off the canvas',
        'canvas only')
WARM = 10
KERNEL = 'render_pose_kernel'


def kernel_times(path, iters):
    """Per set of SETS, the End - Start (us) of the timed dispatches and their Start-to-Start steps, from the kernel trace
    of a `--replay --iters iters` run."""
    rows = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp'])) for r in csv.DictReader(open(path))
                  if KERNEL in r['Kernel_Name'])
    per = WARM + iters
    assert len(rows) == per * len(SETS), '%s: %d dispatches of %s, expected %d' % (path, len(rows), KERNEL, per * len(SETS))
    out = []
    for i in range(len(SETS)):
        timed = rows[i * per + WARM:(i + 1) * per]
        out.append(([(e - s) / 1e3 for s, e in timed], [(b[0] - a[0]) / 1e3 for a, b in zip(timed, timed[1:])]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--hm', type=int, default=64)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--replay', action='store_true', help='only issue the calls, for a kernel trace')
    ap.add_argument('--trace', default=None, help='the *_kernel_trace.csv of a --replay run with the same --iters')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_render.py needs the GPU'
    from dsnt import _lib, synthetic, util, vis
    from dsnt.data import ImageSpecs
    B, S, h, J = a.batch, a.size, a.hm, 16

    class Stats:
        MEAN, STDDEV = synthetic.IMAGE_MEAN, (0.25, 0.26, 0.27)
    g = torch.Generator().manual_seed(0)
    x = ((torch.rand(B, 3, S, S, generator=g) - torch.tensor(Stats.MEAN).view(1, 3, 1, 1)) /
         torch.tensor(Stats.STDDEV).view(1, 3, 1, 1)).cuda()
    coords = (torch.rand(B, J, 2, generator=g) * 1.6 - 0.8).cuda()
    mask = (torch.rand(B, J, generator=g) > 0.1).float().cuda()
    hm = torch.softmax(torch.randn(B, J, h * h, generator=g) * 3, -1).view(B, J, h, h).cuda()
    peak = hm.flatten(2).max(2).values
    out = torch.empty(B, S, S, 3, dtype=torch.uint8, device='cuda')
    base = dict(mean=Stats.MEAN, std=Stats.STDDEV, out=out)
    heat = dict(base, heatmaps=hm, peak=peak, heat_alpha=0.6)
    # every joint far outside: the work every workgroup does before its pixels (joints, tables, bounding boxes), no segment
    sets = {SETS[0]: ((x, coords, mask), heat), SETS[1]: ((x, coords, mask), base), SETS[2]: ((x,), heat),
            SETS[3]: ((x, coords + 8.0, mask), base), SETS[4]: ((x,), base)}
    canvas_bytes, heat_bytes = B * S * S * (3 * 4 + 3), 2 * B * h * h * 4
    moved = {label: canvas_bytes + (heat_bytes if 'heat' in label else 0) for label in SETS}

    def whole(label):
        args, kw = sets[label]
        return lambda: vis.render_pose(*args, **kw)

    def launch_only(label):
        args, kw = sets[label]
        full = dict(coords=None, mask=None, mean=None, std=None, bones=None, width=2.0, joint_radius=0.0,
                    pixel_coords=False, heatmaps=None, heat_colors=None, heat_alpha=1.0, peak=None, out=None)
        full.update(zip(('canvas', 'coords', 'mask'), args), **kw)
        cargs, _, keep = vis._render_args(**full)
        return lambda keep=keep: _lib.call('dsnt_render_pose', *cargs)

    if a.replay:
        for label in SETS:
            fn = whole(label)
            for _ in range(WARM + a.iters):
                fn()
            torch.cuda.synchronize()
        return

    def timed(fn, iters):
        """(device-event us, host-issue us) per call of `iters` back-to-back calls, the least of three runs each."""
        for _ in range(WARM):
            fn()
        ev, host = [], []
        for _ in range(3):
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            c0 = time.perf_counter()
            for _ in range(iters):
                fn()
            c1 = time.perf_counter()
            t1.record()
            torch.cuda.synchronize()
            ev.append(t0.elapsed_time(t1) * 1e3 / iters)
            host.append((c1 - c0) * 1e6 / iters)
        return min(ev), min(host)

    lines = ['render_pose: B=%d, %dx%d model input, default skeleton (15 bones), two %dx%d heat-maps; us per call' %
             (B, S, S, h, h)]
    traced = kernel_times(a.trace, a.iters) if a.trace else None
    for i, label in enumerate(SETS):
        lines.append('%s  (%.1f MB to move)' % (label, moved[label] / 1e6))
        if traced:
            dur, step = traced[i]
            med = statistics.median(dur)
            lines.append('  kernel (trace of %d dispatches)  median %6.1f  least %6.1f  most %6.1f   %.2f TB/s at the median'
                         '   (start to start under the profiler: median %.1f)' %
                         (len(dur), med, min(dur), max(dur), moved[label] / med / 1e6, statistics.median(step)))
        else:
            lines.append('  kernel                           not measured (no --trace)')
        for name, fn in (('events, launch only', launch_only(label)), ('events, render_pose', whole(label))):
            ev, host = timed(fn, a.iters)
            lines.append('  %-32s %6.1f   host issues one call in %6.1f   %s' %
                         (name, ev, host, 'host-bound' if ev <= host * 1.05 else 'device-bound'))

    from PIL import Image  # noqa: F401
    specs = ImageSpecs(S, True, True)

    def host_route():
        xs, cs, ms = x.cpu(), ((coords + 1) * (S / 2)).cpu(), mask.cpu()
        imgs = []
        for b in range(B):
            img = specs.unconvert(xs[b], Stats)
            util.draw_skeleton(img, cs[b], ms[b])
            imgs.append(img)
        return imgs
    host_route()
    reps = []
    for _ in range(3):
        t = time.perf_counter()
        for _ in range(5):
            host_route()
        reps.append((time.perf_counter() - t) / 5 * 1e6)
    lines.append('host route: D2H + unconvert + draw_skeleton per image  %8.1f us per batch (3 runs: %s)' %
                 (min(reps), ', '.join('%.1f' % r for r in reps)))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
