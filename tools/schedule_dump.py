"""Canonical text dump of a traced program's launch lists, made on the CPU (no kernel is launched; the device check of
`_lib.ptr` is bypassed as in tests/test_schedule_cpu.py).  One line per entry of tape.fwd / tape.bwd / tape.f16_uses: list,
launch name, lane and every argument.  Pointers — launch arguments, struct fields, table words — are printed as
`<allocation>+<byte offset>`, so two dumps are equal exactly when the GPU would be handed the same launches with the same
arguments on the same lanes.  An engine refactor that must not change the schedule: `--matrix DIR` before, again after, diff -r.

usage: schedule_dump.py MODEL train|eval N,C,H,W OUT [--reg js] [--record] [--input-grad]
       schedule_dump.py --matrix DIR
MODEL: hg2, resnet34, ... or `standalone` (a two-convolution tape without a parameter arena).  One configuration per process —
the library reads DSNT_OFF / DSNT_X once — so --matrix starts a fresh child per row of MATRIX and writes one file each."""
import bisect
import ctypes as C
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dsnt-pose2d_amd'))
import torch

# launches whose first argument is a table: int64 rows, int32 rows (pack_dgrad_all), a descriptor blob read as 8-byte words (group)
TABLES = ('dsnt_f16_prep_weights', 'dsnt_f16_prep_bn_bounds', 'dsnt_bn_eval_prep', 'dsnt_wgrad_reduce_all', 'dsnt_conv_wgrad_group',
          'dsnt_conv_pack_dgrad_all')
FUSED = dict(DSNT_MFMA='bf16x6', DSNT_SPLIT='f16x3', DSNT_BF16X6_MIN_ROWS='0', DSNT_X_BWD1_MIN_ROWS='0', DSNT_X_FWD1_MIN_ROWS='0')
_LANE = dict(DSNT_X_C3_SPLIT_TILES='0', DSNT_X_GROUP_ROWS='0', DSNT_X_WGRAD_LANE_ROWS='1')
SWITCHES = [('off_conv3s', dict(DSNT_OFF='conv3s+gemm1+wgrad3+wgrad1')), ('off_bwd1', dict(DSNT_OFF='bwd1+stem4w')),
            ('off_fold3', dict(DSNT_OFF='fold3')), ('off_fwd1', dict(DSNT_OFF='fwd1+stem4')), ('off_dgrad_up', dict(DSNT_OFF='dgrad_up')),
            ('x_share', dict(DSNT_X='share_grads=0,defer_res=0')), ('x_flush', dict(DSNT_X='flush_points=0,prep_split=0,wgrad_narrow=0')),
            ('defer_reduce0', dict(DSNT_DEFER_REDUCE='0')), ('fuse_finalize0', dict(DSNT_FUSE_FINALIZE='0')),
            ('mfma_f32', dict(DSNT_MFMA='f32')), ('bf16x6', dict(DSNT_SPLIT='bf16x6', DSNT_BF16X6_MIN_ROWS='0')),
            ('lanes0', dict(DSNT_LANES='0')), ('wgrad_lane0', dict(DSNT_WGRAD_LANE='0')), ('lane_rows0', dict(DSNT_X_WGRAD_LANE_ROWS='0'))]
MATRIX = ([('%s_b%d' % (b, n), [b, 'train', '%d,3,256,256' % n], {}) for b, n in
           (('hg1', 32), ('hg2', 32), ('hg8', 16), ('resnet18', 8), ('resnet34', 8), ('resnet50', 8))] +
          [('hg2_128', ['hg2', 'train', '4,3,128,128'], {}), ('hg2_eval', ['hg2', 'eval', '32,3,256,256', '--reg', 'none'], {}),
           ('hg2_128_no_relu', ['hg2', 'train', '4,3,128,128'], dict(DSNT_DEBUG_NO_RELU='1')),
           ('hg2_eval_record', ['hg2', 'eval', '4,3,128,128', '--record'], {}),
           ('hg2_input_grad', ['hg2', 'train', '32,3,256,256', '--input-grad'], {}), ('standalone', ['standalone', 'train', '2,8,16,16'], {})] +
          [('%s_%s' % (b, tag), [b, 'train', '%d,3,256,256' % n], env) for tag, env in SWITCHES for b, n in (('hg2', 32), ('resnet34', 8))] +
          [('hg2_fused_' + tag, ['hg2', 'train', '4,3,128,128'], dict(FUSED, **env)) for tag, env in
           (('prod', dict(_LANE, DSNT_X_FOLD3_ROWS='0')), ('prod3', dict(_LANE, DSNT_OFF='fold3')), ('fold', dict(DSNT_X_FOLD3_ROWS='0')))])


def cpu_ptr(t):
    """Stands in for dsnt._lib.ptr while a program is traced on the CPU (the real one refuses tensors that are not on a GPU)."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def trace(base, training, shape, reg='js', record=None, input_grad=False):
    """(tape, further named tensors its launches may point into) of one program traced on the CPU, `_lib.ptr` being `cpu_ptr`."""
    import dsnt.engine as E
    from dsnt.model import build_mpii_pose_model
    from dsnt.hourglass import Arena, Program
    if base == 'standalone':        # no parameter arena: the data gradient packs its own weights (`slot is None`)
        t = E.Tape(torch.device('cpu'), True)
        N, Cc, H, W = shape
        ps = [E.ConvParams(*(torch.zeros(s) for s in ((Cc, R, R, Cc), (Cc,), (Cc, R, R, Cc), (Cc,))), pad=R // 2) for R in (3, 1)]
        bnt = [torch.zeros(Cc) for _ in range(6)]
        bn = E.BnParams(*bnt)
        x = t.conv(t.act(N, H, W, Cc, 'x'), ps[0], want_stats=True, name='raw')
        t.to_planar(t.conv(t.norm(x, bn), ps[1], name='normed'), Cc)
        t.finish()
        t.bounds.emit_f16_prep(0)
        return t, ([('p%d.%d' % (i, j), v) for i, p in enumerate(ps) for j, v in enumerate((p.w, p.b, p.gw, p.gb))] +
                   [('bn%d' % i, v) for i, v in enumerate(bnt)])
    m = build_mpii_pose_model(base=base, output_strat='dsnt', reg=reg)
    m.train(training)
    root = m.hg if hasattr(m, 'hg') else m._runner().root
    ar = Arena(root, torch.device('cpu'))
    tape = Program(root, ar, tuple(shape), training, input_grad, record=record).tape
    return tape, [(k, getattr(ar, k)) for k in ('params', 'grads', 'fresh', 'planes', 'planes16', 'wbounds')] + \
        [('buf:' + n, b) for n, b in root.named_buffers()]


def dump(tape, extra=()):
    """(text, number of pointers that lie in no known allocation)."""
    named = [('k%d' % i, t) for i, t in enumerate(tape._keep)] + [('s:%s:%d' % k, t) for k, t in tape._scratch.items()]
    named += list(extra) + [('act%d' % i, a.buf) for i, a in enumerate(tape.acts)]
    named += [('ident%d' % i, t) for i, t in enumerate(tape._ident or ())] + list(zip(('amax', 'famax'), tape.bounds.claimed()))
    allocs = {}
    for label, t in named:
        if isinstance(t, torch.Tensor) and t.untyped_storage().nbytes():
            allocs.setdefault(t.untyped_storage().data_ptr(), (label, t.untyped_storage(), t))
    starts, missed = sorted(allocs), [0]

    def find(v):
        i = bisect.bisect_right(starts, v) - 1
        if i >= 0 and v < starts[i] + allocs[starts[i]][1].nbytes():
            return allocs[starts[i]]

    def ptr(v, sure=True, limit=1 << 44):
        """A pointer, or (not `sure`) an integer that is one if it lies in an allocation, or looks like one: >= `limit`."""
        if not v:
            return '-' if sure else str(v)
        hit = find(v)
        if hit is not None:
            return '%s+%d' % (hit[0], v - hit[1].data_ptr())
        if not sure and v < limit:
            return str(v)
        missed[0] += 1
        return '?%#x' % v

    def struct(s):
        return '%s(%s)' % (type(s).__name__, ','.join(
            '%s=%s' % (n, ptr(getattr(s, n)) if ty is C.c_void_p else repr(getattr(s, n))) for n, ty in s._fields_))

    def arg(a):
        if a is None or isinstance(a, C.c_void_p):
            return ptr(a.value if a is not None else 0)
        if hasattr(a, '_obj'):
            return struct(a._obj)
        if isinstance(a, torch.Tensor):
            return ptr(a.data_ptr())
        if isinstance(a, dict):
            return '{%s}' % ','.join('%s=%s' % (k, arg(a[k])) for k in sorted(a))
        return ptr(a, sure=False) if isinstance(a, int) else repr(a)

    def table(name, a):
        hit = find(a.value)
        if hit is None:
            return ' table=?'
        blob = hit[2].dtype == torch.uint8      # (its words also hold pairs of 32-bit fields: no telling a stray pointer from those)
        words = hit[2].view(torch.int64) if blob else hit[2]
        return ' table=[%s]' % ' '.join(ptr(w, False, 1 << 63 if blob else 1 << 44) for w in words.reshape(-1).tolist())

    lines, where = [], {}
    for tag, lst in (('fwd', tape.fwd), ('bwd', tape.bwd)):
        for i, (fn, args, name, lane) in enumerate(lst):
            where[id(lst[i])] = '%s[%d]' % (tag, i)
            if fn is None:
                lines.append('%s %s %s' % (tag, name, '%d->%d' % args[:2] if name == 'sync' else 'bucket=%s lane=%d' % (args, lane)))
            else:
                lines.append('%s %s lane=%d %s%s' % (tag, name, lane, ' '.join(arg(a) for a in args),
                                                     table(name, args[0]) if name in TABLES else ''))
    for e, u in tape.f16_uses:
        lines.append('use %s %s' % (where.get(id(e), '?'), arg(u)))
    lines.append('unresolved pointers: %d' % missed[0])
    # the algorithmic byte counts (bench.py reads the first two): part of what a refactor must leave as it was
    lines.append('bytes fwd=%d bwd=%d %s' % (tape.bytes_fwd, tape.bytes_bwd, ' '.join('%s=%d' % kv for kv in sorted(tape.bytes_by_name.items()))))
    return '\n'.join(lines) + '\n', missed[0]


def main(argv):
    if argv[0] == '--matrix':
        os.makedirs(argv[1], exist_ok=True)
        for tag, args, env in MATRIX:
            clean = {k: v for k, v in os.environ.items() if not k.startswith('DSNT_')}
            subprocess.run([sys.executable, os.path.abspath(__file__)] + args[:3] + [os.path.join(argv[1], tag + '.txt')] + args[3:],
                           env=dict(clean, **env), check=True)
        return
    base, mode, shape, out = argv[:4]
    from dsnt import _lib
    import dsnt.model  # noqa: F401  (every module that binds `ptr` by name is imported before the patch)
    _lib.ptr = cpu_ptr
    reg = argv[argv.index('--reg') + 1] if '--reg' in argv else 'js'
    tape, extra = trace(base, mode == 'train', [int(v) for v in shape.split(',')], reg, True if '--record' in argv else None,
                        '--input-grad' in argv)
    text, missed = dump(tape, extra)
    with open(out, 'w') as f:
        f.write(text)
    print('%s: %d fwd + %d bwd entries, %d uses, %d unresolved pointers' % (os.path.basename(out), len(tape.fwd), len(tape.bwd),
                                                                          len(tape.f16_uses), missed))
    return 1 if missed else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
