"""The convolution of a tape: which kernel runs its forward, what its backward is made of — the one-launch 1x1 form, or a weight
gradient (direct, slab or grouped) and a data gradient (with the BatchNorm-backward epilogue of the layer in front and, folded
in, the apply of the layer behind) — and the gradients of its residual inputs.  `Tape.conv` / `Tape.conv_ds` build a `ConvOp`,
create its output and register its backward; everything the op decides and emits is here."""
import ctypes as C

import torch

from . import _lib
from ._lib import ConvGeom, BnBwdEpilogue, BnTail, BnPrologue, BnBwdApply


def use6(tape, g):
    return (tape.use_bf16x6 and g.N * g.Ho * g.Wo >= tape.bf16x6_min_rows and
            bool(tape.lib.dsnt_conv_bf16x6_ok(C.byref(g))))


def stream_ok(tape, p, g, res2):
    """A 3x3 convolution the symmetric persistent kernel runs (weights in stream order): at most one residual."""
    return (tape.conv3s and p.R == 3 and p.S == 3 and res2 is None and
            bool(tape.lib.dsnt_conv_fwd_stream_ok(C.byref(g))))


def share(tape, persistent=True):
    """DSNT_CONV_SHARE_CHIP (bit 1 of a launch's flag word) on the side lanes' launches of the persistent kernels (3x3: 3/2
    workgroups per CU; 1x1: half of the CUs): they hold most of a CU's LDS for the whole launch, and the chain's kernels
    need LDS too (-0.2 ms)."""
    return 2 if (persistent and tape.lane != 0) else 0


def stats_tiles(tape, g, big):
    """Rows of per-tile column sums that a tiled launch on geometry g leaves (big: the 128-row tiles of the split-precision kernels)."""
    bm = 128 if big else tape.lib.dsnt_conv_fwd_bm(C.byref(g))
    return (g.N * g.Ho * g.Wo + bm - 1) // bm


def tail_at(slot):
    """The dsnt_out_bounds that makes a launch leave max|written| in a bound slot."""
    tl = BnTail()
    tl.amax = slot.data_ptr()
    return tl


def bn_epilogue(x, n):
    """The BatchNorm(+ReLU) n in front of x's consumer (None: a raw operand) as a data gradient's epilogue reads it."""
    vectors = (n.scale, n.shift, n.mean, n.invstd) if n is not None else (None,) * 4
    return BnBwdEpilogue(_lib.ptr(x.buf), *(_lib.ptr(v) for v in vectors), 1 if (n is not None and n.relu) else 0)


def bn_apply(y, ap):
    """(BnBwdApply of y's pending BatchNorm backward, the tensors behind it for `f16_uses`)."""
    n = ap.n
    return (BnBwdApply(_lib.ptr(y.buf), _lib.ptr(n.scale), _lib.ptr(n.mean), _lib.ptr(n.invstd), _lib.ptr(ap.coef)),
            dict(dz=ap.dz, y=y.buf, scale=n.scale, mean=n.mean, invstd=n.invstd, coef=ap.coef))


def ds_fuse_ok(tape, x, p_ds, p3):
    """`Tape.ds_fuse_ok`: a train step on fp16x3 from DSNT_X_DS_FUSE_ROWS rows, equal halves, the forward's `_ok` predicate,
    x's producer able to leave max|x|."""
    if not (tape.ds_fuse and tape.training and tape.record and tape.use_f16x3 and tape.fwd1):
        return False
    if not (p_ds.R == 1 and p_ds.S == 1 and p_ds.stride == 1 and p3.R == 1 and p3.S == 1 and p3.stride == 1 and
            (p_ds.Cin, p_ds.Cout) == (p3.Cin, p3.Cout) and (p3.Cin, p3.Cout) in ((64, 128), (128, 256)) and
            x.M >= tape.ds_fuse_rows and p_ds.post_reduce is None and p3.post_reduce is None):
        return False
    if any(p.wq is None or p.wq16 is None for p in (p_ds, p3)) or p_ds.wq_stride != p3.wq_stride:
        return False
    g = tape.geom(x, p_ds)
    if not (use6(tape, g) and tape.lib.dsnt_conv1x1_fwd_ok(C.byref(g))):
        return False
    return tape.bounds.operand_amax(x) is not None      # (claims the producer's tail, as the shortcut's own launch would)


class _Dgrad:
    """The operands of one data-gradient launch (`ConvOp.dgrad_operands`)."""
    __slots__ = ('native', 'gd', 'gsrc', 'wd', 'wq', 'wq_stride', 'wq16', 'wbd', 'g_amax', 'd6', 'd16', 'd_stream')

    def __init__(self, native, gd, gsrc, wd, wq, wq_stride, d6, g_amax, d16, d_stream, wq16, wbd):
        self.native, self.gd, self.gsrc = native, gd, gsrc      # the phase kernel of a strided convolution / geometry / dL/dy
        self.wd, self.wq, self.wq_stride, self.d6 = wd, wq, wq_stride, d6       # re-packed weights: fp32, bf16 planes (d6)
        self.g_amax, self.d16, self.d_stream, self.wq16, self.wbd = g_amax, d16, d_stream, wq16, wbd    # ... fp16 planes (d16)


class ConvOp:
    """One traced convolution y = conv(src) + bias [+ res1 + res2]; src is an Act (raw) or a Normed (BN+ReLU folded)."""
    __slots__ = ('tape', 'src', 'x', 'y', 'p', 'g', 'res1', 'res2', 'name', 'normed', 'sc', 'sh', 'relu', 'need_input_grad', 'bucket',
                 'x_amax', 'use6', 'use16', 'slot', 'slot_k', 'fuse1', 'fold3_ok', 'gd')

    def __init__(self, tape, src, p, res1, res2, name, need_input_grad):
        from .engine import Normed      # (the engine imports this module)
        self.tape, self.src, self.p, self.res1, self.res2, self.name = tape, src, p, res1, res2, name
        self.need_input_grad = need_input_grad
        self.normed = isinstance(src, Normed)
        self.x = src.x if self.normed else src
        self.g = tape.geom(self.x, p)
        self.sc, self.sh, self.relu = (src.scale, src.shift, 1 if src.relu else 0) if self.normed else (None, None, 0)
        self.bucket = tape.cur_bucket
        self.y = None                   # the output activation: the tape creates it (`conv_ds`: one for two ops)
        # decided by the forward: the bound slot of a raw A operand, the split-precision kernels the op runs on
        self.x_amax, self.use6, self.use16 = None, False, False
        # decided by `plan_backward`: the slot among the re-packed data-gradient weights, the one-launch 1x1 backward, the folded
        # apply of a 3x3 convolution, the geometry of the stride-1 data gradient
        self.slot, self.slot_k, self.fuse1, self.fold3_ok, self.gd = None, None, False, False, None

    # ------------------------------------------------------------------ helpers
    def operand_bound(self):
        """The bound slot of the A operand as its producer leaves it (None if it cannot); the first call claims the producer's tail."""
        bd = self.tape.bounds
        return bd.operand_amax_bn(self.src) if self.normed else bd.operand_amax(self.x)

    def dz_buffer(self, private):
        """dz of the BatchNorm in front of this op: the op's scratch, or — read again by the backward of the 1x1 convolution
        that produced x (`fold_ok`) — a buffer that outlives this op's launches."""
        t, n = self.tape, self.x.M * self.x.C
        return t.empty(n) if private else t.scratch('da', n).view(-1)[:n]

    def a_operand(self, a_bound):
        """The A operand's part of an `f16_uses` record."""
        return dict(x=self.x.buf, sc=self.sc, sh=self.sh, relu=self.relu, a_bound=a_bound)

    def use(self, e, kind, **operands):
        """One `f16_uses` record: list entry e reads these tensors under these bounds (tests/test_bounds_gpu.py).  e None: the
        record alone, for a launch that does not exist yet (the bucket's grouped weight gradient)."""
        u = dict(kind=kind, name=self.name, **operands)
        if e is not None:
            self.tape.f16_uses.append((e, u))
        return u

    # ------------------------------------------------------------------ forward
    def forward(self, want_stats):
        """Choose the forward kernel — fwd1 / stem4 / stream or tiled fp16x3 / bf16x6 / fp32 with the BatchNorm finalised in its
        prologue / fp32 — and emit it."""
        t, lib, bd = self.tape, self.tape.lib, self.tape.bounds
        src, x, y, p, g, normed, res2 = self.src, self.x, self.y, self.p, self.g, self.normed, self.res2
        sc, sh, relu = self.sc, self.sh, self.relu
        if normed:
            t.check_lane(src)
        part, tail = None, None
        big = self.use6 = use6(t, g) and p.wq is not None
        can16 = big and p.wq16 is not None
        # the large 1x1 convolutions with both operand bounds: the LDS-staged streaming kernel (csrc/fwd1.hip) — its statistics
        # come one row per WORKGROUP, and how many that is depends on the launch's share flag, so a candidate claims its bound
        # (and keeps it if f1 turns out false) BEFORE the statistics buffer is allocated; every other convolution after it
        early = can16 and p.R == 1 and res2 is None and t.fwd1
        x_amax = self.operand_bound() if early else None
        f1 = bool(early and t.use_f16x3 and ((t.training and normed) or x_amax is not None) and
                  lib.dsnt_conv1x1_fwd_ok(C.byref(g)))
        f1_shr = share(t, f1)
        # the stem's space-to-depth convolution (4x4, 16 -> 64 channels, a raw operand): the halo kernel of csrc/stem4.hip
        s4 = bool(can16 and t.use_f16x3 and t.stem4 and not normed and self.res1 is None and res2 is None and
                  lib.dsnt_stem4_fwd_ok(C.byref(g)))
        if want_stats and t.training:
            tiles = (lib.dsnt_conv1x1_fwd_stats_rows(C.byref(g), f1_shr) if f1 else
                     lib.dsnt_stem4_fwd_stats_rows(C.byref(g)) if s4 else stats_tiles(t, g, big))
            part = t.empty(tiles, 2, p.Cout)
            y.stats = (part, tiles)
        if big and t.use_f16x3:
            # the large-tile kernels can leave max|y| behind: a later consumer of the raw y claims it (operand_amax)
            y.amax_tail = tail = BnTail()
        r1 = self.res1.buf if self.res1 is not None else None
        r2 = res2.buf if res2 is not None else None
        if t.use_f16x3 and t.training and normed:
            bd.f16_bn_bound(src)       # also for the weight gradient of convs whose forward is not fp16x3
        # fp16x3 needs a bound of the A operand: train-mode BatchNorm parameters, or the producer's max|x| for a raw x
        if can16 and not early:
            x_amax = self.operand_bound()
        self.x_amax = x_amax
        use16 = self.use16 = can16 and t.use_f16x3 and ((t.training and normed) or x_amax is not None)
        if normed and (use16 or big):
            t.materialize(src)
        if use16:
            st = stream_ok(t, p, g, res2)
            bd.f16_weights(p, stream=st)
            ab = bd.f16_bn_bound(src) if (normed and t.training) else x_amax
            if f1:
                e = t.f('dsnt_conv1x1_fwd_f16x3', x.buf, p.wq16, p.wq_stride, p.wb, ab, p.b, y.buf, sc, sh, relu | f1_shr, r1,
                        part, g, tail)
            elif s4:
                e = t.f('dsnt_stem4_fwd_f16x3', x.buf, p.wq16, p.wq_stride, p.wb, ab, p.b, y.buf, part, g, tail)
            else:
                e = t.f('dsnt_conv_fwd_f16x3_stream' if st else 'dsnt_conv_fwd_f16x3_ex', x.buf, p.wq16, p.wq_stride, p.wb, ab,
                        p.b, y.buf, sc, sh, relu | share(t, st or p.R == 1), r1, r2, part, g, None, tail)
            self.use(e, 'fwd', **self.a_operand(ab), w=p.w, w_bound=p.wb)
        elif big:
            t.f('dsnt_conv_fwd_bf16x6_ex', x.buf, p.wq, p.wq_stride, p.b, y.buf, sc, sh, relu, r1, r2, part, g,
                None, tail)
        elif normed and src.pending is not None and lib.dsnt_conv_fwd_pro_ok(C.byref(g), src.pending[1], src.bn.C):
            # the BatchNorm of this operand has few statistics tiles: finalised in this launch's prologue
            spart, stiles = src.pending
            src.pending = None
            bn = src.bn
            pro = BnPrologue(_lib.ptr(spart), stiles, bn.C, x.M, _lib.ptr(bn.gamma), _lib.ptr(bn.beta), _lib.ptr(bn.rmean),
                             _lib.ptr(bn.rvar), bn.momentum, bn.eps, _lib.ptr(src.mean), _lib.ptr(src.invstd),
                             _lib.ptr(src.scale), _lib.ptr(src.shift))
            t._keep.extend((spart, src.mean, src.invstd, src.scale, src.shift))
            t.f('dsnt_conv_fwd_pro', x.buf, p.w, p.b, y.buf, pro, relu, r1, r2, part, g, tail)
        else:
            if normed:
                t.materialize(src)
            t.f('dsnt_conv_fwd_ex', x.buf, p.w, p.b, y.buf, sc, sh, relu, r1, r2, part, g, None, tail)

    def forward_ds(self, cd, want_stats):
        """The forward of `Tape.conv_ds`: this op (conv3 of a Bottleneck) and cd (the projection shortcut) as ONE launch over
        their shared output (csrc/fwd1.hip DS)."""
        t, bd = self.tape, self.tape.bounds
        src, x, y, p, g = self.src, self.x, self.y, self.p, self.g
        t.check_lane(src)
        self.use6 = cd.use6 = True
        self.use16 = cd.use16 = True
        shr = share(t)
        part = None
        if want_stats:
            tiles = t.lib.dsnt_conv1x1_fwd_stats_rows(C.byref(g), shr)
            part = t.empty(tiles, 2, p.Cout)
            y.stats = (part, tiles)
        y.amax_tail = tail = BnTail()
        ab = bd.f16_bn_bound(src)
        self.x_amax, cd.x_amax = None, bd.operand_amax(cd.x)
        t.materialize(src)
        for q in (p, cd.p):
            bd.f16_weights(q, stream=False)
        e = t.f('dsnt_conv1x1_fwd_ds_f16x3', x.buf, cd.x.buf, p.wq16, cd.p.wq16, p.wq_stride, p.wb, cd.p.wb, ab, cd.x_amax,
                p.b, cd.p.b, y.buf, self.sc, self.sh, self.relu | shr, part, g, cd.g, tail)
        # one record per operand pair
        self.use(e, 'fwd', **self.a_operand(ab), w=p.w, w_bound=p.wb)
        cd.use(e, 'fwd', **cd.a_operand(cd.x_amax), w=cd.p.w, w_bound=cd.p.wb)

    # ------------------------------------------------------------------ backward
    def plan_backward(self):
        """Decided while the forward is traced: the slot among the re-packed data-gradient weights, and whether the backward can take
        over the BatchNorm backward of the op's consumer (`Act.fold_ok`: that BatchNorm's backward, emitted first, leaves its apply
        pending)."""
        t, x, y, p, g = self.tape, self.x, self.y, self.p, self.g
        if self.need_input_grad and t.param_arena is not None:
            self.slot, self.slot_k = t.bounds.dgrad_slot(p)
        # the whole backward of this convolution as ONE launch (csrc/bwd1.hip): 1x1 behind a train-mode BatchNorm, both
        # operand bounds known on the device
        one_pass = t.bwd1 and t.use_f16x3 and t.defer_reduce and self.slot is not None
        self.fuse1 = bool(one_pass and (self.normed or self.x_amax is not None) and p.R == 1 and p.S == 1 and
                          p.post_reduce is None and t.lib.dsnt_conv1x1_bwd_ok(C.byref(g)))
        # ... and without residual inputs (whose gradient IS dL/dy) it can also take over the BatchNorm backward of its consumer
        plain = self.normed and self.res1 is None and self.res2 is None
        # the geometry of the stride-1 data gradient: decided here, read again by `dgrad_operands`
        if p.stride == 1:
            self.gd = ConvGeom(x.N, g.Ho, g.Wo, p.Cout, x.H, x.W, p.Cin, p.R, p.S, 1, p.dil * (p.R - 1) - p.pad, p.dil)
        # the same for a 3x3 convolution on the persistent fp16x3 kernel (conv2 of a Bottleneck: bn3's backward rides in the operand
        # load of conv2's data gradient, csrc/conv3s.hip MODE 4), from DSNT_X_FOLD3_ROWS output rows — if the data gradient of
        # THAT geometry takes the fp16x3 stream kernel: a geometry it refuses is decided HERE, while the consumer BatchNorm can
        # still be told to apply by itself
        self.fold3_ok = bool(t.fold3 and one_pass and plain and t.training and p.R == 3 and p.S == 3 and self.gd is not None and
                             self.use16 and y.M >= t.fold3_rows and use6(t, self.gd) and stream_ok(t, p, self.gd, None))
        y.fold_ok = bool(self.fuse1 and plain) or self.fold3_ok

    def backward(self):
        """Emit the backward: the one-launch 1x1 form, or weight gradient and data gradient; then the residual inputs' gradients."""
        t, y = self.tape, self.y
        gy, ap = y.grad, y.pending_apply
        fused = self.fuse1 and t.bounds.dgrad_planes16 is not None
        fold3 = bool(self.fold3_ok and ap is not None and gy is None and t.bounds.dgrad_planes16 is not None and
                     self.need_input_grad and ap.bound is not None)
        if ap is not None and (not fused or gy is not None) and not fold3:
            t.materialize_apply(y)
            ap, gy = None, y.grad
        assert gy is not None or ap is not None, 'no gradient reached conv output ' + self.name
        if fused and ap is None and y.grad_amax is None:
            fused = False
        wl, defer_res = t.lane, False
        if fused:
            self.backward_fused1(ap, gy)
        elif fold3:
            # the BatchNorm backward of the layer behind a 3x3 convolution, left pending by that layer's own backward
            # (`fold_ok`), rides in this convolution's data gradient (csrc/conv3s.hip MODE 4): the launch forms dL/dy from
            # (dz, y) while it stages its operand and writes it out for the weight gradient, which therefore comes SECOND
            gy = y._grad = t.empty(y.N, y.H, y.W, y.C)
            y.grad_amax, y.pending_apply = ap.bound, None
            self.dgrad(gy, ap)
            wl, defer_res = self.wgrad(gy)
        else:
            wl, defer_res = self.wgrad(gy)
            self.dgrad(gy, None)
        self.residual_grads(gy, wl, defer_res)

    def backward_ds(self, cd):
        """The backward of `Tape.conv_ds`: the two convolutions' own backwards over the same dL/dy, this op's (conv3) first (what
        bn3 and conv2 wait for).  The shortcut's is then the FIRST writer of dL/dx where its stand-alone trace made it the last;
        the sum of the two fp32 contributions is the same either way."""
        y = self.y
        if y.pending_apply is not None:
            self.tape.materialize_apply(y)
        assert y.grad is not None, 'no gradient reached conv output ' + self.name
        self.backward()
        cd.backward()

    def backward_fused1(self, ap, gy):
        """The one-launch backward of a 1x1 convolution (dsnt_conv1x1_bwd_f16x3).  ap: the pending BatchNorm backward of the op's
        consumer, applied in the operand load (else dL/dy = gy is read as it is)."""
        t, lib, bd = self.tape, self.tape.lib, self.tape.bounds
        src, x, y, p, g, name = self.src, self.x, self.y, self.p, self.g, 'dsnt_conv1x1_bwd_f16x3'
        nw = p.w.numel()
        shr = share(t)
        nsp = lib.dsnt_conv1x1_bwd_splits(C.byref(g), shr)
        ws = t.wgrads.slab(p, lib.dsnt_conv1x1_bwd_ws_floats(C.byref(g), shr), nsp)
        wd, wq16, wbd = bd.dgrad_f16(self.slot, self.slot_k, nw)
        total = bd.dgrad_total
        if ap is not None:
            aps, applied = bn_apply(y, ap)
            dy, gb = ap.dz, ap.bound
            y.pending_apply = None
            grad = dict(g_apply=applied, g_bound=gb)
        else:
            aps, dy, gb = None, gy, y.grad_amax
            grad = dict(g=dy, g_bound=gb)
        if self.normed:
            ab = bd.f16_bn_bound_bwd(src)
            # (the BatchNorm in front of THIS convolution may in turn be left to the 1x1 convolution before it)
            fold = t.fold_ok(src)
            dz = self.dz_buffer(fold)
            dz_amax = bd.amax_slot() if fold else None
            part = t.scratch('bnpart', nsp * 2 * x.C).view(-1)
            e = t.b(name, bn_epilogue(x, src), dy, aps, wq16, total, wbd, ab, gb, dz, part, ws, dz_amax, shr, g)
        else:
            # no BatchNorm in front of it (projection shortcuts, the `fc` convolutions): dL/dx itself is written, or
            # added to what x's gradient holds already
            ab = self.x_amax
            buf, acc = t.grad_target(x, amax=True)
            e = t.b(name, bn_epilogue(x, None), dy, None, wq16, total, wbd, ab, gb, buf, None, ws,
                    x.grad_amax, shr | acc, g)
        # (the tensors the launch names inside a struct: `emit` counts the plain arguments)
        t.bwd.count(name, 4 * (x.buf.numel() + (y.buf.numel() if ap is not None else 0)))
        self.use(e, 'bwd1', **self.a_operand(ab), w=wd, w_bound=wbd, **grad)
        if self.normed:
            t._norm_backward(src, dz, reduced=(part, nsp), finalised=False, dz_amax=dz_amax)

    def wgrad(self, gy):
        """Parameter gradients (flat arena, overwritten every step).  Returns (the lane they run on, whether dL/dy stays
        intact for them as the `base` of the residual inputs' gradients)."""
        t, p, g = self.tape, self.p, self.g
        cur = t.lane
        w6 = t.use_bf16x6 and bool(t.lib.dsnt_conv_wgrad_bf16x6_ok(C.byref(g)))
        defer_res = False
        with t.wgrads.placed(self, gy) as (wl, shr):
            if t.defer_reduce:
                defer_res = self.wgrad_slab(gy, shr, w6, wl == cur)
            else:
                ws = t.scratch('wgrad', t.lib.dsnt_conv_wgrad_ws_floats(C.byref(g)))
                t.b('dsnt_conv_wgrad_bf16x6' if w6 else 'dsnt_conv_wgrad', self.x.buf, self.sc, self.sh, self.relu, gy, ws, p.gw, p.gb, 0, g)
                if p.post_reduce is not None:      # the stem's space-to-depth gradient -> the parameter's 7x7 layout
                    t.b(p.post_reduce[0], *p.post_reduce[1])
        return wl, defer_res

    def wgrad_slab(self, gy, shr, w6, on_chain):
        """The weight gradient into a slab of its own that the bucket's one reduction launch sums (`WgradQueue.flush`): a launch here,
        or — low-resolution convolutions — a descriptor for the bucket's grouped launch.  Returns `defer_res`."""
        t, lib = self.tape, self.tape.lib
        x, y, p, g, normed, sc, sh, relu = self.x, self.y, self.p, self.g, self.normed, self.sc, self.sh, self.relu
        # deferred to the bucket's grouped launch: x, gy and the BN vectors are written once per
        # step and gy is not donated onwards (no residual inputs), so they are intact at the flush
        # (... nor shared with an activation whose gradient is accumulated into later: `share_grads`)
        # (a RAW operand — conv1 of a torchvision BasicBlock, resnet.py — rides with the identity prologue: scale 1, shift 0)
        groupable = (w6 and (normed or t.share_grads) and on_chain and not y.grad_shared and
                     0 < g.N * g.Ho * g.Wo <= t.group_rows)
        # ... or, WITH residual inputs (conv3 of the low-resolution Bottlenecks): dL/dy is not donated to them but
        # handed over as the `base` their own gradient continues out of place, and so stays intact as well
        residuals = [r for r in (self.res1, self.res2) if r is not None]
        defer_res = bool(groupable and residuals and t.share_grads and t.defer_res and all(r.untouched for r in residuals))
        grouped = groupable and (not residuals or defer_res)
        # fp16x3: both operand bounds exist (A: train-mode BN parameters, dY: one bn-backward apply wrote it)
        w16 = w6 and t.use_f16x3 and (normed or self.x_amax is not None) and y.grad_amax is not None
        ab = (t.bounds.f16_bn_bound_bwd(self.src) if normed else self.x_amax) if w16 else None
        if w16 and not grouped:
            # dsnt_conv_wgrad_f16x3 cuts the pixels of a 3x3 convolution into its own slabs (halo kernel)
            nws = lib.dsnt_conv_wgrad_f16x3_ws_floats(C.byref(g), shr)
            splits = lib.dsnt_conv_wgrad_f16x3_splits(C.byref(g), shr)
        else:
            nws, splits = lib.dsnt_conv_wgrad_ws_floats(C.byref(g)), lib.dsnt_conv_wgrad_splits(C.byref(g))
        ws = t.wgrads.slab(p, nws, splits)
        if grouped:
            desc = C.create_string_buffer(lib.dsnt_conv_wgrad_desc_bytes())
            gsc, gsh = (sc, sh) if normed else t.identity_bn(x.C)
            if w16:
                nblk = lib.dsnt_conv_wgrad_desc_f16x3(_lib.ptr(x.buf), _lib.ptr(gsc), _lib.ptr(gsh), relu, _lib.ptr(gy),
                                                      _lib.ptr(ws), _lib.ptr(ab), _lib.ptr(y.grad_amax), C.byref(g), desc)
            else:
                nblk = lib.dsnt_conv_wgrad_desc(_lib.ptr(x.buf), _lib.ptr(gsc), _lib.ptr(gsh), relu, _lib.ptr(gy),
                                                _lib.ptr(ws), C.byref(g), desc)
            if nblk <= 0:
                raise RuntimeError('dsnt_conv_wgrad_desc failed: %s' % lib.dsnt_last_error().decode())
            t.wgrads.group(desc.raw, nblk, self.use(None, 'wgrad', **self.a_operand(ab), g=gy, g_bound=y.grad_amax) if w16 else None)
        elif w16:
            e = t.b('dsnt_conv_wgrad_f16x3', x.buf, sc, sh, relu, gy, ws, None, None, shr, ab, y.grad_amax, g)
            self.use(e, 'wgrad', **self.a_operand(ab), g=gy, g_bound=y.grad_amax)
        else:
            t.b('dsnt_conv_wgrad_bf16x6' if w6 else 'dsnt_conv_wgrad', x.buf, sc, sh, relu, gy, ws, None, None,
                shr if w6 else 0, g)
        return defer_res

    def dgrad_operands(self, gy):
        """What the data gradient launches on: the geometry (`gd`, or — a strided convolution the phase kernel of csrc/dgrad_up.hip
        refuses — the stride-1 one over a zero-stuffed dL/dy) and the re-packed weights in the precision the launch takes."""
        t, x, p, g, bd = self.tape, self.x, self.p, self.g, self.tape.bounds
        nw = p.w.numel()
        pad_d = p.dil * (p.R - 1) - p.pad
        assert pad_d >= 0, 'data gradient needs pad <= dil * (R - 1)'
        # strided convolution (ResNet stage transitions): dsnt_conv_dgrad_strided computes the pixels of dX phase by phase
        # straight from dY
        native = p.stride != 1 and self.slot is not None and t.lib.dsnt_conv_dgrad_strided_ok(C.byref(g))
        gd, gsrc = self.gd, gy
        if p.stride != 1 and not native:
            # ... or, for the shapes that kernel refuses: the stride-1 data gradient of dY with zeros stuffed between the pixels
            Hs, Ws = x.H + 2 * p.pad - p.dil * (p.R - 1), x.W + 2 * p.pad - p.dil * (p.S - 1)
            gsrc = t.scratch('stuffed', x.N * Hs * Ws * p.Cout).view(-1)[:x.N * Hs * Ws * p.Cout]
            t.b('dsnt_zero_insert', gy, gsrc, x.N, g.Ho, g.Wo, p.Cout, Hs, Ws, p.stride)
            gd = ConvGeom(x.N, Hs, Ws, p.Cout, x.H, x.W, p.Cin, p.R, p.S, 1, pad_d, p.dil)
        wq = wq_stride = None
        if self.slot is not None:
            wd = bd.dgrad_f32[self.slot:self.slot + nw]
            wq, wq_stride = bd.dgrad_planes[self.slot:self.slot + nw], bd.dgrad_total
            d6 = gd is not None and use6(t, gd)
        else:       # stand-alone use without a parameter arena
            wd = t.scratch('wdgrad', nw)
            t.b('dsnt_conv_pack_dgrad', p.w, wd, p.Cout, p.R, p.S, p.Cin)
            d6 = use6(t, gd) and nw % 8 == 0
            if d6:
                wq, wq_stride = t.scratch('wdgrad6', 3 * nw, torch.bfloat16, 8), nw
                t.b('dsnt_split_bf16x3', wd, wq, nw)
        g_amax = self.y.grad_amax if (t.use_f16x3 and p.stride == 1) else None
        d16 = d6 and g_amax is not None and self.slot is not None and bd.dgrad_planes16 is not None
        d_stream = wq16 = wbd = None
        if d16:
            # (the data gradient's filter is [Cin][3][3][Cout]: its "Cout" is this convolution's Cin)
            d_stream = stream_ok(t, p, gd, None)
            _, wq16, wbd = bd.dgrad_f16(self.slot, self.slot_k, nw, (p.Cin, p.Cout) if d_stream else (0, 0))
        return _Dgrad(native, gd, gsrc, wd, wq, wq_stride, d6, g_amax, d16, d_stream, wq16, wbd)

    def dgrad_launch(self, d, out, res, part=None, bnb=None, tail=None):
        """out = data gradient [+ res], with the BatchNorm-backward epilogue bnb (partial sums into part) and the bound tail."""
        t = self.tape
        if d.native:
            t.b('dsnt_conv_dgrad_strided', d.gsrc, d.wd, out, res, part, self.g, bnb, tail)
        elif d.d16:
            e = t.b('dsnt_conv_fwd_f16x3_stream' if d.d_stream else 'dsnt_conv_fwd_f16x3_ex', d.gsrc, d.wq16, t.bounds.dgrad_total,
                    d.wbd, d.g_amax, None, out, None, None, share(t, d.d_stream or self.p.R == 1), res, None, part, d.gd, bnb, tail)
            self.use(e, 'dgrad', g=d.gsrc, g_bound=d.g_amax, w=d.wd, w_bound=d.wbd)
        elif d.d6:
            t.b('dsnt_conv_fwd_bf16x6_ex', d.gsrc, d.wq, d.wq_stride, None, out, None, None, 0, res, None, part, d.gd, bnb, tail)
        else:
            t.b('dsnt_conv_fwd_ex', d.gsrc, d.wd, None, out, None, None, 0, res, None, part, d.gd, bnb, tail)

    def dgrad(self, gy, ap):
        """The data gradient.  ap: the pending BatchNorm backward of the op's consumer, applied in the operand load of the
        launch, which also writes the dL/dy it forms to gy (`fold3`; None: gy is read)."""
        if not self.need_input_grad:
            return
        t, src, x, y = self.tape, self.src, self.x, self.y
        d = self.dgrad_operands(gy)
        if not self.normed:
            # (d6: the large-tile kernels; their epilogue can leave max|written gradient| as the next bound)
            buf, acc, base = t.grad_target_base(x, amax=bool(d.d6 or d.native))      # (base: the residual operand)
            tl = tail_at(x.grad_amax) if x.grad_amax is not None else None
            self.dgrad_launch(d, buf, base if base is not None else (buf if acc else None), tail=tl)
            return
        # the ReLU mask and the two per-channel sums of the BatchNorm backward ride in the
        # data-gradient epilogue; only finalise + apply remain as separate launches
        # (fold: the 1x1 convolution that produced x forms this BatchNorm's dx in its own backward — dz then has
        # to outlive this op's launches, and its maximum is what the bound of dx is made from)
        fold = not d.native and t.fold_ok(src)
        dz = self.dz_buffer(fold)
        tiles = t.lib.dsnt_conv_dgrad_strided_tiles(C.byref(self.g)) if d.native else stats_tiles(t, d.gd, d.d6)
        part = t.scratch('bnpart', tiles * 2 * x.C).view(-1)
        bnb = bn_epilogue(x, src)
        tl, dz_amax = None, None
        if fold:
            dz_amax = t.bounds.amax_slot()
            tl = tail_at(dz_amax)
        if ap is not None:
            assert d.d16 and d.d_stream and not d.native
            name = 'dsnt_conv_dgrad_f16x3_stream_apply'
            aps, applied = bn_apply(y, ap)
            e = t.b(name, ap.dz, aps, gy, d.wq16, t.bounds.dgrad_total, d.wbd, ap.bound, dz, part, share(t), d.gd, bnb, tl)
            t.bwd.count(name, 4 * y.buf.numel())
            self.use(e, 'dgrad', w=d.wd, w_bound=d.wbd, g_bound=ap.bound, g_apply=applied)
        else:
            self.dgrad_launch(d, dz, None, part, bnb, tl)
        t._norm_backward(src, dz, reduced=(part, tiles), dz_amax=dz_amax)

    def residual_grads(self, gy, wl, defer_res):
        """The gradients of the residual inputs, last: gy is dead after the op's own launches (the weight-gradient lane must have
        read it before anyone accumulates into the donated buffer)."""
        t, y = self.tape, self.y
        if self.res1 is not None or self.res2 is not None:
            t.sync_bwd(wl, t.lane)
        donated = False
        for r in (self.res1, self.res2):
            if r is None:
                continue
            if defer_res:
                r.base, r.base_amax = gy, y.grad_amax
            elif (donated and t.share_grads and r.grad is None and r.pending_apply is None and r.uses == 1 and
                    not r.gives_away and not r.is_branch):
                # the buffer went to the first residual input; this one has a single consumer, so its gradient is dL/dy
                # and nothing else, and its producer only READS it (it gives no buffer away): shared, not copied.  Every
                # later writer of the buffer comes after that reader in lane order, or waits for the lane that reads
                # (`WgradQueue.before_write` goes by the buffer)
                r.grad, r.grad_amax, r.grad_shared = gy, y.grad_amax, True
            else:
                donated = t.grad_identity(r, gy, donate=not donated, g_amax=y.grad_amax) or donated
