"""Static launch-list engine for the hourglass backbone on MI355X.

The reference runs the backbone as ~300 separate PyTorch modules per pass
(`/root/reference/src/dsnt/hourglass.py:30-50,78-90,155-177`) and lets autograd record them
every step.  Here the module tree is traced ONCE per (batch shape, mode) into two flat lists of
C-ABI kernel launches (forward, backward) over pre-allocated NHWC buffers; a step is a replay
of those lists on the current HIP stream (no allocation, no Python graph building, capturable
into a hipGraph).  Fusions decided at trace time:

* BatchNorm+ReLU in front of a conv is folded into the conv's operand load (scale/shift per
  input channel); its batch statistics come from the *producer's* epilogue (per-tile column
  sums written by the previous conv), so a pre-activation Bottleneck is 3 conv launches + 3
  tiny finalise launches instead of 10 elementwise passes;
* residual / skip adds ride in the conv epilogue (up to two addends);
* in backward, identity branches donate the incoming gradient buffer instead of copying, and
  every kernel that produces a gradient can accumulate in place, so fan-in costs no extra pass.

Gradients with respect to parameters are written straight into one flat arena (the same arena
the fused optimiser and the RCCL all-reduce operate on).

This module is the tape: buffers, lanes, gradient plumbing, BatchNorm bookkeeping and the element-wise ops.  The convolution —
its forward choice, its backward plan and everything its backward emits — is a `ConvOp` (dsnt.convop) that `Tape.conv` and
`Tape.conv_ds` build; the launch lists, the operand bounds and the weight-gradient queue are dsnt.launchlist, dsnt.bounds and
dsnt.wgrad_queue.
"""
import os

import torch

from . import _lib, convop
from ._lib import ConvGeom, BnTail
from .bounds import Bounds
from .launchlist import Lanes, LaunchList
from .wgrad_queue import WgradQueue

BN_EPS = 1e-5
BN_MOMENTUM = 0.1


class Act:
    """An activation on the tape: NHWC buffer + lazily created gradient / batch statistics."""
    __slots__ = ('buf', 'N', 'H', 'W', 'C', '_grad', 'stats', 'name', 'grad_amax', 'amax_tail', 'fold_ok',
                 'pending_apply', 'uses', 'gives_away', 'is_branch', 'grad_shared', 'pending_add', 'base', 'base_amax')

    def __init__(self, buf, name=''):
        self.buf = buf
        self.N, self.H, self.W, self.C = buf.shape
        self._grad = None       # torch tensor once some backward op has written it (`grad`)
        # a gradient this activation's CONTINUES without owning it (`ConvOp.residual_grads`, `defer_res`): the next writer writes
        # base + its value into a buffer of its own (`Tape.grad_target`), so that the base stays intact for a deferred reader
        self.base, self.base_amax = None, None
        self.stats = None       # (partial tensor, ntiles)
        self.amax_tail = None   # fp16x3: the dsnt_out_bounds of the producing launch if it can leave max|buf| (operand_amax)
        self.grad_amax = None   # fp16x3: device scalar max|grad| when ONE bn-backward apply wrote the whole gradient
        self.fold_ok = False    # the producing 1x1 convolution can take the BatchNorm backward of its consumer into its own backward
        self.pending_apply = None   # ... and this is that BatchNorm backward, reduced but not applied (Tape._norm_backward)
        self.uses = 0           # forward consumers (each contributes once to the gradient)
        self.gives_away = False     # the producer's backward DONATES this gradient's buffer onwards (residual inputs, upsample + add)
        self.is_branch = False  # `Tape.branch`: an alias of another activation (its gradient is joined to that one's)
        self.grad_shared = False    # .grad is another activation's buffer, read in place (Tape.share_grads): readers must not be deferred
        self.pending_add = None     # (gradient tensor, its bound slot) the NEXT writer of .grad adds in its own pass (Tape.add_later)
        self.name = name

    @property
    def M(self):
        return self.N * self.H * self.W

    @property
    def untouched(self):
        """No gradient has reached this activation in any form: it can still start as another's `base`."""
        return self._grad is None and self.base is None and self.pending_apply is None and self.pending_add is None

    @property
    def grad(self):
        if self._grad is None and self.base is not None:
            # read before any further writer came: the gradient IS the base, read in place (`base` stays set: a later writer
            # still goes out of place, `Tape.grad_target`)
            self._grad, self.grad_amax, self.grad_shared = self.base, self.base_amax, True
        return self._grad

    @grad.setter
    def grad(self, g):
        self._grad = g


class ConvParams:
    """Views into the parameter / gradient arenas for one convolution (weights are OHWI)."""
    __slots__ = ('w', 'b', 'gw', 'gb', 'Cout', 'R', 'S', 'Cin', 'stride', 'pad', 'dil', 'wq', 'wq_stride', 'wq16', 'wb',
                 'post_reduce')

    def __init__(self, w, b, gw, gb, stride=1, pad=0, dil=1):
        self.w, self.b, self.gw, self.gb = w, b, gw, gb
        self.wq, self.wq_stride = None, 0      # bf16x6 planes of w (plane 0 view, plane stride)
        self.wq16, self.wb = None, None        # fp16x3: fp16 planes (same stride) and the device scalar max|w|
        self.post_reduce = None                # (name, args) launched after the slab reduction that writes gw (stem_s2d)
        self.Cout, self.R, self.S, self.Cin = w.shape
        self.stride, self.pad, self.dil = stride, pad, dil


class BnParams:
    __slots__ = ('gamma', 'beta', 'ggamma', 'gbeta', 'rmean', 'rvar', 'C', 'uses', 'momentum', 'eps')

    def __init__(self, gamma, beta, ggamma, gbeta, rmean, rvar, momentum=BN_MOMENTUM, eps=BN_EPS):
        self.gamma, self.beta, self.ggamma, self.gbeta = gamma, beta, ggamma, gbeta
        self.rmean, self.rvar = rmean, rvar
        self.momentum, self.eps = float(momentum), float(eps)
        self.C = gamma.numel()
        self.uses = 0           # backward accumulates dgamma/dbeta from the second use on


class Normed:
    """x seen through a BatchNorm(+ReLU): what a fused conv prologue needs."""
    __slots__ = ('x', 'bn', 'mean', 'invstd', 'scale', 'shift', 'relu', 'abound', 'pending', 'lane')


class PendingApply:
    """A BatchNorm backward reduced but not applied (`Tape._norm_backward` with dz_amax): dz, the Normed it goes through, its
    two coefficients per channel, the bound slots of the dx to be formed and of dz."""
    __slots__ = ('dz', 'n', 'coef', 'bound', 'dz_amax')

    def __init__(self, dz, n, coef, bound, dz_amax):
        self.dz, self.n, self.coef, self.bound, self.dz_amax = dz, n, coef, bound, dz_amax


class Tape:
    def __init__(self, device, training, record=None, want_input_grad=False):
        self.device = device
        # `training` is the BatchNorm mode (batch statistics vs running statistics, nn.Module.train / eval); `record` says
        # whether a backward list is built.  They differ for a backward through an EVAL-mode forward (frozen BatchNorm
        # statistics: dx = scale dz, the two reductions only feed dgamma / dbeta) — rare (bin/train.py never does it), so that
        # program runs on the bound-free kernels: bf16x6, none of the fp16x3-only fused kernels
        self.training = training
        self.record = training if record is None else bool(record)
        self.want_input_grad = want_input_grad      # d loss / d image is asked for: the stem keeps its data gradient
        self._bwd_emitters = []
        self._scratch = {}
        self._keep = []         # keeps ctypes structs / tensors alive
        self.lib = _lib.load()
        self.nbytes = 0
        self._read_switches()
        # the two launch lists (dsnt.launchlist), replayed from C: recorded once into the library, then issued by ONE call per segment
        lanes = Lanes(self.use_lanes, self.n_lanes)
        self.fwd, self.bwd = (LaunchList(self.lib, lanes, self._keep) for _ in range(2))
        self.bounds = Bounds(self)          # fp16x3 operand bounds and the per-step preparation (dsnt.bounds)
        self.wgrads = WgradQueue(self)      # weight gradients held back, grouped and reduced per bucket (dsnt.wgrad_queue)
        self.lane = 0           # the lane being traced onto
        self.cur_bucket = 0         # parameter bucket of the layers being traced (mark_bucket)
        self._ident = None
        self.acts = []          # every activation in creation order (debugging / introspection)
        self.param_arena = None  # flat fp32 parameter arena (set by the Program) for the one-launch pack
        self._planar_src = {}
        # every fp16x3 launch with the tensors behind its operands and bounds: (list entry, {...}) — lets a test walk a
        # step launch by launch and hold each bound against the operand it must dominate (tests/test_bounds_gpu.py)
        self.f16_uses = []

    def _read_switches(self):
        """The switches and thresholds of the schedule: product defaults, each with the environment variable that overrides it
        for an A/B measurement or a test (read once, when the tape is created)."""
        # fp32-accurate split-bf16 matrix-core path for the large convolutions (DSNT_MFMA=f32 disables)
        self.use_bf16x6 = os.environ.get('DSNT_MFMA', 'bf16x6') != 'f32'
        # (16384 -> 8192, the 16x16 level at batch 32: -0.08 ms; -> 4096 once fwd1 took the 1x1 convolutions of that size: the 16x16
        # level at batch 16, hg8 -0.08 ms, nothing between 4096 and 8192 rows at batch 32; 2048: +0.07 ... +0.09)
        self.bf16x6_min_rows = int(os.environ.get('DSNT_BF16X6_MIN_ROWS', '4096'))
        # lanes: 0 = the caller's stream, 1 = a side stream for independent branches (the full-resolution
        # skip branch of every hourglass level runs beside the low-resolution recursion)
        self.use_lanes = os.environ.get('DSNT_LANES', '1') != '0'
        # lanes 3.. : more side lanes (the skip branches of the hourglass levels alternate over them: an inner level's
        # branch, which the main lane needs back first, does not queue behind the outer level's large kernels)
        self.side_lanes = (1, 3)   # two side lanes (one: +0.13 ms, four: +0.35 ms: DESIGN.md "round 2")
        self.n_lanes = 3 + len(self.side_lanes) - 1
        self.chain_lanes = (0,) + self.side_lanes
        # weight gradients feed nothing downstream in backward.  The large ones (>= DSNT_X_WGRAD_LANE_ROWS output rows; 0 =
        # all) of the chain's lanes go to a third lane: the chip then has work while the dependency chain walks the launch-bound
        # low-resolution levels, and the main lane neither runs nor waits for the slab reductions (-0.9 ms/step on hg2).
        # Not the convolutions with residual inputs, whose dY buffer is donated onwards and written again — the writer then
        # has to wait for the lane (measured: +0.45 ms).
        self.wgrad_lane = 2 if (self.use_lanes and os.environ.get('DSNT_WGRAD_LANE', '1') != '0') else None
        self.wgrad_lane_rows = int(os.environ.get('DSNT_X_WGRAD_LANE_ROWS', '16000'))
        # ... and they are HELD BACK (launches collected, not yet on the list) until the chain enters a launch-bound
        # phase: a `release point` is the backward of an up-sampling whose low-resolution operand has at most
        # DSNT_X_RELEASE_ROWS rows.  Issued as they come, the weight gradients share the chip with the large
        # data-gradient kernels and are gone by the time the small levels start; held back, they run beside them.
        # Only while a release point is still ahead in the backward order (a ResNet has none: nothing is held back).
        # (8192 -> 4096 in round 6: at batch 32 the 16 x 16 level — 8192 rows — still fills the chip by itself; released one level
        # further in, the held weight gradients run beside the 8 x 8 / 4 x 4 chains only: hg2 -0.07 ms, hg8 batch 16 unchanged — its
        # 16 x 16 level has 4096 rows; profiles/r06_ab_switches.txt box A)
        self.release_rows = int(os.environ.get('DSNT_X_RELEASE_ROWS', '4096'))
        off = set(os.environ.get('DSNT_OFF', '').replace('+', ',').split(','))       # DSNT_OFF=conv3s,gemm1,wgrad3,wgrad1
        # 3x3 forward / data gradient: the symmetric persistent kernel of csrc/conv3s.hip (stream-ordered weight planes)
        self.conv3s = 'conv3s' not in off
        # the whole backward of a 1x1 convolution in one launch (csrc/bwd1.hip): data gradient with the BatchNorm-backward
        # epilogue + weight gradient + (conv1 of a Bottleneck) the BatchNorm backward of the layer behind, each tensor read once
        self.bwd1 = 'bwd1' not in off
        self.fwd1 = 'fwd1' not in off      # ... and their forward (csrc/fwd1.hip)
        # round 5: the BatchNorm backward behind a 3x3 convolution folded into that convolution's data gradient (conv3s.hip MODE 4)
        self.fold3 = 'fold3' not in off
        self.fold3_rows = int(os.environ.get('DSNT_X_FOLD3_ROWS', '16384'))
        self.stem4 = 'stem4' not in off    # the stem's forward (csrc/stem4.hip)
        # conv3 of a Bottleneck and its projection shortcut (the stem's layer1 and layer3) as one forward launch: the skip tensor
        # is neither written nor read back (`ds_fuse_ok`; DSNT_OFF=dsfuse: two launches).  From DSNT_X_DS_FUSE_ROWS rows: the
        # 128 x 128 and 64 x 64 levels from batch 4 and 16 on.
        self.ds_fuse = 'dsfuse' not in off
        self.ds_fuse_rows = int(os.environ.get('DSNT_X_DS_FUSE_ROWS', '65536'))
        # DSNT_X=<name>=<value>,...: A/B overrides of scheduling constants (tools/ab_env.sh); not product switches
        self._x = dict(kv.split('=') for kv in os.environ.get('DSNT_X', '').split(',') if '=' in kv)
        self.wgrad_narrow = self._x.get('wgrad_narrow', '1')      # DSNT_WGRAD_NARROW: 0 never, 1 always, 2 stem bucket only, 3 stacks only
        # a gradient shared instead of copied (A/B: DSNT_X=share_grads=0): a second residual input with ONE consumer reads dL/dy in
        # place (hourglass.py:175: x + fc_ + score_ — fc_'s gradient IS the sum's): one 268 MB pass per intermediate supervision,
        # 7 per hg8 step.  (The OTHER pass there — x.grad += the skip branch's gradient, Hourglass._level — stays: both buffers
        # arrive by donation, and folding the sum into the branch's last apply would need a five-stream form of that kernel.)
        self.share_grads = self._x.get('share_grads', '1') != '0'
        # the weight gradient of a low-resolution convolution WITH residual inputs (conv3 of a Bottleneck: 2-32 workgroups, 17-25 us
        # on the dependency chain each; 15 per hg2 step, 63 per hg8 step) joins its bucket's grouped launch too: its dL/dy is not
        # donated to the residual input but becomes the `base` that input's gradient continues out of place (Act.base)
        self.defer_res = self._x.get('defer_res', '1') != '0'
        self.flush_points = self._x.get('flush_points', '1') != '0'       # `flush_point` (A/B)
        # the per-step preparation in two halves: what the FORWARD reads (arena planes, weight planes, BatchNorm bounds) and what only
        # the backward reads (re-packed + split data-gradient weights); the main lane waits for the first half only (A/B: prep_split=0)
        self.prep_split = self._x.get('prep_split', '1') != '0'
        # weight-gradient slabs are kept per convolution and reduced once per parameter bucket (one launch
        # instead of one per convolution); DSNT_DEFER_REDUCE=0 reduces inside every dsnt_conv_wgrad call
        self.defer_reduce = os.environ.get('DSNT_DEFER_REDUCE', '1') != '0'
        # weight gradients of the low-resolution levels (few workgroups each, nothing downstream in backward
        # needs them) wait for the end of their parameter bucket and run side by side in one grouped launch;
        # DSNT_X_GROUP_ROWS = largest N*Ho*Wo that is deferred (0 disables)
        self.group_rows = int(os.environ.get('DSNT_X_GROUP_ROWS', '8192')) if self.defer_reduce else 0
        # BatchNorm finalisation of few-tile statistics inside the consumer's prologue (DSNT_FUSE_FINALIZE=0: separate launches)
        self.fuse_finalize = os.environ.get('DSNT_FUSE_FINALIZE', '1') != '0'
        # ... up to this many (tiles x channels) of partial sums.  Measured (tools/bench_bn_prologue.py, MI355X): a finalise
        # launch costs the chain 4-5 us; the prologue costs every workgroup of the consumer 2.8 us at 16 KB of partials,
        # 3.2 us at 32 KB, 4.5 us at 64 KB (no gain), 9 us at 128 KB (a loss): fused up to 32 KB
        # (round 4, with one statistics row per workgroup from the 1x1 kernels: hg2 is indifferent between 0 and 4096 — 12.00-12.03
        # ms — and hg8 at batch 16 is best at 2048: 26.64 vs 26.84 at 4096, 26.76 at 1024, 26.99 with separate launches only)
        self.fuse_finalize_max = int(os.environ.get('DSNT_X_FUSE_FINALIZE_MAX', '2048'))
        # fp16x3 (default; DSNT_SPLIT=bf16x6 turns it off): two fp16 planes + three MFMAs instead of three bf16 planes + six, where an operand
        # bound is available without a host round-trip: train-mode BN+ReLU operands (bound from the BN parameters) and
        # weights (amax in the per-step prep launch)
        self.use_f16x3 = self.use_bf16x6 and os.environ.get('DSNT_SPLIT', 'f16x3') == 'f16x3'
        if self.record and not self.training:
            self.use_f16x3 = False      # (its backward operand bounds come from BATCH statistics: |xhat| <= sqrt(M))
        self.no_relu = bool(os.environ.get('DSNT_DEBUG_NO_RELU'))   # smooth network for exact gradient checks

    # ------------------------------------------------------------------ buffers
    def empty(self, *shape, dtype=torch.float32):
        t = torch.empty(*shape, device=self.device, dtype=dtype)
        self.nbytes += t.numel() * t.element_size()
        self._keep.append(t)
        return t

    def scratch(self, key, numel, dtype=torch.float32, least=1):
        """Shared scratch (valid only within one op's launches on the single stream)."""
        key = (key, self.lane)
        t = self._scratch.get(key)
        if t is None or t.numel() < numel:
            if t is not None:
                self._keep.append(t)   # earlier launches recorded the old pointer
            t = torch.empty(max(numel, least), device=self.device, dtype=dtype)
            self.nbytes += t.numel() * t.element_size()
            self._scratch[key] = t
        return t

    def upload(self, rows, dtype=torch.int64):
        """A table of a table-driven launch, on the device and kept alive."""
        t = torch.tensor(rows, dtype=dtype).to(self.device)
        self._keep.append(t)
        return t

    def act(self, N, H, W, Cc, name=''):
        a = Act(self.empty(N, H, W, Cc), name)
        self.acts.append(a)
        return a

    # ------------------------------------------------------------------ emission helpers
    def f(self, name, *args):
        return self.fwd.emit(self.lane, name, *args)

    def b(self, name, *args):
        return self.bwd.emit(self.lane, name, *args)

    def b_amax(self, name, *args, amax):
        """`name`, or — the gradient it writes has a bound slot — `name`_amax, which leaves max|written| in that slot."""
        return self.b(name, *args) if amax is None else self.b(name + '_amax', *args, amax)

    bytes_fwd = property(lambda self: self.fwd.nbytes)
    bytes_bwd = property(lambda self: self.bwd.nbytes)

    @property
    def bytes_by_name(self):
        both = dict(self.fwd.bytes_by_name)
        for name, nb in self.bwd.bytes_by_name.items():
            both[name] = both.get(name, 0) + nb
        return both

    def on_backward(self, fn):
        lane = self.lane

        def emit():
            saved, self.lane = self.lane, lane
            try:
                fn()
            finally:
                self.lane = saved
        self._bwd_emitters.append(emit)

    # ------------------------------------------------------------------ lanes
    def sync(self, src, dst, bwd=True):
        """`dst` lane waits for everything emitted so far on `src`; mirrored in backward unless bwd=False."""
        if not self.use_lanes:
            return
        self.fwd.sync(src, dst)
        if self.record and bwd:
            self._bwd_emitters.append(lambda: self.bwd.sync(dst, src))

    def sync_bwd(self, src, dst):
        """Backward-list only: `dst` lane waits for what has been emitted on `src` so far."""
        if self.use_lanes and src != dst:
            self.bwd.sync(src, dst)

    def branch(self, x, join=True):
        """Alias of activation x for a branch traced on the side lane: same buffer and statistics,
        private gradient (the two lanes must not accumulate into one buffer concurrently); the
        private gradient is added to x's after the lanes have joined in backward (join=False: the
        caller hands it over itself — Hourglass._level)."""
        if not self.use_lanes:
            return x
        xb = Act(x.buf, x.name + '/branch')
        xb.stats, xb.amax_tail = x.stats, x.amax_tail
        xb.is_branch = True
        x.uses += 1
        if self.record and join:
            def join_grad():
                if xb.grad is not None:
                    self.grad_identity(x, xb.grad, donate=False, g_amax=xb.grad_amax)
            self.on_backward(join_grad)        # registered first -> runs after the branch's backward
        return xb

    def finish(self):
        """Emit the backward list (reverse order of the forward ops)."""
        self.bounds.close_dgrad()
        prep_pos = len(self.bwd)
        self.wgrads.begin_backward()
        for fn in reversed(self._bwd_emitters):
            fn()
        self._bwd_emitters = []
        self.bounds.emit_backward_zero(prep_pos)
        if self.wgrads.pending:           # convolutions outside every parameter bucket (stand-alone modules)
            self.wgrads.flush()

    def mark_bucket(self, k):
        """Forward position where parameter bucket k starts being used: in the (reversed) backward
        list the marker lands right after the last launch that writes bucket k's gradients."""
        self.cur_bucket = k
        if self.record:
            self.on_backward(lambda: self.wgrads.flush(bucket=k))

    def flush_point(self):
        """Forward position behind which (in backward: before which) the weight-gradient slabs written so far are reduced and the
        grouped low-resolution weight gradients launched, without closing the parameter bucket.  A ResNet is ONE bucket: all of its
        grouped weight gradients (every convolution of <= 8192 rows: 337 us at batch 8) and its one slab reduction (128 us) used to
        run behind the last data gradient, with nothing beside them; flushed after every stage they run on the weight-gradient
        lane beside the next stage's launch-bound chain.  (On the hourglass the same cut inside the stem's bucket gains nothing:
        profiles/r05_ab_switches.txt box B.)"""
        if self.record and self.defer_reduce and self.flush_points:
            self.on_backward(self.wgrads.flush)

    def run(self, lst, bucket_hook=None, probe=None):
        """Replay one of the tape's lists.  `probe(entry)` (diagnostics / tests) is called before every launch."""
        lst.replay(bucket_hook, probe)

    # ------------------------------------------------------------------ gradient plumbing
    def add_later(self, a, g, g_amax=None):
        """a.grad += g, left to the next writer of a.grad if that writer can add a second tensor in its own pass
        (`maxpool2`'s backward: dsnt_maxpool2_bwd_add); any other writer first emits the addition as a launch of its own."""
        assert a.grad is not None and a.pending_add is None
        a.pending_add = (g, g_amax)

    def _flush_add(self, a):
        (g, g_amax), a.pending_add = a.pending_add, None
        self.grad_identity(a, g, donate=False, g_amax=g_amax)

    def identity_bn(self, Cc):
        """(ones, zeros) of >= Cc channels: the BatchNorm prologue that changes nothing (a raw operand for a launch form that only
        exists with a prologue — the grouped weight gradients)."""
        if self._ident is None or self._ident[0].numel() < Cc:
            n = max(Cc, 2048)
            self._ident = (torch.ones(n, device=self.device), torch.zeros(n, device=self.device))
        return self._ident

    def grad_target(self, a, amax=False, take_add=False):
        """(buffer, accumulate flag) for a kernel about to write a's gradient.  `amax`: the kernel leaves max|written|
        in a.grad_amax (fp16x3 operand bound).  Every writer rewrites the whole tensor, so the slot stays a valid bound
        while all writers since its creation report into it; a writer that cannot invalidates it."""
        buf, acc, base = self.grad_target_base(a, amax, take_add)
        if base is not None:        # this writer cannot read the base itself: it finds a copy in place
            self.b_amax('dsnt_axpy', base, buf, 1.0, 0, base.numel(), amax=a.grad_amax)
            acc = 1
        return buf, acc

    def grad_target_base(self, a, amax=False, take_add=False):
        """`grad_target` for a writer that can add a third tensor in its own pass: (buffer, accumulate flag, base).  base (or
        None): a's gradient continues one it does not own — base + this writer's value go into the buffer, a NEW one."""
        if a.pending_apply is not None:          # a BatchNorm backward left to a's producer, and now a second contribution
            self.materialize_apply(a)
        if a.pending_add is not None and not take_add:
            self._flush_add(a)                   # this writer cannot add a second tensor in its pass: the separate launch after all
        if a.base is not None:
            base, a.base, a.base_amax = a.base, None, None
            a._grad, a.grad_shared = self.empty(a.N, a.H, a.W, a.C), False
            a.grad_amax = self.bounds.amax_slot() if (self.use_f16x3 and amax) else None
            return a._grad, 0, base
        acc = 1
        if a.grad is None:
            a.grad = self.empty(a.N, a.H, a.W, a.C)
            acc = 0
        else:
            self.wgrads.before_write(a.grad)
        if self.use_f16x3 and amax:
            if a.grad_amax is None:
                a.grad_amax = self.bounds.amax_slot()
        else:
            a.grad_amax = None
        return a.grad, acc, None

    def grad_identity(self, a, g, donate, g_amax=None):
        """a.grad (+)= g.  With `donate`, g's buffer is handed over when a has no gradient yet
        (the caller guarantees g is dead after its own launches).  Returns True if donated.
        g_amax: the bound slot of g, if it has one (it moves with a donated buffer)."""
        if a.pending_apply is not None:
            self.materialize_apply(a)
        if a.pending_add is not None:
            self._flush_add(a)
        if a.grad is None and donate:
            a.grad = g
            a.grad_amax = g_amax
            return True
        buf, acc = self.grad_target(a, amax=True)
        self.b_amax('dsnt_axpy', g, buf, 1.0, acc, g.numel(), amax=a.grad_amax)
        return False

    # ------------------------------------------------------------------ ops
    def geom(self, x, p):
        Ho = (x.H + 2 * p.pad - p.dil * (p.R - 1) - 1) // p.stride + 1
        Wo = (x.W + 2 * p.pad - p.dil * (p.S - 1) - 1) // p.stride + 1
        assert x.C == p.Cin, (x.C, p.Cin)
        return ConvGeom(x.N, x.H, x.W, p.Cin, Ho, Wo, p.Cout, p.R, p.S, p.stride, p.pad, p.dil)

    def ensure_stats(self, a):
        if a.stats is None:
            tiles = (a.M + 127) // 128
            part = self.empty(tiles, 2, a.C)
            self.f('dsnt_bn_stats', a.buf, part, a.M, a.C)
            a.stats = (part, tiles)
        return a.stats

    def finalize_in_consumer(self, bn, tiles):
        """`tiles` rows of partial sums of bn's channels are few enough for the launch that consumes them to finalise them in its
        prologue (forward: the statistics, backward: dgamma / dbeta / coef) instead of a finalise launch of their own."""
        return self.fuse_finalize and bn.C <= 256 and tiles * bn.C <= self.fuse_finalize_max

    def norm(self, x, bn, relu=True):
        """BatchNorm bookkeeping for x under `bn`: finalise kernel -> scale/shift vectors."""
        if self.no_relu:
            relu = False
        n = Normed()
        n.x, n.bn, n.relu = x, bn, relu
        n.abound = None
        n.mean, n.invstd, n.scale, n.shift = (self.empty(bn.C) for _ in range(4))
        n.pending = None
        n.lane = self.lane      # the lane whose launches write scale / shift: every consumer must run there (`check_lane`)
        if self.training:
            n.pending = self.ensure_stats(x)
            # few tiles (the 8x8 / 4x4 levels): the launch that CONSUMES this BatchNorm finalises it in its prologue
            # (`conv`); any other first reader materialises it with the usual launch (`materialize`), as do many tiles here
            if not self.finalize_in_consumer(bn, n.pending[1]):
                self.materialize(n)
        else:
            self.bounds.eval_bn(n)
        return n

    def check_lane(self, n):
        """A consumer of Normed n is about to be emitted on the current lane.  The vectors of n are written by launches of ONE
        lane (the finalise launch at `norm` time, or — deferred — the first consumer's prologue / `materialize`), and nothing
        orders another lane's reader behind them: a second consumer elsewhere would race silently."""
        if n.pending is not None:
            n.lane = self.lane              # this consumer finalises it, here
        elif n.lane != self.lane:
            raise RuntimeError('dsnt: BatchNorm vectors finalised on lane %d are read on lane %d without a synchronisation '
                               '(trace norm() and its consumers on one lane, or sync the lanes)' % (n.lane, self.lane))

    def materialize(self, n):
        """The separate finalise launch of a BatchNorm whose finalisation was left to its consumer (`norm`)."""
        self.check_lane(n)
        if n.pending is not None:
            part, tiles = n.pending
            n.pending = None
            bn = n.bn
            self.f('dsnt_bn_finalize', part, tiles, n.x.M, bn.C, bn.gamma, bn.beta, bn.rmean, bn.rvar,
                   bn.momentum, bn.eps, 1, n.mean, n.invstd, n.scale, n.shift)

    def fold_ok(self, n):
        """The BatchNorm backward of Normed n can be left to the backward of the convolution that produced n.x."""
        x = n.x
        return bool(self.bwd1 and x.fold_ok and x.grad is None and x.pending_apply is None)

    def materialize_apply(self, x):
        """The apply launch of a BatchNorm backward that was left to x's producer (`_norm_backward` with dz_amax) after all:
        x got a second gradient contribution, so its gradient has to exist in memory."""
        ap, x.pending_apply = x.pending_apply, None
        n = ap.n
        buf, acc = self.grad_target(x, amax=True)
        self.b_amax('dsnt_bn_act_bwd_apply', ap.dz, x.buf, n.scale, n.shift, n.mean, n.invstd, ap.coef, 0,
                    buf, acc, x.M, n.bn.C, amax=x.grad_amax)

    def _norm_backward(self, n, da, reduced=None, finalised=False, dz_amax=None):
        """Given da = dL/d relu(bn(x)), accumulate dx into n.x.grad and dgamma/dbeta.  With
        `reduced` = (partials, ntiles) the producer already masked da by the ReLU and reduced it; with `finalised` it
        also wrote dgamma / dbeta / coef.  With dz_amax (the slot in which the producer left max|da|; the
        caller has asked `fold_ok`) dx is NOT written: the finalise launch also leaves the bound of dx, and the backward
        of the 1x1 convolution that produced x forms dx in registers (dsnt_conv1x1_bwd_f16x3)."""
        x, bn = n.x, n.bn
        coef = self.scratch('bncoef', 2 * bn.C)
        relu = 1 if n.relu else 0
        if reduced is not None:
            part, tiles = reduced
            relu = 0                      # da is already dz
        else:
            tiles = (x.M + 127) // 128
            part = self.scratch('bnpart', tiles * 2 * bn.C).view(-1)
            self.b('dsnt_bn_act_bwd_reduce', da, x.buf, n.scale, n.shift, n.mean, n.invstd, relu, part,
                   x.M, bn.C)
        if dz_amax is not None:
            assert reduced is not None and not finalised and x.grad is None
            acc_p = 1 if bn.uses > 0 else 0
            bn.uses += 1
            coef = self.empty(2 * bn.C)          # lives until the producer's backward
            bound = self.bounds.amax_slot()
            self.b('dsnt_bn_bwd_finalize_bound', part, tiles, x.M, bn.C, bn.ggamma, bn.gbeta, acc_p, coef, n.scale,
                   dz_amax, bound)
            x.pending_apply = PendingApply(da, n, coef, bound, dz_amax)
            return
        # eval-mode forward: the statistics are constants — dx = scale dz, i.e. the apply with both coefficients zero
        # (DSNT_BN_FROZEN); the two sums still are dbeta / dgamma
        frozen = not self.training
        fused = (not finalised) and self.finalize_in_consumer(bn, tiles) and not frozen
        assert not (frozen and finalised)
        if not finalised:
            acc_p = 1 if bn.uses > 0 else 0
            bn.uses += 1
            if not fused:
                self.b('dsnt_bn_bwd_finalize', part, tiles, x.M, bn.C, bn.ggamma, bn.gbeta, acc_p | (2 if frozen else 0), coef)
        buf, acc, base = self.grad_target_base(x, amax=True)    # (base: dx = base + value, `conv`'s defer_res)
        if fused:
            # few tiles: the apply launch sums them itself in its prologue (coef) and writes dgamma / dbeta
            coef = self.empty(2 * bn.C)          # private: the launch writes it (a shared scratch could still be in use)
            if base is not None:
                self.b('dsnt_bn_act_bwd_apply_pro_base', da, x.buf, n.scale, n.shift, n.mean, n.invstd, part, tiles,
                       bn.ggamma, bn.gbeta, acc_p, coef, relu, base, buf, x.M, bn.C, x.grad_amax)
            else:
                self.b('dsnt_bn_act_bwd_apply_pro', da, x.buf, n.scale, n.shift, n.mean, n.invstd, part, tiles,
                       bn.ggamma, bn.gbeta, acc_p, coef, relu, buf, acc, x.M, bn.C, x.grad_amax)
        elif base is not None:
            self.b('dsnt_bn_act_bwd_apply_base', da, x.buf, n.scale, n.shift, n.mean, n.invstd, coef, relu,
                   base, buf, x.M, bn.C, x.grad_amax)
        else:
            self.b_amax('dsnt_bn_act_bwd_apply', da, x.buf, n.scale, n.shift, n.mean, n.invstd, coef, relu,
                        buf, acc, x.M, bn.C, amax=x.grad_amax)

    # ------------------------------------------------------------------ convolution
    def conv(self, src, p, res1=None, res2=None, want_stats=False, need_input_grad=True, name=''):
        """y = conv(src) + bias [+ res1 + res2]; src is an Act (raw) or a Normed (BN+ReLU folded)."""
        c = convop.ConvOp(self, src, p, res1, res2, name, need_input_grad)
        c.y = y = self.act(c.x.N, c.g.Ho, c.g.Wo, p.Cout, name)
        c.x.uses += 1
        for r in (res1, res2):
            if r is not None:
                r.uses += 1
                y.gives_away = True             # dL/dy's buffer is handed to a residual input in backward
        c.forward(want_stats)
        if self.record:
            c.plan_backward()
            self.on_backward(c.backward)
        return y

    def ds_fuse_ok(self, x, p_ds, p3):
        """conv3 of a Bottleneck (p3) and its projection shortcut (p_ds, over the block input x) can run as ONE forward launch
        (csrc/fwd1.hip DS).  Asked BEFORE the block is traced: on the fused path the shortcut is not traced on its own and the
        skip tensor never exists.  The backward stays two launches (`ConvOp.backward_ds`)."""
        return convop.ds_fuse_ok(self, x, p_ds, p3)

    def conv_ds(self, src, p, x_ds, p_ds, want_stats=False, name='', name_ds='ds'):
        """y = conv(src) + bias + (conv_ds(x_ds) + bias_ds): `conv(src, p, res1=conv(x_ds, p_ds))` without the skip tensor
        (the caller has asked `ds_fuse_ok`): two ops over one output."""
        c, cd = convop.ConvOp(self, src, p, None, None, name, True), convop.ConvOp(self, x_ds, p_ds, None, None, name_ds, True)
        c.y = cd.y = y = self.act(c.x.N, c.g.Ho, c.g.Wo, p.Cout, name)
        c.x.uses += 1
        x_ds.uses += 1
        c.forward_ds(cd, want_stats)
        # (the shortcut's plan first: the order in which the two-launch path asks for the data-gradient slots)
        cd.plan_backward()
        c.plan_backward()
        y.fold_ok = False               # dL/dy feeds two convolutions: it has to exist in memory
        self.on_backward(lambda: c.backward_ds(cd))
        return y

    def _f_with_stats(self, name, y, tensors, dims):
        """Emit the element-wise forward launch `name` that writes y — as `name`_stats where the same pass also leaves what y's
        consumers need: training, the batch statistics of y (the BatchNorm that reads it next), plus the bound of its raw
        consumers if y is large enough for fp16x3; eval and large, that bound alone (no statistics in eval mode)."""
        part = None
        if self.training:
            tiles = (y.M + 127) // 128
            part = self.empty(tiles, 2, y.C)
            y.stats = (part, tiles)
        if self.use_f16x3 and y.M >= self.bf16x6_min_rows:
            y.amax_tail = BnTail()
        if part is None and y.amax_tail is None:
            self.f(name, *tensors, *dims)
        else:
            self.f(name + '_stats', *tensors, part, *dims, y.amax_tail)

    def bn_act(self, x, bn, relu=True, name=''):
        """Materialised y = relu?(bn(x)) (the stem: hourglass.py:157-159)."""
        n = self.norm(x, bn, relu)
        self.materialize(n)
        y = self.act(x.N, x.H, x.W, x.C, name)
        x.uses += 1
        # the statistics of y (the first Bottleneck's BatchNorm reads it next) and the bound of its raw consumer
        # (that Bottleneck's skip projection) ride in the same pass
        self._f_with_stats('dsnt_bn_act_fwd', y, (x.buf, n.scale, n.shift, 1 if n.relu else 0, y.buf), (x.M, x.C))
        if self.record:
            def backward():
                self._norm_backward(n, y.grad)
            self.on_backward(backward)
        return y

    def maxpool2(self, x, name=''):
        y = self.act(x.N, x.H // 2, x.W // 2, x.C, name)
        x.uses += 1
        idx = self.empty(x.N, x.H // 2, x.W // 2, x.C, dtype=torch.uint8)
        # the consumer is a BatchNorm (hourglass.py:33): its batch statistics ride in the same pass
        self._f_with_stats('dsnt_maxpool2_fwd', y, (x.buf, y.buf, idx), (x.N, x.H, x.W, x.C))
        if self.record:
            def backward():
                add, x.pending_add = x.pending_add, None
                buf, acc = self.grad_target(x, amax=True, take_add=True)
                if add is not None:
                    # a second gradient of x that arrived in a buffer of its own (the skip branch's: Hourglass._level) rides along
                    assert acc == 1
                    self.b('dsnt_maxpool2_bwd_add', y.grad, idx, buf, acc, add[0], x.N, x.H, x.W, x.C, x.grad_amax)
                else:
                    self.b_amax('dsnt_maxpool2_bwd', y.grad, idx, buf, acc, x.N, x.H, x.W, x.C, amax=x.grad_amax)
            self.on_backward(backward)
        return y

    def maxpool3s2(self, x, name=''):
        """3x3 / stride 2 / pad 1 max-pool (the torchvision ResNet stem)."""
        Ho, Wo = (x.H - 1) // 2 + 1, (x.W - 1) // 2 + 1
        y = self.act(x.N, Ho, Wo, x.C, name)
        x.uses += 1
        idx = self.empty(x.N, Ho, Wo, x.C, dtype=torch.uint8)
        self.f('dsnt_maxpool3s2_fwd', x.buf, y.buf, idx, x.N, x.H, x.W, x.C)
        if self.record:
            def backward():
                buf, acc = self.grad_target(x)
                self.b('dsnt_maxpool3s2_bwd', y.grad, idx, buf, acc, x.N, x.H, x.W, x.C)
            self.on_backward(backward)
        return y

    def bn_add_act(self, x, bn, skip, relu=True, name=''):
        """y = relu(bn(x) + skip): the tail of a torchvision residual block (conv -> bn -> += identity -> relu)."""
        n = self.norm(x, bn, relu=False)
        y = self.act(x.N, x.H, x.W, x.C, name)
        x.uses += 1
        skip.uses += 1
        if self.no_relu:
            relu = False
        self.materialize(n)
        self.f('dsnt_bn_add_act_fwd', x.buf, n.scale, n.shift, skip.buf, 1 if relu else 0, y.buf, x.M, x.C)
        if self.record:
            def backward():
                # the block input's gradient can START as dz and continue out of place (below): dz is then handed out as a `base`
                # that later launches — possibly of another lane, possibly held back — still read, so it gets a buffer of its own
                # (a shared scratch would be overwritten by the next block's backward with nothing ordering its readers first)
                share = bool(self.share_grads and skip.untouched)
                if relu:
                    # the ReLU mask (from the stored y), dz and the BatchNorm's two reductions in ONE pass
                    dz = (self.empty(x.M * x.C) if share else self.scratch('dz_tail', x.M * x.C).view(-1)[:x.M * x.C])
                    tiles = (x.M + 127) // 128
                    part = self.scratch('bnpart', tiles * 2 * bn.C).view(-1)
                    self.b('dsnt_bn_add_act_bwd_reduce', y.grad, y.buf, x.buf, n.mean, n.invstd, 1, dz, part, x.M, bn.C)
                    self._norm_backward(n, dz, reduced=(part, tiles))
                else:
                    dz = y.grad
                    self._norm_backward(n, dz)
                if share and skip.untouched:
                    # the block input's gradient starts as dz and continues out of place (the data gradient of conv1 adds it as its
                    # residual operand): no copy
                    skip.base, skip.base_amax = dz, None
                else:
                    self.grad_identity(skip, dz, donate=False)
            self.on_backward(backward)
        return y

    def upsample2_add(self, up, low, name=''):
        out = self.act(up.N, up.H, up.W, up.C, name)
        up.uses += 1
        low.uses += 1
        out.gives_away = True                   # dL/d out's buffer becomes dL/d up in backward
        self._f_with_stats('dsnt_upsample2_add_fwd', out, (up.buf, low.buf, out.buf), (up.N, up.H, up.W, up.C))
        if self.record:
            point = self.wgrads.release_point(low.M)

            def backward():
                if point:
                    self.wgrads.pass_release_point()
                buf, acc = self.grad_target(low, amax=True)
                self.b_amax('dsnt_upsample2_bwd', out.grad, buf, acc, up.N, up.H, up.W, up.C, amax=low.grad_amax)
                self.grad_identity(up, out.grad, donate=True, g_amax=out.grad_amax)
            self.on_backward(backward)
        return out

    def to_planar(self, x, C_logical, name='', out=None, gin=None):
        """NHWC activation -> logical NCHW tensor [N, C, H, W] (model surface); returns the tensor.
        In backward the incoming NCHW gradient is transposed into x.grad (first writer).
        out / gin: the caller's buffers (slices of one slab when a model has several outputs of one shape)."""
        out = self.empty(x.N, C_logical, x.H, x.W) if out is None else out
        x.uses += 1
        if gin is None:
            gin = self.empty(x.N, C_logical, x.H, x.W) if self.record else None
        self.f('dsnt_nhwc_to_nchw', x.buf, out, x.N, C_logical, x.H * x.W, x.C)
        if self.record:
            def backward():
                assert x.grad is None, 'planar output must be the first gradient writer'
                buf, _ = self.grad_target(x)
                self.b('dsnt_nchw_to_nhwc', gin, buf, x.N, C_logical, x.H * x.W, x.C)
            self.on_backward(backward)
        return out, gin

    def from_planar(self, src_nchw, Cpad, name=''):
        """Logical NCHW input [N, C, H, W] -> NHWC Act with channels zero-padded to Cpad."""
        N, Cc, H, W = src_nchw.shape
        a = self.act(N, H, W, Cpad, name)
        e = self.f('dsnt_nchw_to_nhwc', src_nchw, a.buf, N, Cc, H * W, Cpad)
        self._planar_src[id(a)] = (src_nchw, e)
        return a

    def stem_s2d(self, x, p, name='stem'):
        """The 7x7 / stride 2 / pad 3 convolution of a planar (<= 4 channel) input as a 4x4 / stride 1 / pad 1 convolution
        on its space-to-depth form (csrc/flat.hip: dsnt_s2d_input / dsnt_s2d_weights): K = 256 in 16-channel steps,
        so the stem runs on the split-precision matrix-core kernels like every other large convolution instead of the
        fp32 MFMA (245 -> ~80 us at batch 32; -0.08 ms a step).  Returns None if it does not apply (the caller then uses `conv`)."""
        got = self._planar_src.get(id(x))
        if (got is None or not self.use_f16x3 or p.R != 7 or p.S != 7 or p.stride != 2 or p.pad != 3
                or p.dil != 1 or x.C != 4 or x.H % 2 or x.W % 2 or x.N * (x.H // 2) * (x.W // 2) < self.bf16x6_min_rows):
            return None
        src, entry = got
        self.fwd.remove(entry)                      # the NHWC copy of the image is not needed
        xs = self.act(x.N, x.H // 2 + 1, x.W // 2 + 1, 16, 'input_s2d')
        xs.amax_tail = BnTail()
        self.f('dsnt_s2d_input', src, xs.buf, x.N, src.shape[1], x.H, x.W, xs.amax_tail)
        n = p.Cout * 256
        w2, gw2 = self.empty(p.Cout, 4, 4, 16), self.empty(p.Cout, 4, 4, 16)
        p2 = ConvParams(w2, p.b, gw2, p.gb, 1, 1, 1)
        p2.wq, p2.wq_stride = self.empty(3 * n, dtype=torch.bfloat16), n
        p2.wq16, p2.wb = self.empty(2 * n, dtype=torch.float16), self.empty(64)
        p2.post_reduce = ('dsnt_s2d_weights', (gw2, p.gw, p.Cout, 1))
        # the re-packed filter and its planes: one tiny launch on the MAIN lane right before the convolution (the table-driven
        # preparation of all other weights runs on the side lane beside it)
        self.f('dsnt_s2d_weights_prep', p.w, w2, p2.wq16, p2.wq, p2.wb, p.Cout)
        self.bounds.prepared_elsewhere(p2.wq16)     # (here, not by the table-driven launch)
        mark = len(self.fwd)
        y = self.conv(xs, p2, want_stats=True, need_input_grad=False, name=name)
        self.bounds.exempt(self.fwd[mark:])
        return y
