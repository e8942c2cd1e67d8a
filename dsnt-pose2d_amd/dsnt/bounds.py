"""The fp16x3 operand bounds of a tape and the per-step preparation that fills them: the slot buffers of the backward and the
forward bounds, the tables of the preparation launches (weight planes, BatchNorm bounds, eval-mode BatchNorm vectors, re-packed
data-gradient weights) and the place of those launches on the forward list."""
import struct

import torch


def _f32_bits(v):
    return struct.unpack('<I', struct.pack('<f', float(v)))[0]


class Bounds:
    # launches that read weight planes or operand bounds: the preparation must have finished before the first of them
    _PREP_CONSUMERS = ('dsnt_conv_fwd_f16x3_ex', 'dsnt_conv_fwd_f16x3_stream', 'dsnt_conv1x1_fwd_f16x3', 'dsnt_conv1x1_fwd_ds_f16x3',
                       'dsnt_stem4_fwd_f16x3',
                       'dsnt_conv_fwd_bf16x6_ex', 'dsnt_conv_fwd_bf16x6')

    def __init__(self, tape):
        self.tape = tape
        self._f16_w_rows, self._f16_w_seen, self._f16_w_stream = [], set(), {}
        self._f16_bn_rows = []
        self._eval_bn_rows = []     # eval mode: every BatchNorm's vectors come from ONE table-driven launch per forward
        self._f16_dw_rows = []      # fp16x3 planes of the re-packed data-gradient weights
        # backward bounds, zeroed at the start of every backward: they follow the gradient through every writer that can report
        # one (apply, axpy, pool / upsample backward) and through donations
        self._amax_buf, self._amax_used = None, 0
        self._famax_buf, self._famax_used, self._famax_of, self._famax_bn_of = None, 0, {}, {}   # forward activations: zeroed at the start of every forward
        self._prep_exempt = set()
        # the re-packed data-gradient weights: (conv params, dst offset) of every conv whose data gradient is needed, ...
        self.dgrad_slots, self.dgrad_total = [], 0
        self.dgrad_f32, self.dgrad_planes, self.dgrad_planes16, self.dgrad_bounds = None, None, None, None
        self._dgrad_pack = None     # ... and the arguments of the one re-packing launch (`close_dgrad`, emitted by `emit_f16_prep`)

    # ------------------------------------------------------------------ registration
    def f16_weights(self, p, wq16=None, wsrc=None, wb=None, stream=False):
        """Register conv weights (default: the arena's forward layout) for the per-step fp16x3 preparation.
        stream: the planes of a 3x3 filter in the K-step order of dsnt_conv_fwd_f16x3_stream (csrc/conv3s.hip)."""
        wq16 = p.wq16 if wq16 is None else wq16
        key = wq16.data_ptr()
        if key not in self._f16_w_seen:
            self._f16_w_seen.add(key)
            wsrc = p.w if wsrc is None else wsrc
            wb = p.wb if wb is None else wb
            n = wsrc.numel()
            assert n % 4 == 0
            self._f16_w_rows.append([wsrc.data_ptr(), wq16.data_ptr(), wb.data_ptr(), n, p.wq_stride] +
                                    ([p.Cout, p.Cin] if stream else [0, 0]))
            self._f16_w_stream[key] = stream
        assert self._f16_w_stream.get(key, False) == stream, 'one weight tensor, two plane layouts'

    def prepared_elsewhere(self, wq16):
        """Planes that a launch of the caller's prepares, not the table-driven one."""
        self._f16_w_seen.add(wq16.data_ptr())

    def exempt(self, entries):
        """Forward entries that read nothing the preparation writes, whatever their names say: the main lane does not wait for them."""
        self._prep_exempt.update(id(e) for e in entries)

    def f16_bn_bound(self, n):
        """Device scalar >= |relu?(bn(x))| of the train-mode BatchNorm seen through Normed n."""
        if n.abound is None:
            n.abound = self.tape.empty(64)            # a bound = 64 slots (DSNT_BOUND_SLOTS)
            self._f16_bn_rows.append([n.bn.gamma.data_ptr(), n.bn.beta.data_ptr(), n.abound.data_ptr(), n.bn.C,
                                      _f32_bits(float(n.x.M) ** 0.5)])
        return n.abound

    @staticmethod
    def f16_bn_bound_bwd(n):
        """The same bound for a backward consumer.  The forward list computes it every step (emit_f16_prep) only if
        some forward conv asked for it before the list was closed; rows added later would be lost."""
        assert n.abound is not None, 'fp16x3 backward needs the BN bound its forward conv registered'
        return n.abound

    def eval_bn(self, n):
        """Eval mode: the vectors of Normed n come from its BatchNorm's running statistics."""
        bn = n.bn
        self._eval_bn_rows.append([bn.gamma.data_ptr(), bn.beta.data_ptr(), bn.rmean.data_ptr(), bn.rvar.data_ptr(),
                                   n.mean.data_ptr(), n.invstd.data_ptr(), n.scale.data_ptr(), n.shift.data_ptr(),
                                   bn.C, _f32_bits(bn.eps)])

    def amax_slot(self):
        if self._amax_buf is None:
            self._amax_buf = self.tape.empty(64 * 4096)
        assert self._amax_used + 64 <= self._amax_buf.numel(), 'backward bound slots exhausted'
        self._amax_used += 64
        return self._amax_buf[self._amax_used - 64:self._amax_used]

    def _famax_slot(self):
        if self._famax_buf is None:
            self._famax_buf = self.tape.empty(64 * 2048)      # hg8 with every level on fp16x3 claims ~800 slots
        assert self._famax_used + 64 <= self._famax_buf.numel(), 'forward bound slots exhausted'
        self._famax_used += 64
        return self._famax_buf[self._famax_used - 64:self._famax_used]

    def claimed(self):
        """(backward, forward) bound slots claimed so far, None where none was: what a test reads after a step."""
        return tuple(buf[:used] if buf is not None else None
                     for buf, used in ((self._amax_buf, self._amax_used), (self._famax_buf, self._famax_used)))

    def operand_amax(self, x):
        """Bound slot for activation x used as a RAW fp16x3 operand (no BatchNorm in between: skip projections, `lin`
        convolutions): the launch that produced x is asked — through its dsnt_out_bounds, read at launch time — to leave
        max|x| there (-0.24 ms against bf16x6 for those convolutions).  None if the producer cannot."""
        t = x.amax_tail
        if t is None or not self.tape.use_f16x3:
            return None
        slot = self._famax_of.get(id(t))
        if slot is None:
            slot = self._famax_slot()
            t.amax = slot.data_ptr()
            self._famax_of[id(t)] = slot
            self.tape._keep.append(t)
        return slot

    def operand_amax_bn(self, n):
        """Eval mode: bound slot for relu?(bn(x)) as an fp16x3 operand.  The BatchNorm vectors come from running
        statistics (one dsnt_bn_eval_prep launch at the head of the forward), so the launch that produces x can form
        the operand itself and leave its exact maximum (dsnt_out_bounds.amax_bn).  One BatchNorm per producer; None if
        the producer cannot or is already taken by another BatchNorm."""
        t = n.x.amax_tail
        if t is None or not self.tape.use_f16x3 or self.tape.training:
            return None
        got = self._famax_bn_of.get(id(t))
        if got is not None:
            return got[1] if got[0] is n else None
        slot = self._famax_slot()
        t.amax_bn, t.amax_scale, t.amax_shift = slot.data_ptr(), n.scale.data_ptr(), n.shift.data_ptr()
        t.amax_relu = 1 if n.relu else 0
        self._famax_bn_of[id(t)] = (n, slot)
        self.tape._keep.append(t)
        return slot

    # ------------------------------------------------------------------ re-packed data-gradient weights
    def dgrad_slot(self, p):
        """(offset, index) of p's weights among the re-packed data-gradient weights."""
        slot = self.dgrad_total, len(self.dgrad_slots)
        self.dgrad_slots.append((p, slot[0]))
        self.dgrad_total += (p.w.numel() + 7) // 8 * 8
        return slot

    def dgrad_f16(self, slot, slot_k, nw, order=(0, 0)):
        """(fp32 weights, fp16 planes, bound) of a slot, its planes registered with the preparation; order: (K, N) of the stream
        layout."""
        wd, wq16 = self.dgrad_f32[slot:slot + nw], self.dgrad_planes16[slot:slot + nw]
        wbd = self.dgrad_bounds[64 * slot_k:64 * slot_k + 64]
        self._f16_dw_rows.append([wd.data_ptr(), wq16.data_ptr(), wbd.data_ptr(), nw, self.dgrad_total, *order])
        return wd, wq16, wbd

    def close_dgrad(self):
        """Every slot is known: one launch re-packs (tap-flipped, transposed) and bf16-splits every dgrad weight."""
        if not self.dgrad_slots:
            return
        t = self.tape
        total = (self.dgrad_total + 7) // 8 * 8
        self.dgrad_f32 = t.empty(total)
        self.dgrad_planes = t.empty(3 * total, dtype=torch.bfloat16)
        rows = [[(p.w.data_ptr() - t.param_arena.data_ptr()) // 4, dst, p.Cout, p.R, p.S, p.Cin] for p, dst in self.dgrad_slots]
        # launched by the forward list's preparation (emit_f16_prep), off the backward's critical path
        self._dgrad_pack = (t.upload(rows, torch.int32), len(rows), t.param_arena, self.dgrad_f32, self.dgrad_planes, total)
        self.dgrad_total = total
        if t.use_f16x3:
            self.dgrad_planes16 = t.empty(2 * total, dtype=torch.float16)
            self.dgrad_bounds = t.empty(64 * len(rows))

    # ------------------------------------------------------------------ emission
    def emit_backward_zero(self, pos):
        """fp16x3: zero the backward slots at position `pos` of the backward list."""
        if self._amax_used:
            t = self.tape
            t.b('dsnt_fill_zero', self._amax_buf, self._amax_used)
            t.bwd.insert(pos, t.bwd.pop())

    def emit_f16_prep(self, pos, head=()):
        """Insert the per-step preparation launches at position `pos` of the forward list: fp16x3 weight planes and BN
        operand bounds, eval-mode BN vectors and — weights do not change between a forward and its backward — the
        re-packed / split data-gradient weights.  `head` = entries already on the list at `pos` that belong to the
        preparation (the bf16 split of the arena).  With lanes, all of it runs on the side lane beside the stem
        convolution (which reads fp32 weights) and the main lane waits right before the first launch that needs it."""
        t = self.tape
        fwd = t.fwd
        # (eval mode: the BN vectors are needed at once, and there is nothing to hide the launches behind)
        side = 1 if (t.use_lanes and t.training) else 0      # (beside the stem: -0.15 ms)
        saved_lane, t.lane = t.lane, side
        prep = [(fn, args, name, side) for fn, args, name, _ in head]
        with fwd.into(prep):
            for name, rows, more in (('dsnt_f16_prep_weights', self._f16_w_rows, (7,)), ('dsnt_f16_prep_bn_bounds', self._f16_bn_rows, ()),
                                     ('dsnt_bn_eval_prep', self._eval_bn_rows, ())):
                if rows:
                    t.f(name, t.upload(rows), len(rows), *more)
            fwd_half = len(prep)                # everything from here on is read by the backward list only
            if self._dgrad_pack is not None:
                t.f('dsnt_conv_pack_dgrad_all', *self._dgrad_pack)
            if self._f16_dw_rows:
                t.f('dsnt_f16_prep_weights', t.upload(self._f16_dw_rows), len(self._f16_dw_rows), 7)
            if self._famax_used:
                t.lane = 0
                t.f('dsnt_fill_zero', self._famax_buf, self._famax_used)
                prep.insert(0, prep.pop())      # main lane, first: every producer comes after it
                fwd_half += 1                   # (the boundary index moves with it)
        t.lane = saved_lane
        relay = None
        if side and t.prep_split and t.n_lanes > 3 and 0 < fwd_half < len(prep):
            # the backward-only half keeps running on the side lane while the forward proceeds: an idle lane takes the dependency
            # on the FIRST half here (a list entry records and waits at one position), the main lane waits for that lane below
            relay = t.n_lanes - 1
            prep.insert(fwd_half, fwd.sync_entry(side, relay))
        fwd[pos:pos + len(head)] = prep
        if side and prep:
            first = next((i for i in range(pos + len(prep), len(fwd))
                          if fwd[i][0] is not None and fwd[i][2] in self._PREP_CONSUMERS
                          and id(fwd[i]) not in self._prep_exempt), len(fwd))
            if relay is not None:
                # the relay lane is taken to be idle up to here: an op (or a wait) traced onto it before `first` would put the main
                # lane behind that op without anyone noticing — refuse at trace time instead
                for ent in fwd[pos + len(prep):first]:
                    busy = ent[3] == relay if ent[0] is not None else (ent[2] == 'sync' and relay in ent[1][:2])
                    assert not busy, 'prep relay lane %d is in use before the first prep consumer (%s)' % (relay, ent[2])
            fwd.insert(first, fwd.sync_entry(side if relay is None else relay, 0))
