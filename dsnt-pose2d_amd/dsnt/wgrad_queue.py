"""The weight gradients of a tape's backward list between the convolution that wants one and the list: which lane runs it,
whether its launches are held back until the chain enters a launch-bound phase, the slabs waiting for their bucket's one
reduction launch and the descriptors waiting for its one grouped launch."""
import contextlib

import torch


class WgradQueue:
    def __init__(self, tape):
        self.tape = tape
        self._pending_reduce = []   # table rows of the slabs written since the last flush
        self._pending_group = []    # (descriptor bytes, workgroups) since the last flush
        self._pending_group_uses = []
        self._post_reduce = []      # (name, args) launched after the next reduction
        self._held = []             # launches collected, not yet on the list
        self._release_total, self._release_left = 0, 0
        self._lane_reads = set()    # gradient buffers a weight gradient on its own lane still reads

    # ------------------------------------------------------------------ placement
    @contextlib.contextmanager
    def placed(self, c, gy):
        """Inside the block c (a `ConvOp`: `ConvOp.wgrad`) emits its weight gradient where it belongs: (lane, DSNT_WGRAD_* share flags)."""
        t, g = self.tape, c.g
        cur = wl = t.lane
        # the weight gradient feeds nothing downstream in backward: run it on its own lane so the data-gradient chain never waits
        # for it.  DSNT_X_WGRAD_LANE_ROWS > 0: only the large convolutions of the chain's lanes whose dY nobody writes again (no
        # residual inputs: the gradient buffer is not donated onwards) — their weight gradients then fill the chip while the
        # main lane walks the launch-bound low-resolution levels
        if t.wgrad_lane is not None and (t.wgrad_lane_rows == 0 or (
                cur in t.chain_lanes and c.res1 is None and c.res2 is None and g.N * g.Ho * g.Wo >= t.wgrad_lane_rows)):
            wl = t.wgrad_lane
        # DSNT_WGRAD_SHARE_CHIP (-0.2 ms): one workgroup per CU beside the chain — except for the first convolution of the
        # network (no data gradient: it is the LAST launch of backward and has the chip to itself)
        share = 2 if (wl != cur and c.need_input_grad) else 0
        # DSNT_WGRAD_NARROW for the hourglass stacks' 3x3 weight gradients: the lane has slack there (the 1x1 weight
        # gradients left it), the stem's bucket is the tail of backward and keeps the wider plan
        if share and t.wgrad_narrow in ('1', {0: '2'}.get(c.bucket, '3')):
            share |= 4
        hold = wl != cur and self._release_left > 0
        with t.bwd.into(self._held) if hold else contextlib.nullcontext():
            t.sync_bwd(cur, wl)
            t.lane = wl
            if wl != cur:
                # gy may be donated onwards and accumulated into by a later launch of another lane: that writer waits
                # for the weight-gradient lane first (`before_write`)
                self._lane_reads.add(gy.data_ptr())
            yield wl, share
            t.lane = cur

    def before_write(self, grad):
        """A launch of the current lane is about to accumulate into `grad`."""
        if grad.data_ptr() in self._lane_reads:
            self._lane_reads.discard(grad.data_ptr())
            self.release()                                      # a held-back launch that reads it must be on the list first
            self.tape.sync_bwd(self.tape.wgrad_lane, self.tape.lane)    # a weight gradient on its own lane still reads this buffer

    def release_point(self, rows):
        """Forward: is the backward of this up-sampling (`rows` at its low resolution) a point that releases what is held?"""
        point = self.tape.wgrad_lane is not None and rows <= self.tape.release_rows
        self._release_total += point
        return point

    def begin_backward(self):
        self._release_left = self._release_total

    def pass_release_point(self):
        self._release_left -= 1
        self.release()

    def release(self):
        """Put the held-back weight-gradient launches on the backward list here."""
        if self._held:
            self.tape.bwd.extend(self._held)
            self._held = []

    # ------------------------------------------------------------------ slabs and their reduction
    def slab(self, p, nfloats, splits):
        """A slab of `splits` partial weight gradients of p, summed into p.gw / p.gb by the next flush."""
        t = self.tape
        ws = t.empty(nfloats)        # lives until the bucket's reduction
        t.bwd.workspace.add(ws.data_ptr())
        self._pending_reduce.append([ws.data_ptr(), p.gw.data_ptr(), p.gb.data_ptr() if p.gb is not None else 0,
                                     splits, p.Cout * p.R * p.S * p.Cin, p.Cout, 0])
        if p.post_reduce is not None:
            self._post_reduce.append(p.post_reduce)
        return ws

    def group(self, desc, blocks, use=None):
        """A descriptor for the next flush's grouped launch (use: its `f16_uses` record)."""
        self._pending_group.append((desc, blocks))
        if use is not None:
            self._pending_group_uses.append(use)

    @property
    def pending(self):
        return bool(self._pending_reduce)

    def flush(self, bucket=None):
        """Reduce every slab written since the last flush, on the lane `_flush_lane` picks; bucket: ... and close that parameter
        bucket (the marker carries the lane on which the bucket's gradients become complete: the replay calls the hook with that
        lane's stream current, so a collective started there orders itself after the reduction)."""
        t = self.tape
        lane, t.lane = t.lane, self._flush_lane()
        self._flush()
        if bucket is not None:
            t.bwd.mark(bucket, t.lane)
        t.lane = lane

    def _flush_lane(self):
        """The lane that reduces a bucket's weight-gradient slabs, made to wait for every lane that wrote one.  With a
        weight-gradient lane it is that lane — the main lane neither waits for the backlog of weight gradients nor
        runs the reduction; without, the main lane."""
        t = self.tape
        self.release()
        fl = t.wgrad_lane if t.wgrad_lane is not None else 0
        for src in t.chain_lanes:
            t.sync_bwd(src, fl)
        return fl

    def _flush(self):
        """Emit the one-launch reduction of every weight-gradient slab written since the last flush."""
        t, rows = self.tape, self._pending_reduce
        if not rows:
            return
        self._pending_reduce = []
        if self._pending_group:
            descs, self._pending_group = self._pending_group, []
            blob = b''.join(d for d, _ in descs)
            gtable = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(t.device)
            t._keep.append(gtable)
            blocks = (max(n for _, n in descs) + 7) // 8 * 8
            e = t.b('dsnt_conv_wgrad_group', gtable, len(descs), blocks)
            t.f16_uses.extend((e, u) for u in self._pending_group_uses)
            self._pending_group_uses = []
        blocks = max((r[4] // 4 + (r[5] + 3) // 4 + 63) // 64 for r in rows)
        t.b('dsnt_wgrad_reduce_all', t.upload(rows), len(rows), blocks)
        for nm, args in self._post_reduce:          # gradients that are reduced in another layout than the parameter's
            t.b(nm, *args)
        self._post_reduce = []
