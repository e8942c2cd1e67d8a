"""PCKh accumulation on the device (reference `src/dsnt/evaluator.py:9-87`).

Same class surface as the reference's `PCKhEvaluator` (`JOINT_NAMES`, `JOINT_GROUPS`, `meters`,
`add`, `reset`, `calculate_pckh_distance`), but `add` is one kernel over [B, J] instead of a
Python double loop with a D2H copy per step (`bin/train.py:376-377`); `add_normalized` also folds
in the back-projection to image space (`bin/train.py:243-258`, fp64 like the reference).
Meter values are accumulated as device tensors and only read when `.value()` is called.

`PCKhCurve` answers every threshold at once: one launch per batch adds into a device-resident histogram of the
normalised distance per joint (`dsnt_pckh_hist`), and PCKh at each threshold, for each joint and group,
is a cumulative sum of that table taken when the user asks.

`ErrorField` is the reference's `bin/investigate.py` on the device: where in the frame joints are missed and which way
(`dsnt_error_field`), again one launch per batch into device-resident tables.

`Reliability` asks whether a per-joint confidence knows when the joint is right: one launch per batch adds into a table of
score row against distance column (`dsnt_score_hist`), from which accuracy per score, risk against
coverage, an operating point and a monotone `ScoreCalibration` (applied on the device by `dsnt_score_lookup`) are read.

`PCKhBootstrap` asks how far a PCKh can be trusted and whether one model really beats another: one launch per batch adds
into `R + 1` copies of the curve's table, copy `r` weighting every example by a Poisson(1) draw keyed on the example's id
(`dsnt_pckh_boot`), from which standard errors, percentile intervals and a paired comparison are read.

`JointConfusion` asks what kind of miss it was: one launch per batch adds every valid joint to the cell of the joint of the
same person its prediction landed on, its own (a hit), its mirror, another or none, and counts the mirrored pairs that were
exchanged (`dsnt_joint_confusion`).  `target_mass` asks whether the heat-map was right and the read-out
wrong: the mass of each joint's map within the threshold of the truth and of the mirror joint's truth, one launch
(`dsnt_target_mass`), a per-joint score that `Reliability` tabulates against PCKh like any other.

The five table evaluators keep their joint names and their state in `_JointTables`; all of them, and `target_mass`,
prepare a batch with `_batch_args`.
"""
import ctypes

import numpy as np
import torch

from ._lib import ptr, call


def _batch_args(norm_pred, norm_target, joint_mask, head_lengths, transform_m, transform_b):
    """`(pred, target, m, b, mask, head)` as the kernels take them: f32, f32, f64, f64 `[B, 2]`, f32, f64, contiguous and
    on `norm_pred`'s device."""
    B, dev = norm_pred.shape[0], norm_pred.device
    return (norm_pred.detach().to(torch.float32).contiguous(),
            norm_target.detach().to(device=dev, dtype=torch.float32).contiguous(),
            transform_m.to(device=dev, dtype=torch.float64).contiguous(),
            transform_b.to(device=dev, dtype=torch.float64).reshape(B, 2).contiguous(),
            joint_mask.to(device=dev, dtype=torch.float32).contiguous(),
            head_lengths.to(device=dev, dtype=torch.float64).contiguous())


class _Meter:
    def __init__(self):
        self.reset()

    def reset(self):
        self.hits = None
        self.count = None

    def add_tensors(self, hits, count):
        self.hits = hits if self.hits is None else self.hits + hits
        self.count = count if self.count is None else self.count + count

    def value(self):
        if self.count is None or float(self.count) == 0:
            return float('nan'), None
        return float(self.hits) / float(self.count), None


class PCKhEvaluator:
    """Class for calculating and accumulating PCKh values."""

    JOINT_NAMES = [
        'rankle', 'rknee', 'rhip', 'lhip', 'lknee', 'lankle', 'pelvis', 'thorax',
        'upperneck', 'headtop', 'rwrist', 'relbow', 'rshoulder', 'lshoulder',
        'lelbow', 'lwrist',
    ]
    JOINT_GROUPS = {
        'ubody': {'rwrist', 'relbow', 'rshoulder', 'lshoulder', 'lelbow', 'lwrist'},
        'total_anewell': {'rankle', 'rknee', 'rhip', 'lhip', 'lknee', 'lankle',
                          'rwrist', 'relbow', 'lelbow', 'lwrist'},
        'total_mpii': set(JOINT_NAMES) - {'pelvis', 'thorax'},
        'all': set(JOINT_NAMES),
    }

    def __init__(self, threshold=0.5):
        self.threshold = threshold
        self.meters = {n: _Meter() for n in self.JOINT_NAMES + list(self.JOINT_GROUPS)}
        self._members = {g: [self.JOINT_NAMES.index(n) for n in sorted(names)]
                         for g, names in self.JOINT_GROUPS.items()}
        self._member_idx = {}      # (device, n_joints) -> {group: device index tensor}: no host upload per batch

    @staticmethod
    def calculate_pckh_distance(pred, target, ref_dist):
        return torch.dist(target, pred) / ref_dist

    def _accumulate(self, hits, valid):
        n_joints = hits.shape[1]
        hj, vj = hits.sum(0), valid.sum(0)
        for j in range(n_joints):
            name = self.JOINT_NAMES[j] if n_joints == len(self.JOINT_NAMES) else None
            if name is not None:
                self.meters[name].add_tensors(hj[j], vj[j])
        key = (hj.device, n_joints)
        groups = self._member_idx.get(key)
        if groups is None:
            groups = {g: torch.tensor([i for i in idx if i < n_joints], dtype=torch.long, device=hj.device)
                      for g, idx in self._members.items()}
            self._member_idx[key] = groups
        for g, idx in groups.items():
            self.meters[g].add_tensors(hj.index_select(0, idx).sum(), vj.index_select(0, idx).sum())

    def add_normalized(self, norm_pred, norm_target, joint_mask, head_lengths, transform_m,
                       transform_b):
        """PCKh of predictions given in normalised coords: back-projected with
        `coords @ transform_m + transform_b` (fp64) on the device, then thresholded."""
        B, J = norm_pred.shape[0], norm_pred.shape[1]
        dev = norm_pred.device
        args = _batch_args(norm_pred, norm_target, joint_mask, head_lengths, transform_m, transform_b)
        hits = torch.empty(B, J, device=dev)
        valid = torch.empty(B, J, device=dev)
        call('dsnt_pckh', *map(ptr, args), float(self.threshold), ptr(hits), ptr(valid), B, J)
        self._accumulate(hits, valid)

    def add(self, pred, target, joint_mask, head_lengths):
        """Calculate and accumulate PCKh values for batch (coords already in image space)."""
        B = pred.shape[0]
        dev = pred.device
        eye = torch.eye(2, dtype=torch.float64, device=dev).expand(B, 2, 2)
        zero = torch.zeros(B, 2, dtype=torch.float64, device=dev)
        # NaN targets of masked-out joints (tests/test_evaluator.py:27-31) are fine: the hit test
        # is gated by the mask inside the kernel
        self.add_normalized(pred, target, joint_mask, head_lengths, eye, zero)

    def reset(self):
        for m in self.meters.values():
            m.reset()


def _fp32_ascending(values, most, what):
    """`values` as the fp64 values of their fp32 roundings: between 1 and `most`, finite and strictly ascending."""
    out = [float(np.float32(v)) for v in np.asarray(values, dtype=np.float64).reshape(-1)]
    if not 1 <= len(out) <= most:
        raise ValueError('between 1 and %d %s, got %d' % (most, what, len(out)))
    if not all(np.isfinite(out)) or any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError('%s must be finite and strictly ascending as fp32 values' % what)
    return out


class _JointTables:
    """What the table evaluators share: the names of joints and groups, and the state.  The state is a tuple of host
    tensors (`_host`: merged, loaded and reduced) plus, per device that fed a batch, a tuple of tensors of the same
    shapes that the kernel adds into (`_tables`); their sum is the total.  A subclass sets `_host` when it is constructed
    and raises in `_mergeable` unless another accumulator counts the same thing."""

    JOINT_NAMES = PCKhEvaluator.JOINT_NAMES
    JOINT_GROUPS = PCKhEvaluator.JOINT_GROUPS

    def __init__(self, n_joints, joint_names, joint_groups):
        self.n_joints = int(n_joints)
        if self.n_joints < 1:
            raise ValueError('n_joints must be positive')
        if joint_names is None and self.n_joints == len(self.JOINT_NAMES):
            joint_names = self.JOINT_NAMES
            if joint_groups is None:
                joint_groups = self.JOINT_GROUPS
        self.joint_names = list(joint_names) if joint_names is not None else []
        if self.joint_names and len(self.joint_names) != self.n_joints:
            raise ValueError('%d joint names for %d joints' % (len(self.joint_names), self.n_joints))
        groups = {g: sorted(self.joint_names.index(n) for n in names) for g, names in (joint_groups or {}).items()}
        groups.setdefault('all', list(range(self.n_joints)))
        self.groups = groups
        self._tables = {}                 # device -> the tensors there, in the order the devices were first used
        self._identity = {}               # (device, B) -> (m, b) of `add`

    def _rows(self, name):
        if isinstance(name, (int, np.integer)) and not isinstance(name, bool):
            if not 0 <= name < self.n_joints:
                raise KeyError(name)
            return [int(name)]
        if name in self.groups:
            return self.groups[name]
        if name in self.joint_names:
            return [self.joint_names.index(name)]
        raise KeyError(name)

    def _names(self):
        return (self.joint_names or list(range(self.n_joints))) + list(self.groups)

    def _on(self, dev):
        """The tables on `dev`, zero when it is first used."""
        tables = self._tables.get(dev)
        if tables is None:
            tables = self._tables[dev] = tuple(torch.zeros_like(t, device=dev) for t in self._host)
        return tables

    def _identity_on(self, dev, B):
        """The identity transform `(m, b)` of a batch whose coords are already in image space."""
        ident = self._identity.get((dev, B))
        if ident is None:
            ident = self._identity[dev, B] = (torch.eye(2, dtype=torch.float64, device=dev).repeat(B, 1, 1),
                                              torch.zeros(B, 2, dtype=torch.float64, device=dev))
        return ident

    def reset(self):
        for tables in list(self._tables.values()) + [self._host]:
            for t in tables:
                t.zero_()

    def _total(self):
        """The state on the host, as fresh tensors: `_host` plus each device's tables."""
        total = tuple(t.clone() for t in self._host)
        for tables in self._tables.values():
            for t, d in zip(total, tables):
                t += d.cpu()
        return total

    def _take(self, *state):
        """Make `state` the whole state: the device tables are zeroed where they are."""
        for tables in self._tables.values():
            for t in tables:
                t.zero_()
        self._host = tuple(t.to(device='cpu', dtype=h.dtype).clone() for t, h in zip(state, self._host))

    def merge(self, other):
        """Add `other`'s total to this one's host state."""
        self._mergeable(other)
        for t, o in zip(self._host, other._total()):
            t += o

    def all_reduce(self, group=None):
        """Sum the state over the ranks of a `torch.distributed` group (evaluation sharded with
        `EpochLoader(rank=, world_size=)`); nothing to do in a single process."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        state = self._total()
        if dist.get_backend(group) == 'nccl':
            state = tuple(t.cuda() for t in state)
        for t in state:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        self._take(*state)


class _ThresholdTables(_JointTables):
    """One integer table whose last axis is the distance column of `dsnt_pckh_hist`: the thresholds, and the count."""

    MAX_THRESHOLDS = 64                   # DSNT_PCKH_HIST_MAX_T

    def _set_thresholds(self, thresholds):
        thr = _fp32_ascending(thresholds, self.MAX_THRESHOLDS, 'thresholds')
        self.thresholds = torch.tensor(thr, dtype=torch.float64)
        self.T = len(thr)
        self._thr_arg = (ctypes.c_double * self.T)(*thr)          # host array, passed by value to the kernel

    def _index(self, threshold):
        t = float(np.float32(threshold))
        hit = (self.thresholds == t).nonzero()
        if hit.numel() != 1:
            raise KeyError('PCKh@%r was not accumulated: not one of the %d thresholds' % (threshold, self.T))
        return int(hit)

    def counts(self):
        """The table, int64 on the host."""
        return self._total()[0]


class PCKhCurve(_ThresholdTables):
    """PCKh at many thresholds, and the area under that curve, from one integer table `[J, T + 1]` on the device.

    `table[j][k]` counts the valid joints `j` whose distance lies in `(thresholds[k - 1], thresholds[k]]`; column `T`
    holds those beyond the last threshold (NaN and inf among them).  Each threshold is held as the fp64 value of its
    fp32 rounding, as `dsnt_pckh` holds its one threshold, so `pckh(t)` is the very count `PCKhEvaluator(t)` gives.
    `name` below is a joint name, a group name or a joint index."""

    def __init__(self, thresholds=None, n_joints=16, joint_names=None, joint_groups=None):
        super().__init__(n_joints, joint_names, joint_groups)
        self._set_thresholds(np.arange(51) / 100 if thresholds is None else thresholds)
        self._host = (torch.zeros(self.n_joints, self.T + 1, dtype=torch.int64),)

    # ------------------------------------------------------------------ adding batches
    def add_normalized(self, norm_pred, norm_target, joint_mask, head_lengths, transform_m, transform_b,
                       return_distances=False):
        """Add a batch given in normalised coords (back-projected in fp64 as in `PCKhEvaluator.add_normalized`): one
        kernel, no reduction and no host synchronisation.  `return_distances`: the f64 [B, J] distances in head lengths,
        NaN where the mask is not 1."""
        B, J = norm_pred.shape[0], norm_pred.shape[1]
        if J != self.n_joints:
            raise ValueError('%d joints, the table has %d' % (J, self.n_joints))
        dev = norm_pred.device
        args = _batch_args(norm_pred, norm_target, joint_mask, head_lengths, transform_m, transform_b)
        dist = torch.empty(B, J, dtype=torch.float64, device=dev) if return_distances else None
        call('dsnt_pckh_hist', *map(ptr, args), self._thr_arg, self.T, ptr(self._on(dev)[0]), ptr(dist), B, J)
        return dist

    def add(self, pred, target, joint_mask, head_lengths):
        """Add a batch whose coords are already in image space."""
        self.add_normalized(pred, target, joint_mask, head_lengths, *self._identity_on(pred.device, pred.shape[0]))

    # ------------------------------------------------------------------ reading results
    def _valid(self, counts, name):
        return int(counts[self._rows(name)].sum())

    def _curve(self, counts, name):
        row = counts[self._rows(name)].sum(0)
        hits, n = row[:self.T].cumsum(0).double(), int(row.sum())
        return hits / n if n else torch.full((self.T,), float('nan'), dtype=torch.float64)

    def _auc(self, curve):
        if self.T == 1:
            raise ValueError('the area under the curve needs at least two thresholds')
        t, c = self.thresholds.numpy(), curve.numpy()
        area = (np.diff(t) * (c[1:] + c[:-1]) / 2.0).sum()
        return float(area / (t[-1] - t[0]))

    def valid(self, name='total_mpii'):
        return self._valid(self.counts(), name)

    def curve(self, name='total_mpii'):
        """PCKh at every threshold, f64 [T]; NaN where nothing was valid."""
        return self._curve(self.counts(), name)

    def pckh(self, threshold, name='total_mpii'):
        """PCKh at one of the constructed thresholds (KeyError for any other)."""
        return float(self._curve(self.counts(), name)[self._index(threshold)])

    def auc(self, name='total_mpii'):
        """Trapezoid of the curve over the thresholds, divided by their span."""
        return self._auc(self._curve(self.counts(), name))

    def summary(self, threshold=0.5):
        """PCKh of every joint and group at `threshold`, and under 'auc' the area for every group."""
        k, counts = self._index(threshold), self.counts()
        out = {name: float(self._curve(counts, name)[k]) for name in self._names()}
        if self.T > 1:
            out['auc'] = {g: self._auc(self._curve(counts, g)) for g in self.groups}
        return out

    # ------------------------------------------------------------------ combining and saving
    def _mergeable(self, other):
        if other.n_joints != self.n_joints or not torch.equal(other.thresholds, self.thresholds):
            raise ValueError('merge needs the same joints and identical thresholds')

    def state_dict(self):
        return {'thresholds': self.thresholds.clone(), 'table': self.counts()}

    def load_state_dict(self, state):
        table, thresholds = state['table'], state['thresholds']
        if table.dim() != 2 or tuple(table.shape) != (self.n_joints, thresholds.numel() + 1):
            raise ValueError('table of shape %s for %d joints and %d thresholds'
                             % (tuple(table.shape), self.n_joints, thresholds.numel()))
        self._set_thresholds(thresholds.cpu().numpy())
        self._tables = {}                 # (their width may have changed)
        self._take(table)


class PCKhBootstrap(_ThresholdTables):
    """How far a PCKh can be trusted, and whether one model beats another: a Poisson bootstrap over examples.

    `table[r][j][k]`, int64 `[R + 1, J, T + 1]`: slice 0 is `PCKhCurve`'s table, and slice `r` in 1..R counts every example
    `w(id, r)` times, `w` ~ Poisson(1) drawn by Philox from the example's id, `r` and `seed` alone (`dsnt_pckh_boot`).  The
    example (a person) is what is resampled: all its joints share the weight.  Because the weight hangs on the id, the
    table does not depend on batching, order or sharding, and two accumulators with one seed that were fed the same ids
    resampled the same people, which is what `compare` needs.  `index` is the int64 `[B]` id of each example of a batch
    (`EpochLoader`'s `sample['index']`).  `name` below is a joint name, a group name or a joint index."""

    def __init__(self, replicates=1000, thresholds=(0.5,), seed=0, n_joints=16, joint_names=None, joint_groups=None):
        self.R = int(replicates)
        if self.R < 1:
            raise ValueError('replicates must be positive')
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        super().__init__(n_joints, joint_names, joint_groups)
        self._set_thresholds(thresholds)
        self._host = (torch.zeros(self.R + 1, self.n_joints, self.T + 1, dtype=torch.int64),)

    # ------------------------------------------------------------------ adding batches
    def add_normalized(self, norm_pred, norm_target, joint_mask, head_lengths, transform_m, transform_b, index):
        """Add a batch given in normalised coords (back-projected in fp64 as in `PCKhEvaluator.add_normalized`) with the
        ids of its examples: one kernel, no reduction and no host synchronisation."""
        B, J = norm_pred.shape[0], norm_pred.shape[1]
        if J != self.n_joints:
            raise ValueError('%d joints, the table has %d' % (J, self.n_joints))
        index = torch.as_tensor(index)
        if index.is_floating_point() or index.is_complex() or index.dtype == torch.bool:
            raise ValueError('index must hold integers, got %s' % index.dtype)
        if tuple(index.shape) != (B,):
            raise ValueError('index of shape %s for %d examples' % (tuple(index.shape), B))
        dev = norm_pred.device
        args = _batch_args(norm_pred, norm_target, joint_mask, head_lengths, transform_m, transform_b)
        index = index.detach().to(device=dev, dtype=torch.int64).contiguous()
        call('dsnt_pckh_boot', *map(ptr, args), ptr(index), self._thr_arg, self.T, ctypes.c_uint64(self.seed), self.R,
             ptr(self._on(dev)[0]), B, J)

    def add(self, pred, target, joint_mask, head_lengths, index):
        """Add a batch whose coords are already in image space."""
        self.add_normalized(pred, target, joint_mask, head_lengths, *self._identity_on(pred.device, pred.shape[0]), index)

    # ------------------------------------------------------------------ reading results
    def _hits(self, counts, threshold, name):
        """(hits, valid) per slice, int64 numpy [R + 1], of the joints of `name` at one constructed threshold."""
        k = self._index(threshold)
        table = counts[:, self._rows(name)].sum(1).numpy()
        return table[:, :k + 1].sum(1), table.sum(1)

    def _replicates(self, counts, threshold, name):
        hits, n = self._hits(counts, threshold, name)
        return _ratio(hits[1:], n[1:])

    def pckh(self, threshold=0.5, name='total_mpii'):
        """The point estimate, from slice 0: `PCKhCurve.pckh` of the same feed."""
        hits, n = self._hits(self.counts(), threshold, name)
        return float(_ratio(hits[0], n[0]))

    def replicates(self, threshold=0.5, name='total_mpii'):
        """PCKh of every replicate, f64 [R]: weighted hits / weighted valid, NaN where nothing valid was drawn."""
        return self._replicates(self.counts(), threshold, name)

    def stderr(self, threshold=0.5, name='total_mpii'):
        """Sample standard deviation (ddof 1) of the finite replicates."""
        return _spread(self._replicates(self.counts(), threshold, name))

    def interval(self, threshold=0.5, name='total_mpii', level=0.95):
        """Percentile interval `(lo, hi)` of the finite replicates at `level`."""
        return _percentiles(self._replicates(self.counts(), threshold, name), level)

    def compare(self, other, threshold=0.5, name='total_mpii', level=0.95):
        """Paired comparison with `other`, an accumulator of the same seed fed the same examples (another model's
        predictions for them): a dict of `diff` (point estimate, self - other), `interval` and `stderr` of the
        per-replicate differences, and `p_greater`, the share of replicates in which self is ahead plus half the ties."""
        if (other.seed, other.R) != (self.seed, self.R):
            raise ValueError('compare needs the same seed and replicates')
        self._mergeable(other)
        mine, theirs = self.counts(), other.counts()
        # the weighted valid count of every replicate and joint agrees exactly when both saw the same examples
        if not torch.equal(mine.sum(2), theirs.sum(2)):
            raise ValueError('compare needs both accumulators fed the same examples')
        d = self._replicates(mine, threshold, name) - other._replicates(theirs, threshold, name)
        d = d[np.isfinite(d)]
        a, b = self._hits(mine, threshold, name), other._hits(theirs, threshold, name)
        return {'diff': float(_ratio(a[0][0], a[1][0]) - _ratio(b[0][0], b[1][0])), 'interval': _percentiles(d, level),
                'stderr': _spread(d),
                'p_greater': float(((d > 0).sum() + 0.5 * (d == 0).sum()) / d.size) if d.size else float('nan')}

    # ------------------------------------------------------------------ combining and saving
    def _mergeable(self, other):
        if ((other.seed, other.R, other.n_joints) != (self.seed, self.R, self.n_joints)
                or not torch.equal(other.thresholds, self.thresholds)):
            raise ValueError('merge needs the same seed, replicates, joints and identical thresholds')

    def state_dict(self):
        return {'thresholds': self.thresholds.clone(), 'seed': self.seed, 'replicates': self.R, 'table': self.counts()}

    def load_state_dict(self, state):
        table, thresholds = state['table'], state['thresholds']
        if int(state['seed']) != self.seed or int(state['replicates']) != self.R:
            raise ValueError('state of seed %d and %d replicates, this bootstrap has seed %d and %d'
                             % (state['seed'], state['replicates'], self.seed, self.R))
        if table.dim() != 3 or tuple(table.shape) != (self.R + 1, self.n_joints, thresholds.numel() + 1):
            raise ValueError('table of shape %s for %d replicates, %d joints and %d thresholds'
                             % (tuple(table.shape), self.R, self.n_joints, thresholds.numel()))
        self._set_thresholds(thresholds.cpu().numpy())
        self._tables = {}                 # (their width may have changed)
        self._take(table)


class ErrorField(_JointTables):
    """Where in the frame joints miss PCKh@`threshold`, and in which direction (reference `bin/investigate.py`).

    The normalised ground-truth location of every valid joint inside [-1, 1]^2 falls into one cell of a `bins` x `bins`
    grid (cells `[by, bx]`; `e_k <= t < e_{k+1}`, the last edge closed, as `scipy.stats.binned_statistic_dd` bins).  Per
    joint and cell the tables hold how many joints there were, how many missed (exactly the joints `PCKhEvaluator` gives
    no hit), how many of the misses had a finite offset, and the fp64 sums of those offsets (prediction - truth,
    normalised coordinates).  `name` below is a joint name, a group name or a joint index; groups sum their joints in
    ascending index.

    One owner per cell adds a batch's samples in ascending order, so tables fed by `add_normalized` alone are
    bit-identical however the set was cut into batches.  `merge` and `all_reduce` add fp64 sums on the host, in the
    order in which they are called, and `all_reduce` in the backend's order: the last bits of `mean_offset` then depend
    on that order (the counts never do)."""

    MAX_BINS = 32                         # DSNT_ERROR_FIELD_MAX_BINS

    def __init__(self, bins=8, threshold=0.5, n_joints=16, joint_names=None, joint_groups=None):
        self.bins, self.threshold = int(bins), float(threshold)
        if not 1 <= self.bins <= self.MAX_BINS:
            raise ValueError('between 1 and %d bins, got %d' % (self.MAX_BINS, self.bins))
        super().__init__(n_joints, joint_names, joint_groups)
        self.edges = np.linspace(-1, 1, self.bins + 1)
        self.centres = 0.5 * self.edges[1:] + 0.5 * self.edges[:-1]
        self._edges_arg = (ctypes.c_double * (self.bins + 1))(*self.edges)    # host array, passed by value to the kernel
        shape = (self.n_joints, self.bins, self.bins)
        self._host = (torch.zeros((3,) + shape, dtype=torch.int64), torch.zeros((2,) + shape, dtype=torch.float64))

    # ------------------------------------------------------------------ adding batches
    def add_normalized(self, norm_pred, norm_target, joint_mask, head_lengths, transform_m, transform_b):
        """Add a batch given in normalised coords (back-projected in fp64 as in `PCKhEvaluator.add_normalized` for the
        hit test; binned and subtracted as given): one kernel, no reduction and no host synchronisation."""
        B, J = norm_pred.shape[0], norm_pred.shape[1]
        if J != self.n_joints:
            raise ValueError('%d joints, the tables have %d' % (J, self.n_joints))
        args = _batch_args(norm_pred, norm_target, joint_mask, head_lengths, transform_m, transform_b)
        counts, sums = self._on(norm_pred.device)
        call('dsnt_error_field', *map(ptr, args), self.threshold, self._edges_arg, self.bins, ptr(counts), ptr(sums), B, J)

    # ------------------------------------------------------------------ reading results
    def tables(self):
        """(counts int64 [3, J, bins, bins]: total, miss, miss with a finite offset; sums f64 [2, J, bins, bins]: of dx
        and of dy) on the host."""
        return self._total()

    def _plane(self, table, name):
        """One plane [J, bins, bins] summed over the joints of `name`, in ascending index."""
        rows = self._rows(name)
        out = table[rows[0]].clone()
        for j in rows[1:]:
            out += table[j]
        return out.numpy()

    def totals(self, name='all'):
        """Valid joints whose target lay in each cell, int64 [bins, bins]."""
        return self._plane(self.tables()[0][0], name)

    def misses(self, name='all'):
        """Those of them that missed, int64 [bins, bins]."""
        return self._plane(self.tables()[0][1], name)

    def miss_rate(self, name='all'):
        """misses / totals, f64 [bins, bins]; 0 where there were no joints."""
        counts = self.tables()[0]
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.nan_to_num(self._plane(counts[1], name) / self._plane(counts[0], name))

    def mean_offset(self, name='all'):
        """Mean (dx, dy) of the misses of each cell, f64 [bins, bins, 2]; NaN where no miss had a finite offset."""
        counts, sums = self.tables()
        n = self._plane(counts[2], name)
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.stack((self._plane(sums[0], name) / n, self._plane(sums[1], name) / n), axis=-1)

    def quiver(self, name='all'):
        """`(X, Y, U, V, C)` for `ax.quiver`: cell centres, mean offsets and miss rates as flat arrays, sorted by
        ascending miss rate so that the worst cells are drawn last."""
        X, Y = np.meshgrid(self.centres, self.centres)
        C, field = self.miss_rate(name), self.mean_offset(name)
        at = np.unravel_index(np.argsort(C.flatten()), C.shape)
        return X[at], Y[at], field[..., 0][at], field[..., 1][at], C[at]

    # ------------------------------------------------------------------ combining and saving
    def _mergeable(self, other):
        if (other.n_joints, other.bins, other.threshold) != (self.n_joints, self.bins, self.threshold):
            raise ValueError('merge needs the same joints, bins and threshold')

    def state_dict(self):
        counts, sums = self.tables()
        return {'bins': self.bins, 'threshold': self.threshold, 'counts': counts, 'sums': sums}

    def load_state_dict(self, state):
        counts, sums = state['counts'], state['sums']
        shape = (self.n_joints, self.bins, self.bins)
        if int(state['bins']) != self.bins or float(state['threshold']) != self.threshold:
            raise ValueError('state of %d bins at threshold %g, this field has %d at %g'
                             % (state['bins'], state['threshold'], self.bins, self.threshold))
        if tuple(counts.shape) != (3,) + shape or tuple(sums.shape) != (2,) + shape:
            raise ValueError('tables of shape %s and %s for %d joints and %d bins'
                             % (tuple(counts.shape), tuple(sums.shape), self.n_joints, self.bins))
        self._take(counts, sums)


def _mirror_of(mirror, n_joints):
    """`mirror` as a list of `n_joints` ints, an involution of `0..n_joints-1` (`mirror[j] == j`: no partner).  None is
    the MPII left/right permutation for 16 joints and the identity otherwise."""
    if mirror is None:
        if n_joints == len(PCKhEvaluator.JOINT_NAMES):
            from .inference import HFLIP_INDICES      # (imported here: dsnt.inference imports this module)
            mirror = HFLIP_INDICES.tolist()
        else:
            mirror = range(n_joints)
    mirror = [int(v) for v in mirror]
    if len(mirror) != n_joints:
        raise ValueError('%d mirror indices for %d joints' % (len(mirror), n_joints))
    for j, v in enumerate(mirror):
        if not 0 <= v < n_joints or mirror[v] != j:
            raise ValueError('mirror is not an involution of 0..%d (mirror[%d] = %d)' % (n_joints - 1, j, v))
    return mirror


def _fp32_threshold(threshold):
    """One threshold as the fp64 value of its fp32 rounding, as `dsnt_pckh` holds it: finite and not negative."""
    t = float(np.float32(threshold))
    if not (np.isfinite(t) and t >= 0):
        raise ValueError('the threshold must be finite and not negative, got %r' % (threshold,))
    return t


class JointConfusion(_JointTables):
    """What kind of miss it was: which joint of the same person a prediction landed on (`dsnt_joint_confusion`,
    DESIGN.md §21).

    `table[j][k]`, int64 `[J, J + 1]`: every valid joint `j` adds 1 to exactly one cell of its row.  Column `j` is a hit
    within `threshold` head lengths of its own target, the very hit `PCKhEvaluator(threshold)` counts; otherwise column
    `k` is the annotated joint `k != j` of the same person whose target is nearest to the prediction among those within
    `threshold` (an exact tie goes to the smallest `k`); otherwise column `J`: it landed on no annotated joint, which is
    also where a NaN prediction ends.  `mutual[j]`, int64 `[J]`, counts the joints that landed on their `mirror` joint
    while that joint, valid itself, landed on them: the pair was exchanged, which both collapsing onto one of the two
    targets is not.  `mirror` is an involution of the joints (`mirror[j] == j`: no partner), by default
    `inference.HFLIP_INDICES` for 16 joints and the identity otherwise.  Integer tables: they do not depend on batching,
    order or sharding.  `name` below is a joint name, a group name or a joint index."""

    MAX_JOINTS = 64                       # DSNT_CONFUSION_MAX_J

    def __init__(self, threshold=0.5, n_joints=16, joint_names=None, joint_groups=None, mirror=None):
        super().__init__(n_joints, joint_names, joint_groups)
        if self.n_joints > self.MAX_JOINTS:
            raise ValueError('at most %d joints, got %d' % (self.MAX_JOINTS, self.n_joints))
        self.threshold = _fp32_threshold(threshold)
        self.mirror = _mirror_of(mirror, self.n_joints)
        self._mirror_arg = (ctypes.c_int * self.n_joints)(*self.mirror)       # host array, passed by value to the kernel
        self._host = (torch.zeros(self.n_joints, self.n_joints + 1, dtype=torch.int64),
                      torch.zeros(self.n_joints, dtype=torch.int64))

    # ------------------------------------------------------------------ adding batches
    def add_normalized(self, norm_pred, norm_target, joint_mask, head_lengths, transform_m, transform_b):
        """Add a batch given in normalised coords (back-projected in fp64 as in `PCKhEvaluator.add_normalized`): one
        kernel, no reduction and no host synchronisation."""
        B, J = norm_pred.shape[0], norm_pred.shape[1]
        if J != self.n_joints:
            raise ValueError('%d joints, the tables have %d' % (J, self.n_joints))
        args = _batch_args(norm_pred, norm_target, joint_mask, head_lengths, transform_m, transform_b)
        table, mutual = self._on(norm_pred.device)
        call('dsnt_joint_confusion', *map(ptr, args), self.threshold, self._mirror_arg, ptr(table), ptr(mutual), B, J)

    def add(self, pred, target, joint_mask, head_lengths):
        """Add a batch whose coords are already in image space."""
        self.add_normalized(pred, target, joint_mask, head_lengths, *self._identity_on(pred.device, pred.shape[0]))

    # ------------------------------------------------------------------ reading results
    def counts(self):
        """The table, int64 `[J, J + 1]` on the host."""
        return self._total()[0]

    def mutual(self):
        """The exchanges, int64 `[J]` on the host."""
        return self._total()[1]

    def _kinds(self, state, name):
        """(valid, hit, mirror, nowhere, mutual) of the joints of `name` as Python ints; every row reads its own mirror
        column."""
        table, mutual = state
        rows = self._rows(name)
        J = self.n_joints
        return (int(table[rows].sum()), sum(int(table[j, j]) for j in rows),
                sum(int(table[j, self.mirror[j]]) for j in rows if self.mirror[j] != j),
                sum(int(table[j, J]) for j in rows), sum(int(mutual[j]) for j in rows))

    def _rates(self, state, name):
        n, hit, mirror, nowhere, mutual = self._kinds(state, name)
        if not n:
            return dict.fromkeys(('hit', 'mirror', 'other', 'nowhere', 'mutual'), float('nan'))
        return {'hit': hit / n, 'mirror': mirror / n, 'other': (n - hit - mirror - nowhere) / n, 'nowhere': nowhere / n,
                'mutual': mutual / n}

    def valid(self, name='total_mpii'):
        return self._kinds(self._total(), name)[0]

    def pckh(self, name='total_mpii'):
        """hits / valid: `PCKhEvaluator(threshold)`'s figure; NaN when nothing was valid."""
        return self._rates(self._total(), name)['hit']

    def rates(self, name='total_mpii'):
        """Shares of the valid joints of `name`: `hit`, `mirror` (landed on the mirror joint), `other` (on any other
        joint), `nowhere` (on no annotated joint), which sum to 1, and `mutual` (the part of `mirror` that was an
        exchange).  NaN when nothing was valid."""
        return self._rates(self._total(), name)

    def matrix(self, normalize=False):
        """The table as numpy `[J, J + 1]`: the counts, or with `normalize` every row over its sum (f64, NaN for a row
        without a valid joint)."""
        table = self.counts().numpy()
        return _ratio(table, table.sum(1, keepdims=True)) if normalize else table

    def top(self, n=10):
        """The `n` largest confusions: `(from, onto, count, share of from's misses)` for the joint-to-joint cells off
        the diagonal that are not empty, by count descending, then by the two indices.  Joints go by name where they
        have one."""
        table = self.counts()
        J = self.n_joints
        label = self.joint_names or list(range(J))
        misses = [int(table[j].sum()) - int(table[j, j]) for j in range(J)]
        cells = [(-int(table[j, k]), j, k) for j in range(J) for k in range(J) if k != j and table[j, k] > 0]
        return [(label[j], label[k], -c, -c / misses[j]) for c, j, k in sorted(cells)[:n]]

    def summary(self):
        """`rates` of every joint and group."""
        state = self._total()
        return {name: self._rates(state, name) for name in self._names()}

    # ------------------------------------------------------------------ combining and saving
    def _mergeable(self, other):
        if (other.n_joints, other.threshold, other.mirror) != (self.n_joints, self.threshold, self.mirror):
            raise ValueError('merge needs the same joints, threshold and mirror')

    def state_dict(self):
        table, mutual = self._total()
        return {'threshold': self.threshold, 'mirror': torch.tensor(self.mirror, dtype=torch.int64), 'table': table,
                'mutual': mutual}

    def load_state_dict(self, state):
        table, mutual = state['table'], state['mutual']
        J = self.n_joints
        if float(state['threshold']) != self.threshold or [int(v) for v in state['mirror']] != self.mirror:
            raise ValueError('state of threshold %g and mirror %s, this table has %g and %s'
                             % (state['threshold'], [int(v) for v in state['mirror']], self.threshold, self.mirror))
        if tuple(table.shape) != (J, J + 1) or tuple(mutual.shape) != (J,):
            raise ValueError('tables of shape %s and %s for %d joints' % (tuple(table.shape), tuple(mutual.shape), J))
        self._take(table, mutual)


def target_mass(heatmaps, norm_target, joint_mask, head_lengths, transform_m, transform_b, threshold=0.5, mirror=None):
    """How much of each joint's heat-map lies where the truth is (`dsnt_target_mass`): f32 `[B, J, 2]` on
    the device of `heatmaps` `[B, J, h, w]`, one launch and no host synchronisation.

    `[..., 0]` is the sum of the joint's map over the pixels whose centre (`dsnt.nn.generate_xy`'s grid, back-projected
    in fp64 as a prediction is) lies within `threshold` head lengths of the joint's target, `[..., 1]` the same round the
    target of its `mirror` joint (`JointConfusion`'s `mirror`), NaN where the joint has no partner or the partner is not
    annotated.  Both are NaN where `joint_mask` is not 1.  They are sums of the values as given, so they are
    probabilities only for a normalised map (the 'dsnt' heat-maps; not raw logits or 'gauss' maps).  Summed in fp64 in a
    fixed order: bit-reproducible.

    A miss that held most of its mass at the truth is a failure of the read-out, one whose mass sits on the mirror joint
    a failure of the map.  As a score, `Reliability` tabulates it against PCKh:

        mass = target_mass(heatmaps, target, mask, head, m, b)
        rel = Reliability([0.5], thresholds=(0.5,))
        rel.add_normalized(pred, target, mask, head, m, b, mass[..., 0])
        rate, support = rel.accuracy(0.5)      # row 1: the joints with at least half their mass at the truth, of which
                                               # support[1] * (1 - rate[1]) missed all the same"""
    if heatmaps.dim() != 4:
        raise ValueError('heat-maps [B, J, h, w], got %s' % (tuple(heatmaps.shape),))
    B, J, h, w = heatmaps.shape
    if not 1 <= J <= JointConfusion.MAX_JOINTS:
        raise ValueError('between 1 and %d joints, got %d' % (JointConfusion.MAX_JOINTS, J))
    if tuple(norm_target.shape) != (B, J, 2) or tuple(joint_mask.shape) != (B, J):
        raise ValueError('targets of shape %s and a mask of shape %s for %d x %d joints'
                         % (tuple(norm_target.shape), tuple(joint_mask.shape), B, J))
    mirror, threshold = _mirror_of(mirror, J), _fp32_threshold(threshold)
    args = _batch_args(heatmaps, norm_target, joint_mask, head_lengths, transform_m, transform_b)       # the maps: f32
    out = torch.empty(B, J, 2, dtype=torch.float32, device=heatmaps.device)
    call('dsnt_target_mass', *map(ptr, args), threshold, (ctypes.c_int * J)(*mirror), ptr(out), B, J, h, w)
    return out


def _ratio(num, den):
    """num / den in fp64, NaN where den is 0."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(den > 0, np.asarray(num, np.float64) / np.asarray(den, np.float64), np.nan)


def _spread(values):
    """Sample standard deviation (ddof 1) of the finite `values`; NaN with fewer than two."""
    v = np.asarray(values, np.float64)
    v = v[np.isfinite(v)]
    return float(np.std(v, ddof=1)) if v.size > 1 else float('nan')


def _percentiles(values, level):
    """`(lo, hi)`: the `(1 - level) / 2` and `1 - (1 - level) / 2` quantiles (linear) of the finite `values`."""
    if not 0 < level < 1:
        raise ValueError('level must lie in (0, 1)')
    v = np.asarray(values, np.float64)
    v = v[np.isfinite(v)]
    if not v.size:
        return float('nan'), float('nan')
    lo, hi = np.quantile(v, [(1 - level) / 2, 1 - (1 - level) / 2], method='linear')
    return float(lo), float(hi)


def _pav(hits, n, increasing):
    """Pool-adjacent-violators over the rows with support: `hits`, `n` are Python ints per score row in ascending score.
    Returns the pooled `(hits, n)` of every supported row (None for the others), rates non-decreasing in the score if
    `increasing`, else non-increasing.  Pools are integer pairs compared by cross-multiplication: exact."""
    rows = [r for r in range(len(n)) if n[r] > 0]
    if not increasing:
        rows.reverse()                    # non-increasing in the score is non-decreasing walked from the top
    pools = []                            # [hits, n, rows]
    for r in rows:
        pools.append([hits[r], n[r], [r]])
        while len(pools) > 1 and pools[-2][0] * pools[-1][1] > pools[-1][0] * pools[-2][1]:
            h, m, members = pools.pop()
            pools[-1][0] += h
            pools[-1][1] += m
            pools[-1][2] += members
    out = [None] * len(n)
    for h, m, members in pools:
        for r in members:
            out[r] = (h, m)
    return out


class Reliability(_ThresholdTables):
    """Does a per-joint score (a confidence such as `stats['peak']`, or a spread) know when the joint is right?

    `table[j][r][k]`, int64 `[J, S + 2, T + 1]`, counts the valid joints `j` whose score lies in row `r` and whose
    distance lies in `PCKhCurve`'s column `k`.  With the `S` score edges `e`, row `r` is the number of edges `<=` the
    score: row 0 is `score < e[0]`, row `S` is `score >= e[S - 1]`, a score on an edge belongs to the row above it, and
    row `S + 1` holds the NaN scores ("unscored").  Edges and thresholds are held as the fp64 values of their fp32
    roundings, so an fp32 score compares exactly.  Summed over the score rows the table is `PCKhCurve`'s.  Everything
    read from it is computed on the host from the integers.  `name` below is a joint name, a group name or a joint
    index."""

    MAX_EDGES = 64                        # DSNT_SCORE_HIST_MAX_S

    def __init__(self, score_edges, thresholds=(0.5,), n_joints=16, higher_is_better=True, joint_names=None,
                 joint_groups=None):
        self.higher_is_better = bool(higher_is_better)
        super().__init__(n_joints, joint_names, joint_groups)
        self._set_thresholds(thresholds)
        self._set_edges(score_edges)
        self._host = (torch.zeros(self.n_joints, self.S + 2, self.T + 1, dtype=torch.int64),)

    def _set_edges(self, score_edges):
        edges = _fp32_ascending(score_edges, self.MAX_EDGES, 'score edges')
        self.score_edges = torch.tensor(edges, dtype=torch.float64)
        self.S = len(edges)
        self._edges_arg = (ctypes.c_double * self.S)(*edges)      # host array, passed by value to the kernel

    # ------------------------------------------------------------------ adding batches
    def add_normalized(self, norm_pred, norm_target, joint_mask, head_lengths, transform_m, transform_b, score):
        """Add a batch given in normalised coords (back-projected in fp64 as in `PCKhEvaluator.add_normalized`) with its
        scores, f32 `[B, J]` on the device (any view, e.g. `stats['peak']`): one kernel, no reduction and no host
        synchronisation."""
        B, J = norm_pred.shape[0], norm_pred.shape[1]
        if J != self.n_joints:
            raise ValueError('%d joints, the table has %d' % (J, self.n_joints))
        if tuple(score.shape) != (B, J):
            raise ValueError('scores of shape %s for %d x %d joints' % (tuple(score.shape), B, J))
        dev = norm_pred.device
        args = _batch_args(norm_pred, norm_target, joint_mask, head_lengths, transform_m, transform_b)
        score = score.detach().to(device=dev, dtype=torch.float32).contiguous()
        call('dsnt_score_hist', *map(ptr, args), ptr(score), self._edges_arg, self.S, self._thr_arg, self.T,
             ptr(self._on(dev)[0]), B, J)

    def add(self, pred, target, joint_mask, head_lengths, score):
        """Add a batch whose coords are already in image space."""
        self.add_normalized(pred, target, joint_mask, head_lengths, *self._identity_on(pred.device, pred.shape[0]), score)

    # ------------------------------------------------------------------ reading results
    def _hits(self, counts, threshold, name):
        """(hits, support) per score row, int64 numpy [S + 2], of the joints of `name` at one constructed threshold."""
        k = self._index(threshold)
        table = counts[self._rows(name)].sum(0).numpy()
        return table[:, :k + 1].sum(1), table.sum(1)

    def accuracy(self, threshold=0.5, name='total_mpii'):
        """`(rate f64 [S + 2], support int64 [S + 2])`: the hit rate of every score row (the last is the unscored row),
        NaN where the row is empty."""
        hits, n = self._hits(self.counts(), threshold, name)
        return _ratio(hits, n), n

    def risk_coverage(self, threshold=0.5, name='total_mpii'):
        """What is kept, and how good it is, at each of the S + 1 cuts on the score: a dict of `cut` f64, `kept` int64,
        `coverage` f64 and `pckh` f64.  With `higher_is_better` cut c keeps the joints with `score >= cut[c]`, cut =
        [-inf, e_0, ..., e_{S-1}]; otherwise those with `score < cut[c]`, cut = [e_0, ..., e_{S-1}, +inf].  `coverage` =
        kept / valid, where valid counts the unscored joints too, which no cut keeps; `pckh` is NaN where nothing is kept."""
        hits, n = self._hits(self.counts(), threshold, name)
        edges = self.score_edges.numpy()
        if self.higher_is_better:         # cut c keeps the score rows >= c
            cut = np.concatenate(([-np.inf], edges))
            kept, good = n[:-1][::-1].cumsum()[::-1], hits[:-1][::-1].cumsum()[::-1]
        else:                             # cut c keeps the score rows <= c
            cut = np.concatenate((edges, [np.inf]))
            kept, good = n[:-1].cumsum(), hits[:-1].cumsum()
        return {'cut': cut, 'kept': kept.copy(), 'coverage': _ratio(kept, np.full_like(kept, n.sum())),
                'pckh': _ratio(good, kept)}

    def operating_point(self, min_pckh, threshold=0.5, name='total_mpii'):
        """`(cut, coverage, pckh)` of the cut that keeps the most joints while their PCKh is at least `min_pckh` (the
        loosest such cut where several keep as many); None if no cut that keeps a joint reaches it."""
        rc = self.risk_coverage(threshold, name)
        order = range(self.S + 1) if self.higher_is_better else range(self.S, -1, -1)      # loosest cut first
        best = None
        for c in order:
            if rc['kept'][c] > 0 and rc['pckh'][c] >= min_pckh and (best is None or rc['kept'][c] > rc['kept'][best]):
                best = c
        return None if best is None else (float(rc['cut'][best]), float(rc['coverage'][best]), float(rc['pckh'][best]))

    def _calibrated_row(self, hits, n):
        """f32 [S + 2]: P(hit | score row), monotone over the rows with support (`_pav`); a scored row without support
        takes the value of the nearest supported row below it in score, else the nearest above; the unscored row its own
        rate.  NaN where there is nothing to go by."""
        S = self.S
        pools = _pav([int(v) for v in hits[:S + 1]], [int(v) for v in n[:S + 1]], self.higher_is_better)
        row = np.full(S + 2, np.nan, np.float32)
        above = next((p for p in pools if p is not None), None)    # for the rows below the first supported one
        below = None
        for r in range(S + 1):
            below = pools[r] if pools[r] is not None else below
            pool = below if below is not None else above
            if pool is not None:
                row[r] = np.float32(pool[0] / pool[1])
        if n[S + 1] > 0:
            row[S + 1] = np.float32(int(hits[S + 1]) / int(n[S + 1]))
        return row

    def calibration(self, threshold=0.5, name=None, score=None):
        """A `ScoreCalibration` of P(joint within `threshold` | score): with `name=None` one row of values per joint,
        otherwise one shared row from that joint or group.  `score` names the statistic this table was fed, which
        `predict(calibration=)` will apply it to (`stat_score`); by default 'peak' if `higher_is_better`, else 'spread'."""
        counts = self.counts()
        names = range(self.n_joints) if name is None else [name]
        values = np.stack([self._calibrated_row(*self._hits(counts, threshold, nm)) for nm in names])
        if score is None:
            score = 'peak' if self.higher_is_better else 'spread'
        return ScoreCalibration(self.score_edges, values, score)

    # ------------------------------------------------------------------ combining and saving
    def _mergeable(self, other):
        if (other.n_joints != self.n_joints or not torch.equal(other.thresholds, self.thresholds)
                or not torch.equal(other.score_edges, self.score_edges)):
            raise ValueError('merge needs the same joints and identical score edges and thresholds')

    def state_dict(self):
        return {'score_edges': self.score_edges.clone(), 'thresholds': self.thresholds.clone(),
                'higher_is_better': self.higher_is_better, 'table': self.counts()}

    def load_state_dict(self, state):
        table, thresholds, edges = state['table'], state['thresholds'], state['score_edges']
        if table.dim() != 3 or tuple(table.shape) != (self.n_joints, edges.numel() + 2, thresholds.numel() + 1):
            raise ValueError('table of shape %s for %d joints, %d score edges and %d thresholds'
                             % (tuple(table.shape), self.n_joints, edges.numel(), thresholds.numel()))
        self._set_thresholds(thresholds.cpu().numpy())
        self._set_edges(edges.cpu().numpy())
        self.higher_is_better = bool(state['higher_is_better'])
        self._tables = {}                 # (their shape may have changed)
        self._take(table)


class ScoreCalibration:
    """A step function of a per-joint score: `values[j][r]` for the score row `r` of `Reliability` (`values` f32
    `[J, S + 2]`, or `[1, S + 2]` shared by all joints; the last column answers a NaN score).  `score` names the statistic
    it was fitted on, for `stat_score`.  Calling it applies it on the device (`dsnt_score_lookup`): one launch, and no
    host synchronisation once `values` has been uploaded to that device."""

    MAX_EDGES = Reliability.MAX_EDGES

    def __init__(self, score_edges, values, score='peak'):
        self.load_state_dict({'score_edges': score_edges, 'values': values, 'score': score})

    def state_dict(self):
        return {'score_edges': self.score_edges.clone(), 'values': self.values.clone(), 'score': self.score}

    def load_state_dict(self, state):
        edges = _fp32_ascending(torch.as_tensor(state['score_edges']).cpu().numpy(), self.MAX_EDGES, 'score edges')
        values = torch.as_tensor(state['values']).detach().to(device='cpu', dtype=torch.float32).contiguous().clone()
        if values.dim() != 2 or values.shape[0] < 1 or values.shape[1] != len(edges) + 2:
            raise ValueError('values of shape %s for %d score edges' % (tuple(values.shape), len(edges)))
        self.score_edges = torch.tensor(edges, dtype=torch.float64)
        self.S = len(edges)
        self._edges_arg = (ctypes.c_double * self.S)(*edges)      # host array, passed by value to the kernel
        self.values = values
        self.score = str(state['score'])
        self._values = {}                 # device -> the values there

    def __call__(self, score):
        """The value of every score: f32, the shape of `score` (`[..., J]` where the values are per joint)."""
        rows = self.values.shape[0]
        if rows > 1 and (score.dim() < 1 or score.shape[-1] != rows):
            raise ValueError('scores of shape %s for values of %d joints' % (tuple(score.shape), rows))
        s = score.detach().to(torch.float32).contiguous()
        out = torch.empty_like(s)
        if s.numel():
            values = self._values.get(s.device)
            if values is None:
                values = self._values[s.device] = self.values.to(s.device)
            call('dsnt_score_lookup', ptr(s), self._edges_arg, self.S, ptr(values), int(rows > 1), ptr(out), s.numel(),
                 rows)
        return out


def stat_score(stats, name):
    """The score called `name` of a statistics dict (`inference.STATS_DOC`), f32 `[B, J]`: 'peak' (higher is better), or
    'spread' = `sqrt(trace(cov_image))` in pixels (lower is better)."""
    if name == 'peak':
        return stats['peak']
    if name == 'spread':
        cov = stats['cov_image']
        return torch.sqrt(cov[..., 0, 0] + cov[..., 1, 1]).float()
    raise KeyError('no score called %r: peak or spread' % (name,))
