"""Input-image contract of the pose models and the training-sample transform (reference `src/dsnt/data.py`).

`ImageSpecs` (`data.py:19-78`) is what the models expose (`model.image_specs`).  `convert` pools a float image to
`size` and normalises it (one HIP launch); `unconvert` undoes the normalisation and returns a PIL image.

`DeviceAugment` is `MPIIDataset.__getitem__` (`data.py:118-226`) for a whole batch on the GPU: from the
`R x R` uint8 crops the MPII loader returns (already on the device) to the model's input, the transformed
keypoints, their mask and the back-projection, in two launches on the current stream with no host round trip.
Reading the MPII files and parsing its annotations stay out of scope: the boundary is "source crops already
on the device".  The exact transform (Pillow's rotation, torchvision 0.2.0's centre crop) is documented in
`csrc/augment.hip`.

`DeviceDataset` keeps a whole training set of crops resident on the device, and `EpochLoader` runs shuffled epochs
over it: the order (a counter-based permutation), the gather and the transform are all device launches, so an epoch
needs no host work (the reference's `DataLoader(train_data, batch_size, shuffle=True, num_workers=4)`).

`ImagePool` keeps full decoded images on the device and crops person boxes from them (`dsnt_crop_affine`, Pillow's
affine bilinear sampler bit for bit); `box_matrix` builds the box matrices, and `DeviceDataset.from_pool` builds a
training set from the crops.

`ExampleScores` keeps, per dataset row, how badly the row was predicted the last time it was seen (one launch per batch,
`dsnt_example_scores`), and `WeightedLoader` runs epochs that draw rows with replacement in proportion to arbitrary
weights, those of `ExampleScores.weights_from_table` for one: an exact fixed-point CDF built on the device once per
re-weighting (`dsnt_sample_cdf`) and one counter-based draw per batch (`dsnt_sample_indices`) in front of the same gather
kernels (`csrc/sampler.hip`).

`Occlude` hides parts of a finished batch: per sample up to `max_rects` rectangles, placed uniformly or on a visible
joint, filled with a constant, with noise or with the same pixels of another sample of the batch, in one launch keyed by
(seed, step, sample) like the augmentation (`dsnt_occlude`, `csrc/occlude.hip`).  Both loaders take
one as `occlude=`.
"""
import math

import numpy as np
import torch

from . import _lib
from .evaluator import _batch_args
from .inference import HFLIP_INDICES


def _stats(specs, dataset_stats):
    mean = dataset_stats.MEAN if specs.subtract_mean else [0, 0, 0]
    std = dataset_stats.STDDEV if specs.divide_stddev else [1, 1, 1]
    return mean, std


class ImageSpecs:
    def __init__(self, size, subtract_mean, divide_stddev):
        self._size = size
        self._subtract_mean = subtract_mean
        self._divide_stddev = divide_stddev

    @property
    def size(self):
        return self._size

    @property
    def subtract_mean(self):
        return self._subtract_mean

    @property
    def divide_stddev(self):
        return self._divide_stddev

    def convert(self, img, dataset_stats):
        """`adaptive_avg_pool2d(img, size)` then `Normalize(MEAN, STDDEV)` (each only if the spec asks for it) on a
        float32 device tensor `[3, H, W]` or `[N, 3, H, W]` with values in [0, 1].  `dataset_stats` has `MEAN` and
        `STDDEV` (per channel).  Returns a new tensor `[.., 3, size, size]`."""
        _lib.f32(img)
        if img.dim() not in (3, 4) or img.shape[-3] != 3:
            raise RuntimeError('dsnt: convert expects [3, H, W] or [N, 3, H, W], got %s' % (tuple(img.shape),))
        x = img if img.dim() == 4 else img.unsqueeze(0)
        mean, std = _stats(self, dataset_stats)
        m = torch.tensor(mean, dtype=torch.float32).to(img.device, non_blocking=True)
        s = torch.tensor(std, dtype=torch.float32).to(img.device, non_blocking=True)
        N, C, H, W = x.shape
        out = torch.empty(N, C, self.size, self.size, device=img.device, dtype=torch.float32)
        _lib.call('dsnt_pool_normalize', _lib.ptr(x), N, C, H, W, self.size, _lib.ptr(m), _lib.ptr(s), _lib.ptr(out))
        return out if img.dim() == 4 else out[0]

    def unconvert(self, img_tensor, dataset_stats):
        """A `[3, H, W]` tensor with the specs' normalisation undone, as a PIL RGB image (the reference's
        `ToPILImage`: x * 255 truncated to uint8).  For looking at samples; it copies to the host."""
        from PIL import Image
        mean, std = _stats(self, dataset_stats)
        x = img_tensor.detach().to('cpu', torch.float32).clone()
        for t, m, s in zip(x, mean, std):
            t.mul_(s).add_(m)
        return Image.fromarray(x.mul(255).byte().permute(1, 2, 0).numpy(), 'RGB')


def _check(name, t, dtype, shape):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError('dsnt: %s must be a tensor' % name)
    if t.dtype != dtype:
        raise RuntimeError('dsnt: %s must be %s, got %s' % (name, dtype, t.dtype))
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError('dsnt: %s must have shape %s, got %s' % (name, tuple(shape), tuple(t.shape)))
    _lib.ptr(t)          # refuses CPU and non-contiguous tensors
    return t


class DeviceAugment:
    """The MPII training-sample transform (reference `MPIIDataset.__getitem__`, `data.py:118-226`) for a batch.

    `DeviceAugment(image_specs, mean, std, use_aug=True, train=True, seed=0)`; `mean` / `std` are the dataset's
    per-channel statistics (used as `image_specs` says, like `convert`).  Call it as

        sample = aug(src_u8, keypoints, keypoint_mask, matrix, head_lengths, step, params=None)

    with device tensors `src_u8` uint8 `[B, R, R, 3]` (the crops `load_cropped_image(id, size=R, margin=R/4)`
    returns), `keypoints` float64 `[B, J, 2]` (original-image pixels), `keypoint_mask` `[B, J]`, `matrix` float64
    `[B, 3, 3]` (the bounding-box transform) and `head_lengths` `[B]`.  It returns the reference's sample dict,
    batched: `input` f32 `[B, 3, S, S]` (S = image_specs.size), `part_coords` f32 `[B, J, 2]`, `part_mask` f32
    `[B, J]`, `transform_m` f64 `[B, 2, 2]`, `transform_b` f64 `[B, 1, 2]`, `hflip` bool `[B]`, `normalize` f64
    `[B]`, and `params`: the per-sample `scale` f32, `rot` f32 (degrees), `hflip` uint8 and `gain` f32 `[B, 3]`.

    Parameters: with `use_aug`, drawn on the device by a counter-based generator keyed by (seed, step, sample), so
    the same (seed, step) gives the same batch and nothing is carried between calls; `params` (a dict with those four
    tensors on the device) overrides the draw.  Without `use_aug`: the identity (scale 1, no rotation, no flip,
    gain 1).  `train` masks joints that leave the crop (`|coord| >= 1`), as the reference does for the train subset.
    Values of given `params` are not checked on the host (that would synchronise): the kernel clamps the crop side
    `int(R * scale)` into `[1, 8R]` (1 below the range or at NaN, 8R above it).
    Everything is enqueued on the current stream; nothing synchronises with the host.

    `flip_pair=True` (flip test-time augmentation, `inference.predict(..., paired=True)`): the same launch also
    writes every pixel mirrored into a second half, and the dict gains `input_pair` f32 `[2B, 3, S, S]` whose rows
    `B..2B-1` are exactly `input.flip(-1)`; `input` is then a view of its first half, with the same values.
    """

    def __init__(self, image_specs, mean, std, use_aug=True, train=True, seed=0):
        self.image_specs = image_specs
        self.mean = [float(v) for v in (mean if image_specs.subtract_mean else (0, 0, 0))]
        self.std = [float(v) for v in (std if image_specs.divide_stddev else (1, 1, 1))]
        self.use_aug = use_aug
        self.train = train
        self.seed = int(seed)
        self._dev = {}        # device -> (mean, std, flip table) on that device

    def _consts(self, device):
        c = self._dev.get(device)
        if c is None:
            c = (torch.tensor(self.mean, dtype=torch.float32, device=device),
                 torch.tensor(self.std, dtype=torch.float32, device=device),
                 HFLIP_INDICES.to(device))
            self._dev[device] = c
        return c

    def __call__(self, src_u8, keypoints, keypoint_mask, matrix, head_lengths, step, params=None, flip_pair=False):
        if not isinstance(src_u8, torch.Tensor) or src_u8.dim() != 4 or src_u8.shape[1] != src_u8.shape[2] \
                or src_u8.shape[3] != 3:
            raise RuntimeError('dsnt: src_u8 must be [B, R, R, 3] (HWC crops), got %s'
                               % (tuple(src_u8.shape) if isinstance(src_u8, torch.Tensor) else type(src_u8),))
        B, R = src_u8.shape[0], src_u8.shape[1]
        _check('src_u8', src_u8, torch.uint8, (B, R, R, 3))
        dev = src_u8.device
        J = keypoints.shape[1] if isinstance(keypoints, torch.Tensor) and keypoints.dim() == 3 else -1
        _check('keypoints', keypoints, torch.float64, (B, J, 2))
        _check('matrix', matrix, torch.float64, (B, 3, 3))
        if not isinstance(keypoint_mask, torch.Tensor) or tuple(keypoint_mask.shape) != (B, J):
            raise RuntimeError('dsnt: keypoint_mask must be a [B, J] tensor')
        kmask = _check('keypoint_mask', keypoint_mask.to(torch.float32), torch.float32, (B, J))
        if not isinstance(head_lengths, torch.Tensor) or tuple(head_lengths.shape) != (B,):
            raise RuntimeError('dsnt: head_lengths must be a [B] tensor')
        normalize = _check('head_lengths', head_lengths.to(torch.float64), torch.float64, (B,))
        if src_u8.device != keypoints.device or keypoints.device != matrix.device or matrix.device != kmask.device:
            raise RuntimeError('dsnt: DeviceAugment inputs must be on one device')
        draw = 0
        if params is not None:
            scale = _check('params.scale', params['scale'], torch.float32, (B,)).clone()
            rot = _check('params.rot', params['rot'], torch.float32, (B,)).clone()
            hflip = _check('params.hflip', params['hflip'], torch.uint8, (B,)).clone()
            gain = _check('params.gain', params['gain'], torch.float32, (B, 3)).clone()
        elif self.use_aug:
            draw = 1
            scale = torch.empty(B, dtype=torch.float32, device=dev)
            rot = torch.empty(B, dtype=torch.float32, device=dev)
            hflip = torch.empty(B, dtype=torch.uint8, device=dev)
            gain = torch.empty(B, 3, dtype=torch.float32, device=dev)
        else:
            scale = torch.ones(B, dtype=torch.float32, device=dev)
            rot = torch.zeros(B, dtype=torch.float32, device=dev)
            hflip = torch.zeros(B, dtype=torch.uint8, device=dev)
            gain = torch.ones(B, 3, dtype=torch.float32, device=dev)
        sample = self._launch(src_u8, keypoints, kmask, matrix, B, step, (draw, scale, rot, hflip, gain), flip_pair,
                              params is not None)
        sample['normalize'] = normalize
        sample['hflip'] = hflip.bool()
        return sample

    def _flip_table(self, J, flips, dev):
        """The joint permutation of a flip; `flips`: some sample may be flipped (drawn or given parameters)."""
        flip = self._consts(dev)[2]
        if J == flip.numel():
            return flip
        if flips:
            raise RuntimeError('dsnt: with flips the keypoints need the %d MPII joints (inference.HFLIP_INDICES), got %d'
                               % (flip.numel(), J))
        key = (dev, J)
        if key not in self._dev:
            self._dev[key] = torch.arange(J, device=dev)       # never applied: no sample is flipped
        return self._dev[key]

    def _launch(self, crops, keypoints, kmask, matrix, B, step, p, flip_pair, given, gather=None):
        """The image and keypoint launches of one batch, shared by `__call__` and `EpochLoader`.  `p` = (draw, scale, rot,
        hflip, gain); `given`: the parameters were passed in.  `gather` = (idx, head_lengths, draw_offset): sample b is
        row idx[b] of the pools `crops`, `keypoints`, `kmask`, `matrix`, `head_lengths`, and `normalize` is written
        too.  Returns the sample dict; the caller fills in `hflip` (and, batched, `normalize`)."""
        dev = crops.device
        R, J, S = crops.shape[1], keypoints.shape[1], self.image_specs.size
        draw, scale, rot, hflip, gain = p
        mean, std, _ = self._consts(dev)
        flip = self._flip_table(J, draw or given, dev)
        pair = torch.empty(2 * B if flip_pair else B, 3, S, S, dtype=torch.float32, device=dev)
        name = 'dsnt_augment_fwd_pair' if flip_pair else 'dsnt_augment_fwd'
        drawn = (B, R, S, _lib.ptr(scale), _lib.ptr(rot), _lib.ptr(hflip), _lib.ptr(gain), draw,
                 self.seed & (2 ** 64 - 1), int(step) & (2 ** 64 - 1))
        if gather is None:
            _lib.call(name, _lib.ptr(crops), *drawn, _lib.ptr(mean), _lib.ptr(std), _lib.ptr(pair))
        else:
            idx, head_lengths, draw_offset = gather
            N = crops.shape[0]
            _lib.call(name + '_gather', _lib.ptr(crops), N, _lib.ptr(idx), *drawn, draw_offset, _lib.ptr(mean),
                      _lib.ptr(std), _lib.ptr(pair))
        pc = torch.empty(B, J, 2, dtype=torch.float32, device=dev)
        pm = torch.empty(B, J, dtype=torch.float32, device=dev)
        tm = torch.empty(B, 2, 2, dtype=torch.float64, device=dev)
        tb = torch.empty(B, 1, 2, dtype=torch.float64, device=dev)
        kp_args = (_lib.ptr(scale), _lib.ptr(rot), _lib.ptr(hflip), _lib.ptr(flip), 1 if self.train else 0,
                   _lib.ptr(pc), _lib.ptr(pm), _lib.ptr(tm), _lib.ptr(tb))
        normalize = None
        if gather is None:
            _lib.call('dsnt_augment_keypoints', _lib.ptr(matrix), _lib.ptr(keypoints), _lib.ptr(kmask), B, J, *kp_args)
        else:
            normalize = torch.empty(B, dtype=torch.float64, device=dev)
            _lib.call('dsnt_augment_keypoints_gather', _lib.ptr(matrix), _lib.ptr(keypoints), _lib.ptr(kmask),
                      _lib.ptr(head_lengths), N, _lib.ptr(idx), B, J, *kp_args, _lib.ptr(normalize))
        sample = {'normalize': normalize, 'transform_b': tb, 'transform_m': tm, 'input': pair[:B], 'part_mask': pm,
                  'part_coords': pc, 'hflip': None, 'params': {'scale': scale, 'rot': rot, 'hflip': hflip, 'gain': gain}}
        if flip_pair:
            sample['input_pair'] = pair
        return sample


_OCC_FILLS = {'value': 0, 'noise': 1, 'paste': 2}       # DSNT_OCCLUDE_FILL_*
_OCC_CENTRES = {'uniform': 0, 'joint': 1}                # DSNT_OCCLUDE_CENTRE_*
_OCC_MAX_RECTS = 8                                       # DSNT_OCCLUDE_MAX_RECTS
_OCC_MAX_JOINTS = 256                                    # DSNT_OCCLUDE_MAX_JOINTS


def _triple(name, v):
    v = [float(x) for x in v]
    if len(v) != 3:
        raise RuntimeError('dsnt: %s needs one value per channel, got %d' % (name, len(v)))
    return v


class Occlude:
    """Synthetic occlusion of a batch that `DeviceAugment` or a loader made: rectangles of the input are replaced.

    `Occlude(p=0.5, max_rects=2, side=(0.1, 0.4), fill='value', centre='uniform', fill_value=(0, 0, 0), mean=(0, 0, 0),
    std=(1, 1, 1), mask_covered=False, seed=0)`; `Occlude.like(augment, **kw)` takes the resolved `mean` / `std` and the
    seed of a `DeviceAugment`.  A sample is occluded with probability `p` and then gets 1..`max_rects` (at most 8)
    rectangles whose sides are drawn independently from `side`, a range of fractions of the input's side S turned into
    pixels as `max(1, round(f * S))`; a rectangle is centred on a uniformly drawn pixel (`centre='uniform'`) or on the
    pixel of a joint with a non-zero `part_mask` that lies in the image (`'joint'`; with no such joint, uniformly) and
    clipped to the image.  `fill`: `'value'`, channel c becomes `fill_value[c]` (a value of the normalised input: 0 is the
    dataset mean where the specs subtract it); `'noise'`, uniform noise in (0, 1] normalised with `mean` / `std` as the
    augmentation normalises pixels; `'paste'`, the same pixels of another sample of the batch (the identity in a batch
    of one).

        out = occ(sample, step, draw_offset=0, rects=None, donor=None)

    returns a shallow copy of the sample dict in which `input` is a new, occluded tensor, `occluded` uint8 `[B, J]` says
    which joints' pixels were covered (whatever their mask; a joint outside the image is never covered), and `params`
    (a copy) gains `occ_rects` int32 `[B, max_rects, 4]`, rows `(x0, y0, x1, y1)` half-open and zero where unused, and
    `occ_donor` int32 `[B]`.  Covered joints stay supervised unless `mask_covered=True`, which replaces `part_mask` by
    `part_mask * (1 - occluded)`.  The sample passed in and its tensors are not modified.  The draw is counter-based,
    keyed by (`seed`, `step`, `draw_offset` + sample) with no state between calls, in Philox domains of its own: the same
    key gives the same bits, and a loader's rank r passes r * B as it does to the augmentation.  Given `rects` (int32
    `[B, max_rects, 4]` on the device) nothing is drawn; `donor` (int32 `[B]`) then defaults to the next sample,
    `(b + 1) % B`.  Their values are not checked on the host (that would synchronise): the kernel clamps every coordinate
    into `[0, S]` and every donor into `[0, B)`, and a rectangle with `x1 <= x0` or `y1 <= y0` is empty.  A sample with
    `input_pair` is refused: flip evaluation is not training.  One launch on the current stream; nothing synchronises.
    """

    def __init__(self, p=0.5, max_rects=2, side=(0.1, 0.4), fill='value', centre='uniform', fill_value=(0, 0, 0),
                 mean=(0, 0, 0), std=(1, 1, 1), mask_covered=False, seed=0):
        p, K = float(p), int(max_rects)
        if not 0.0 <= p <= 1.0:
            raise RuntimeError('dsnt: Occlude needs 0 <= p <= 1, got %r' % (p,))
        if not 1 <= K <= _OCC_MAX_RECTS:
            raise RuntimeError('dsnt: max_rects must lie in [1, %d], got %d' % (_OCC_MAX_RECTS, K))
        lo, hi = (float(v) for v in side)
        if not 0.0 < lo <= hi <= 1.0:
            raise RuntimeError('dsnt: side must be fractions 0 < min <= max <= 1 of the input, got %r' % (tuple(side),))
        if fill not in _OCC_FILLS:
            raise RuntimeError("dsnt: fill must be 'value', 'noise' or 'paste', got %r" % (fill,))
        if centre not in _OCC_CENTRES:
            raise RuntimeError("dsnt: centre must be 'uniform' or 'joint', got %r" % (centre,))
        self.p, self.max_rects, self.side, self.fill, self.centre = p, K, (lo, hi), fill, centre
        self.fill_value, self.mean, self.std = _triple('fill_value', fill_value), _triple('mean', mean), _triple('std', std)
        self.mask_covered, self.seed = bool(mask_covered), int(seed)
        self._dev = {}        # device -> (fill_value, mean, std) on that device

    @classmethod
    def like(cls, augment, **kw):
        """An `Occlude` with the resolved `mean` / `std` and the seed of `augment`, a `DeviceAugment`."""
        if not isinstance(augment, DeviceAugment):
            raise RuntimeError('dsnt: Occlude.like needs a DeviceAugment, got %s' % type(augment))
        return cls(**dict(dict(mean=augment.mean, std=augment.std, seed=augment.seed), **kw))

    def sides(self, S):
        """`side` in pixels of an S x S input: `(side_min, side_max)`."""
        lo, hi = (min(int(S), max(1, int(round(f * S)))) for f in self.side)
        return lo, hi

    def _consts(self, device):
        c = self._dev.get(device)
        if c is None:
            c = self._dev[device] = tuple(torch.tensor(v, dtype=torch.float32, device=device)
                                          for v in (self.fill_value, self.mean, self.std))
        return c

    def __call__(self, sample, step, draw_offset=0, rects=None, donor=None):
        if not isinstance(sample, dict) or 'input' not in sample:
            raise RuntimeError('dsnt: Occlude takes the sample dict of DeviceAugment or a loader')
        if 'input_pair' in sample:
            raise RuntimeError('dsnt: Occlude refuses a flip_pair sample (input_pair): flip evaluation is not training')
        draw_offset = int(draw_offset)
        if not 0 <= draw_offset < 2 ** 32:
            raise RuntimeError('dsnt: draw_offset must lie in [0, 2^32), got %d' % draw_offset)
        x = sample['input']
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
            raise RuntimeError('dsnt: input must be [B, 3, S, S], got %s'
                               % (tuple(x.shape) if isinstance(x, torch.Tensor) else type(x),))
        B, S, K = x.shape[0], x.shape[2], self.max_rects
        if not (1 <= B <= 65535 and 1 <= S <= 4096):
            raise RuntimeError('dsnt: Occlude takes 1 <= B <= 65535 and 1 <= S <= 4096, got B=%d S=%d' % (B, S))
        _check('input', x, torch.float32, (B, 3, S, S))
        dev = x.device
        pc, pm = sample.get('part_coords'), sample.get('part_mask')
        J = pc.shape[1] if isinstance(pc, torch.Tensor) and pc.dim() == 3 else 0
        if J > _OCC_MAX_JOINTS:
            raise RuntimeError('dsnt: Occlude takes at most %d joints, got %d' % (_OCC_MAX_JOINTS, J))
        if pc is not None:
            _check('part_coords', pc, torch.float32, (B, J, 2))
            _check('part_mask', pm, torch.float32, (B, J))
            if pc.device != dev or pm.device != dev:
                raise RuntimeError('dsnt: Occlude inputs must be on one device')
        if rects is None:
            if donor is not None:
                raise RuntimeError('dsnt: a given donor needs given rects')
            draw = 1
            rects = torch.empty(B, K, 4, dtype=torch.int32, device=dev)
            donor = torch.empty(B, dtype=torch.int32, device=dev)
        else:
            draw = 0
            rects = _check('rects', rects, torch.int32, (B, K, 4))
            donor = (torch.arange(1, B + 1, dtype=torch.int32, device=dev) % B if donor is None
                     else _check('donor', donor, torch.int32, (B,)))
            if rects.device != dev or donor.device != dev:
                raise RuntimeError('dsnt: Occlude inputs must be on one device')
        lo, hi = self.sides(S)
        fv, mean, std = self._consts(dev)
        out = torch.empty_like(x)
        occluded = torch.empty(B, J, dtype=torch.uint8, device=dev)
        _lib.call('dsnt_occlude', _lib.ptr(x), _lib.ptr(out), B, S, K, lo, hi, int(round(self.p * 2 ** 24)),
                  _OCC_FILLS[self.fill], _OCC_CENTRES[self.centre], _lib.ptr(fv), _lib.ptr(mean), _lib.ptr(std),
                  _lib.ptr(pc) if J else None, _lib.ptr(pm) if J else None, J, _lib.ptr(rects), _lib.ptr(donor),
                  _lib.ptr(occluded) if J else None, draw, self.seed & (2 ** 64 - 1), int(step) & (2 ** 64 - 1),
                  draw_offset)
        res = dict(sample)
        res['input'] = out
        res['occluded'] = occluded
        if self.mask_covered and pm is not None:
            res['part_mask'] = pm * (1 - occluded.to(torch.float32))
        res['params'] = dict(sample.get('params') or {}, occ_rects=rects, occ_donor=donor)
        return res


_FIELDS = ('crops', 'keypoints', 'keypoint_mask', 'matrix', 'head_lengths')
_DTYPES = (torch.uint8, torch.float64, torch.float32, torch.float64, torch.float64)
_STAGE_BYTES = 64 << 20


def _host_array(name, a):
    """A numpy array (or memmap) of `a`, or `a` itself if it is already a device tensor.  No copy of a host array."""
    if isinstance(a, torch.Tensor):
        return a if a.is_cuda else a.numpy()
    if isinstance(a, np.ndarray):
        return a
    raise RuntimeError('dsnt: %s must be a numpy array or a tensor, got %s' % (name, type(a)))


def _dataset_shapes(crops, keypoints, keypoint_mask, matrix, head_lengths):
    """(N, R, J) of a training set, or an error naming the first field with a wrong shape."""
    if crops.ndim != 4 or crops.shape[1] != crops.shape[2] or crops.shape[3] != 3 or crops.shape[0] < 1:
        raise RuntimeError('dsnt: crops must be [N, R, R, 3] (HWC crops, N >= 1), got %s' % (tuple(crops.shape),))
    N, R = crops.shape[0], crops.shape[1]
    J = keypoints.shape[1] if keypoints.ndim == 3 else -1
    for name, t, shape in (('keypoints', keypoints, (N, J, 2)), ('keypoint_mask', keypoint_mask, (N, J)),
                           ('matrix', matrix, (N, 3, 3)), ('head_lengths', head_lengths, (N,))):
        if tuple(t.shape) != shape or J < 1:
            raise RuntimeError('dsnt: %s must have shape %s, got %s' % (name, shape, tuple(t.shape)))
    return N, R, J


class DeviceDataset:
    """A training set resident on one device: the pool `EpochLoader` gathers batches from.

    Fields (rows = samples): `crops` uint8 `[N, R, R, 3]` (what `DeviceAugment` takes as `src_u8`), `keypoints` float64
    `[N, J, 2]`, `keypoint_mask` float32 `[N, J]`, `matrix` float64 `[N, 3, 3]`, `head_lengths` float64 `[N]`.  The
    constructor takes device tensors of exactly these dtypes; `from_arrays` uploads host data in chunks, `save` / `load`
    keep a packed set as plain `.npy` files.  Only shapes, dtypes and devices are checked.  The full MPII crop set at
    R = 384 (25k samples) is 11 GB.
    """

    def __init__(self, crops, keypoints, keypoint_mask, matrix, head_lengths):
        ts = (crops, keypoints, keypoint_mask, matrix, head_lengths)
        for name, t in zip(_FIELDS, ts):
            if not isinstance(t, torch.Tensor):
                raise RuntimeError('dsnt: DeviceDataset.%s must be a tensor (use DeviceDataset.from_arrays for host data)'
                                   % name)
        N, R, J = _dataset_shapes(*ts)
        for name, t, dtype in zip(_FIELDS, ts, _DTYPES):
            if t.dtype != dtype:
                raise RuntimeError('dsnt: %s must be %s, got %s' % (name, dtype, t.dtype))
        for t in ts:
            _lib.ptr(t)          # refuses CPU and non-contiguous tensors
        if any(t.device != crops.device for t in ts):
            raise RuntimeError('dsnt: DeviceDataset fields must be on one device')
        self.crops, self.keypoints, self.keypoint_mask, self.matrix, self.head_lengths = ts

    def __len__(self):
        return self.crops.shape[0]

    @property
    def device(self):
        return self.crops.device

    @property
    def nbytes(self):
        return sum(getattr(self, f).numel() * getattr(self, f).element_size() for f in _FIELDS)

    @classmethod
    def from_arrays(cls, crops, keypoints, keypoint_mask, matrix, head_lengths, device='cuda', chunk_bytes=_STAGE_BYTES):
        """Upload a training set from numpy arrays, `np.load(..., mmap_mode='r')` memmaps or CPU tensors.  `crops` must
        be uint8; the other fields are converted to their dtype (`keypoint_mask` may be bool or integer).  Every field
        goes through one pinned staging buffer of at most `chunk_bytes`, a chunk of rows at a time, so the host never
        holds a second full copy.  Synchronises with the device (it is the one-off packing step)."""
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('dsnt: DeviceDataset lives on a HIP device, not %s (no CPU fallback)' % device)
        arrays = [_host_array(n, a) for n, a in zip(_FIELDS, (crops, keypoints, keypoint_mask, matrix, head_lengths))]
        _dataset_shapes(*arrays)
        for name, a in zip(_FIELDS, arrays):
            kind = _kind(a)
            if name == 'crops' and str(a.dtype).replace('torch.', '') != 'uint8':
                raise RuntimeError('dsnt: crops must be uint8, got %s' % a.dtype)
            if name in ('keypoints', 'matrix', 'head_lengths') and kind != 'f':
                raise RuntimeError('dsnt: %s must be floating point, got %s' % (name, a.dtype))
            if name == 'keypoint_mask' and kind not in 'biuf':
                raise RuntimeError('dsnt: keypoint_mask must be real or bool, got %s' % a.dtype)
        stage = _stage(arrays, chunk_bytes)
        with torch.cuda.device(device):
            out = [_upload(a, dtype, device, stage) for a, dtype in zip(arrays, _DTYPES)]
        return cls(*out)

    def save(self, directory):
        """Write the fields as `<directory>/<field>.npy` (through one pinned staging buffer; `load` reads them back)."""
        import os
        os.makedirs(directory, exist_ok=True)
        stage = _stage([getattr(self, n) for n in _FIELDS], _STAGE_BYTES)
        for name in _FIELDS:
            t = getattr(self, name)
            mm = np.lib.format.open_memmap(os.path.join(directory, name + '.npy'), mode='w+',
                                           dtype=str(t.dtype).replace('torch.', ''), shape=tuple(t.shape))
            rows = _chunk_rows(t, stage)
            for r0 in range(0, len(t), rows):
                part = t[r0:r0 + rows]
                buf = stage[:part.numel() * t.element_size()].view(t.dtype).view(part.shape)
                buf.copy_(part)                                  # synchronous: the device has written it on return
                mm[r0:r0 + rows] = buf.numpy()
            mm.flush()
            del mm

    @classmethod
    def load(cls, directory, device='cuda', chunk_bytes=_STAGE_BYTES):
        """A set written by `save`: the `.npy` files are memory-mapped and uploaded in chunks."""
        import os
        arrays = [np.load(os.path.join(directory, n + '.npy'), mmap_mode='r') for n in _FIELDS]
        return cls.from_arrays(*arrays, device=device, chunk_bytes=chunk_bytes)

    @classmethod
    def from_pool(cls, pool, idx, matrix, keypoints, keypoint_mask, head_lengths, size=384, chunk_bytes=_STAGE_BYTES):
        """A training set cropped on the device from the full images of an `ImagePool`: row i is `pool.crop` of image
        `idx[i]` through `matrix[i]` at `size` x `size`, written by `dsnt_crop_affine` a chunk of rows at a time straight
        into the crop tensor.  `idx` [N] (integer), `matrix` [N, 3, 3], `keypoints` [N, J, 2] (original-image pixels),
        `keypoint_mask` [N, J], `head_lengths` [N]: numpy arrays, CPU tensors or tensors on the pool's device; host data
        is uploaded as `from_arrays` does.  The crops follow `matrix` and Pillow's affine sampler, not torchdata's
        `load_cropped_image`.  Raises if a row has no crop (index outside the pool, singular matrix); that check
        synchronises once, at the end (it is the one-off packing step)."""
        if not isinstance(pool, ImagePool):
            raise RuntimeError('dsnt: from_pool needs an ImagePool, got %s' % type(pool))
        device = pool.device
        names = ('idx', 'matrix', 'keypoints', 'keypoint_mask', 'head_lengths')
        arrays = [_host_array(n, a) for n, a in zip(names, (idx, matrix, keypoints, keypoint_mask, head_lengths))]
        N = arrays[0].shape[0] if arrays[0].ndim == 1 else -1
        J = arrays[2].shape[1] if arrays[2].ndim == 3 else -1
        for name, a, shape in zip(names, arrays, ((N,), (N, 3, 3), (N, J, 2), (N, J), (N,))):
            if tuple(a.shape) != shape or N < 1 or J < 1:
                raise RuntimeError('dsnt: %s must have shape %s, got %s' % (name, shape, tuple(a.shape)))
        if _kind(arrays[0]) not in 'iu':
            raise RuntimeError('dsnt: idx must be integer, got %s' % arrays[0].dtype)
        for name, a in zip(names[1:], arrays[1:]):
            if _kind(a) not in ('biuf' if name == 'keypoint_mask' else 'f'):
                raise RuntimeError('dsnt: %s must be %s, got %s' % (name, 'real or bool' if name == 'keypoint_mask'
                                                                     else 'floating point', a.dtype))
        R = int(size)
        if not 1 <= R <= 8192:
            raise RuntimeError('dsnt: size must lie in [1, 8192], got %d' % R)
        stage = _stage(arrays, chunk_bytes)
        dtypes = (torch.int64, torch.float64, torch.float64, torch.float32, torch.float64)
        with torch.cuda.device(device):
            rows, m, kp, km, hl = [_upload(a, dt, device, stage) for a, dt in zip(arrays, dtypes)]
            crops = torch.empty(N, R, R, 3, dtype=torch.uint8, device=device)
            valid = torch.empty(N, dtype=torch.uint8, device=device)
            for r0 in range(0, N, _CROP_ROWS):
                r1 = min(N, r0 + _CROP_ROWS)
                pool._crop_into(rows[r0:r1], m[r0:r1], crops[r0:r1], valid[r0:r1])
            bad = int((valid == 0).sum())
        if bad:
            raise RuntimeError('dsnt: from_pool: %d of %d rows have no crop (index outside the pool of %d images, or a '
                               'singular or non-finite matrix)' % (bad, N, len(pool)))
        return cls(crops, kp, km, m, hl)


def _kind(a):
    """numpy's dtype kind ('b', 'i', 'u', 'f', ...) of an array or a tensor."""
    if isinstance(a, torch.Tensor):
        if a.dtype == torch.bool:
            return 'b'
        return 'f' if a.dtype.is_floating_point else 'c' if a.dtype.is_complex else 'u' if a.dtype == torch.uint8 else 'i'
    return a.dtype.kind


def _stage(arrays, chunk_bytes):
    """The one pinned staging buffer of an upload or a save: at most `chunk_bytes`, at least one row (8-byte
    elements) of every field."""
    row = max(int(np.prod(a.shape[1:], dtype=np.int64)) * 8 for a in arrays)
    return torch.empty(max(row, min(int(chunk_bytes), row * len(arrays[0]))), dtype=torch.uint8, pin_memory=True)


def _chunk_rows(t, stage):
    row = max(1, int(np.prod(t.shape[1:], dtype=np.int64))) * t.element_size()
    return max(1, stage.numel() // row)


def _upload(a, dtype, device, stage, dst=None):
    """`a` on `device` as `dtype`, through the pinned `stage` a chunk of rows at a time; into `dst` (a contiguous device
    tensor of `a`'s shape) when given."""
    if isinstance(a, torch.Tensor):                    # already on a device
        if dst is not None:
            return dst.copy_(a)
        return a.to(device=device, dtype=dtype).contiguous()
    if dst is None:
        dst = torch.empty(a.shape, dtype=dtype, device=device)
    rows = _chunk_rows(dst, stage)
    for r0 in range(0, len(a), rows):
        part = a[r0:r0 + rows]
        buf = stage[:part.size * dst.element_size()].view(dtype).view(part.shape)
        np.copyto(buf.numpy(), part, casting='unsafe')
        dst[r0:r0 + len(part)].copy_(buf, non_blocking=True)
        torch.cuda.current_stream().synchronize()      # the staging buffer is reused by the next chunk
    return dst


class EpochLoader:
    """Epochs of `DeviceAugment` samples gathered from a `DeviceDataset`, with no host work per batch.

    `EpochLoader(dataset, batch_size, augment, seed=0, shuffle=True, drop_last=False, rank=0, world_size=1,
    flip_pair=False, occlude=None)`.  Iterating yields the rest of the current epoch (then moves to the next), as the reference's
    `DataLoader(..., shuffle=True)` does.  Each sample is `DeviceAugment`'s dict (same keys and dtypes; `input_pair`
    with `flip_pair`) plus `index`, int64 `[B]`, the dataset rows used.  A batch is three launches on the current
    stream: the indices (`dsnt_epoch_indices`), the image and the keypoints (the `_gather` kernels, which read the
    rows directly from the pool).  Nothing synchronises with the host and nothing crop-sized is allocated.

    Order: position p of epoch e is `order(p)`, a bijection of [0, N) keyed by (`seed`, e), computed on the device
    (`csrc/augment.hip`); `shuffle=False` keeps dataset order.  Augmentation: step `e * len(self) + b` of `augment`
    (keyed by `augment.seed`), so resuming at (epoch, batch) reproduces the batch.  `drop_last=False` keeps a final
    partial batch.  With `world_size` W > 1 (`drop_last` required), rank r takes positions
    `[(s*W + r)*B, (s*W + r + 1)*B)` of the epoch's order at its batch s and draws with sample offset r*B: the ranks
    shard one epoch without communicating.  With `use_aug=False` the identity parameters are shared read-only
    tensors.  `occlude`: an `Occlude` applied to every batch (one more launch) with the batch's own step and the rank's
    draw offset, so resuming and rank sharding reproduce the occlusions as they reproduce the augmentation; not with
    `flip_pair`.  `None`: the batches are exactly those of a loader without the argument.
    """

    def __init__(self, dataset, batch_size, augment, seed=0, shuffle=True, drop_last=False, rank=0, world_size=1,
                 flip_pair=False, occlude=None):
        if not isinstance(dataset, DeviceDataset):
            raise RuntimeError('dsnt: EpochLoader needs a DeviceDataset, got %s' % type(dataset))
        if not isinstance(augment, DeviceAugment):
            raise RuntimeError('dsnt: EpochLoader needs a DeviceAugment, got %s' % type(augment))
        if occlude is not None and not isinstance(occlude, Occlude):
            raise RuntimeError('dsnt: occlude must be an Occlude or None, got %s' % type(occlude))
        if occlude is not None and flip_pair:
            raise RuntimeError('dsnt: occlude does not go with flip_pair (flip evaluation is not training)')
        self.dataset = dataset
        B, W, r, n = int(batch_size), int(world_size), int(rank), self._positions()
        if B < 1 or B > 65535:
            raise RuntimeError('dsnt: batch_size must be in [1, 65535], got %d' % B)
        if W < 1 or not 0 <= r < W:
            raise RuntimeError('dsnt: need 0 <= rank < world_size, got rank %d of %d' % (r, W))
        if W > 1 and not drop_last:
            raise RuntimeError('dsnt: world_size > 1 needs drop_last=True (every rank takes whole batches)')
        if drop_last and B * W > n:
            raise RuntimeError('dsnt: drop_last with batch_size %d x world_size %d > %d samples leaves no batch'
                               % (B, W, n))
        if r * B >= 2 ** 32:
            raise RuntimeError('dsnt: rank * batch_size must be < 2^32 (the draw offset)')
        augment._flip_table(dataset.keypoints.shape[1], augment.use_aug, dataset.device)    # refuses J != 16 with flips
        self.batch_size, self.augment = B, augment
        self.seed, self.shuffle, self.drop_last = int(seed), bool(shuffle), bool(drop_last)
        self.rank, self.world_size, self.flip_pair = r, W, bool(flip_pair)
        self.occlude = occlude
        self.epoch, self.batch = 0, 0
        self._identity = {}

    def _positions(self):
        """Positions of one epoch over all ranks (a subclass may run epochs of another length)."""
        return len(self.dataset)

    def __len__(self):
        """Batches per epoch of this rank."""
        n, B = self._positions(), self.batch_size
        return n // (B * self.world_size) if self.drop_last else (n + B - 1) // B

    def set_epoch(self, epoch):
        self.epoch, self.batch = int(epoch), 0

    def state_dict(self):
        """Where iteration resumes: `batch` is the next batch of `epoch` to yield."""
        return {'epoch': self.epoch, 'batch': self.batch, 'seed': self.seed}

    def load_state_dict(self, state):
        self.epoch, self.batch, self.seed = int(state['epoch']), int(state['batch']), int(state['seed'])

    def _order(self, epoch, first, count):
        idx = torch.empty(count, dtype=torch.int64, device=self.dataset.device)
        _lib.call('dsnt_epoch_indices', len(self.dataset), self.seed & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1), first,
                  count, 1 if self.shuffle else 0, _lib.ptr(idx))
        return idx

    def indices(self, epoch=None):
        """The order of `epoch` (default: the current one) over all ranks, int64 `[N]` on the device."""
        return self._order(self.epoch if epoch is None else epoch, 0, len(self.dataset))

    def _params(self, B, dev):
        if self.augment.use_aug:
            return (1, torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev),
                    torch.empty(B, dtype=torch.uint8, device=dev), torch.empty(B, 3, dtype=torch.float32, device=dev))
        p = self._identity.get(B)
        if p is None:                                      # read by the kernels, never written (draw == 0)
            p = self._identity[B] = (0, torch.ones(B, dtype=torch.float32, device=dev),
                                     torch.zeros(B, dtype=torch.float32, device=dev),
                                     torch.zeros(B, dtype=torch.uint8, device=dev),
                                     torch.ones(B, 3, dtype=torch.float32, device=dev))
        return p

    def _batch(self, epoch, s):
        d, B, W, r = self.dataset, self.batch_size, self.world_size, self.rank
        first = (s * W + r) * B
        count = min(B, self._positions() - first)
        idx = self._order(epoch, first, count)
        p = self._params(count, d.device)
        sample = self.augment._launch(d.crops, d.keypoints, d.keypoint_mask, d.matrix, count, epoch * len(self) + s, p,
                                      self.flip_pair, False, gather=(idx, d.head_lengths, r * B))
        sample['hflip'] = p[3].view(torch.bool)
        sample['index'] = idx
        if self.occlude is not None:
            sample = self.occlude(sample, epoch * len(self) + s, draw_offset=r * B)
        return sample

    def __iter__(self):
        while self.batch < len(self):
            s = self.batch
            sample = self._batch(self.epoch, s)
            self.batch = s + 1
            yield sample
        self.epoch, self.batch = self.epoch + 1, 0


_SAMPLE_MAX_N = 1 << 24    # DSNT_SAMPLE_MAX_N
_SAMPLE_TILE = 1024        # DSNT_SAMPLE_TILE


class ExampleScores:
    """Per dataset row, how badly the row was predicted the last time it was seen.

    `ExampleScores(n, device='cuda')` owns `table`, int64 `[n]` on the device: `(stamp << 32) | bits(score)` of the row's
    latest batch, 0 for a row never seen.  The score of an example is the mean over its joints with mask 1 of the PCKh
    distance (`PCKhEvaluator`'s, in head lengths), fp32.  `stamp` is the caller's clock, an integer in [1, 2^31) that does
    not decrease (the epoch number plus one, or the global step): the newest stamp owns a row, and within one stamp the
    larger score, so a row drawn twice in a batch ends the same way whatever the order of arrival.
    """

    def __init__(self, n, device='cuda'):
        n, device = int(n), torch.device(device)
        if n < 1:
            raise RuntimeError('dsnt: ExampleScores needs n >= 1 rows, got %d' % n)
        if device.type != 'cuda':
            raise RuntimeError('dsnt: ExampleScores lives on a HIP device, not %s (no CPU fallback)' % device)
        self.table = torch.zeros(n, dtype=torch.int64, device=device)

    def __len__(self):
        return self.table.shape[0]

    def add(self, index, norm_pred, norm_target, joint_mask, head_lengths, transform_m, transform_b, stamp):
        """Score a batch given in normalised coords (back-projected in fp64 as in `PCKhEvaluator.add_normalized`) and leave
        the scores in the rows `index` (int64 `[B]`, `EpochLoader`'s `sample['index']`; a row outside the table, such as the
        -1 of an all-zero weighting, and an example with no valid joint or a non-finite score write nothing).  Returns the
        scores, f32 `[B]`, NaN with no valid joint.  One launch; nothing is read back to the host."""
        B, J = norm_pred.shape[0], norm_pred.shape[1]
        stamp = int(stamp)
        if not 1 <= stamp < 2 ** 31:
            raise RuntimeError('dsnt: stamp must lie in [1, 2^31), got %d' % stamp)
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or tuple(index.shape) != (B,):
            raise RuntimeError('dsnt: index must be an int64 [%d] tensor' % B)
        dev = self.table.device
        if norm_pred.device != dev or index.device != dev:
            raise RuntimeError('dsnt: the batch must be on the table\'s device %s' % dev)
        args = _batch_args(norm_pred, norm_target, joint_mask, head_lengths, transform_m, transform_b)
        score = torch.empty(B, dtype=torch.float32, device=dev)
        _lib.call('dsnt_example_scores', *map(_lib.ptr, args), _lib.ptr(index.contiguous()), len(self), stamp,
                  _lib.ptr(self.table), _lib.ptr(score), B, J)
        return score

    @staticmethod
    def _split(table):
        """(seen bool, score f32, stamp int64) of a table, on the table's device."""
        if not isinstance(table, torch.Tensor) or table.dtype != torch.int64 or table.dim() != 1:
            raise RuntimeError('dsnt: a score table is an int64 [n] tensor')
        return table != 0, (table & 0xFFFFFFFF).to(torch.int32).view(torch.float32), table >> 32

    def scores(self):
        """f32 `[n]`: the latest score of every row, NaN for a row never seen."""
        seen, score, _ = self._split(self.table)
        return torch.where(seen, score, torch.full_like(score, float('nan')))

    def last_seen(self):
        """int64 `[n]`: the stamp of every row's latest score, 0 for a row never seen."""
        return self._split(self.table)[2]

    def merge(self, other_table):
        """Take the element-wise maximum with another table (an `ExampleScores` or its `table`): per row the newer stamp,
        the larger score within one stamp.  This is how the tables of two ranks combine."""
        other = other_table.table if isinstance(other_table, ExampleScores) else other_table
        if not isinstance(other, torch.Tensor) or other.dtype != torch.int64 or other.shape != self.table.shape:
            raise RuntimeError('dsnt: merge needs an int64 [%d] table' % len(self))
        torch.maximum(self.table, other.to(self.table.device), out=self.table)

    def state_dict(self):
        return {'table': self.table.clone()}

    def load_state_dict(self, state):
        table = state['table']
        if not isinstance(table, torch.Tensor) or table.dtype != torch.int64 or table.shape != self.table.shape:
            raise RuntimeError('dsnt: the state holds no int64 [%d] table' % len(self))
        self.table.copy_(table)

    @staticmethod
    def weights_from_table(table, power=1.0, floor=0.1, unseen='max'):
        """Row weights from a score table (int64 `[n]`, on any device): f32 `[n]`.  A seen row gets
        `floor + (score / mean seen score) ** power` (the ratio reads as 1 while the mean is 0: nothing to tell rows
        apart by), an unseen row the largest weight of a seen row (`unseen='max'`: see everything before trusting the
        scores) or 1 (`unseen='mean'`); with no row seen every weight is 1.  Plain torch ops on the table's device, once
        per re-weighting, without a host synchronisation."""
        power, floor = float(power), float(floor)
        if not (math.isfinite(power) and math.isfinite(floor) and floor >= 0):
            raise RuntimeError('dsnt: weights_from_table needs a finite power and a finite floor >= 0, got %r and %r'
                               % (power, floor))
        if unseen not in ('max', 'mean'):
            raise RuntimeError("dsnt: unseen must be 'max' or 'mean', got %r" % (unseen,))
        seen, score, _ = ExampleScores._split(table)
        one = torch.ones_like(score)
        count = seen.sum()
        mean = (torch.where(seen, score, torch.zeros_like(score)).double().sum() / count).float()
        w = floor + torch.where(mean > 0, score / mean, one) ** power
        rest = torch.where(seen, w, torch.full_like(w, float('-inf'))).max() if unseen == 'max' else one
        return torch.where(count > 0, torch.where(seen, w, rest), one)


class WeightedLoader(EpochLoader):
    """Epochs that draw rows with replacement in proportion to row weights, with no host work per batch.

    `WeightedLoader(dataset, batch_size, augment, weights, seed=0, samples_per_epoch=None, drop_last=False, rank=0,
    world_size=1, flip_pair=False, occlude=None)`: an `EpochLoader` whose position p of epoch e is a weighted draw keyed by (`seed`, e,
    p) alone (`dsnt_sample_indices`), not a permutation: a row may come twice in a batch, and a row may not come at all.
    An epoch is `samples_per_epoch` positions (default `len(dataset)`, at most 2^32); batches, ranks, `drop_last`, the
    augmentation's steps and draw offsets are `EpochLoader`'s, with that number in the place of the dataset's length.

    `weights`: f32 `[len(dataset)]` on the dataset's device, any scale.  NaN, infinite, negative and zero weights count as
    0, and so does a weight below about 2^-32 of the largest: such rows are never drawn (the CDF is exact fixed point at 32
    bits below the largest weight's binade, `dsnt_sample_cdf`).  If no weight counts every index is -1 and every sample
    NaN with mask 0.  `set_weights(w)` rebuilds the CDF in place (five small launches, nothing allocated but the call's
    own temporaries); between epochs or mid-epoch, the next batch draws from it.  `state_dict()` carries the CDF, so a
    resumed loader repeats the uninterrupted batches exactly.
    """

    def __init__(self, dataset, batch_size, augment, weights, seed=0, samples_per_epoch=None, drop_last=False, rank=0,
                 world_size=1, flip_pair=False, occlude=None):
        self._samples = None if samples_per_epoch is None else int(samples_per_epoch)
        if self._samples is not None and not 1 <= self._samples <= 2 ** 32:
            raise RuntimeError('dsnt: samples_per_epoch must lie in [1, 2^32], got %d' % self._samples)
        super().__init__(dataset, batch_size, augment, seed=seed, shuffle=True, drop_last=drop_last, rank=rank,
                         world_size=world_size, flip_pair=flip_pair, occlude=occlude)
        n = len(dataset)
        if n > _SAMPLE_MAX_N:
            raise RuntimeError('dsnt: WeightedLoader takes at most 2^24 rows, got %d' % n)
        self._check_weights(weights)
        self._cdf = torch.empty(n, dtype=torch.int64, device=dataset.device)
        self._scratch = torch.empty(1 + (n + _SAMPLE_TILE - 1) // _SAMPLE_TILE, dtype=torch.int64, device=dataset.device)
        self.set_weights(weights)

    def _check_weights(self, w):
        n, dev = len(self.dataset), self.dataset.device
        if not isinstance(w, torch.Tensor) or w.dtype != torch.float32:
            raise RuntimeError('dsnt: weights must be a float32 tensor, got %s'
                               % (w.dtype if isinstance(w, torch.Tensor) else type(w),))
        if tuple(w.shape) != (n,):
            raise RuntimeError('dsnt: weights must have shape %s (one per dataset row), got %s' % ((n,), tuple(w.shape)))
        if w.device != dev:
            raise RuntimeError('dsnt: weights must be on the dataset\'s device %s, got %s' % (dev, w.device))

    def _positions(self):
        return len(self.dataset) if self._samples is None else self._samples

    def set_weights(self, weights):
        """Draw from `weights` (f32 `[len(dataset)]` on the dataset's device) from the next batch on."""
        self._check_weights(weights)
        _lib.call('dsnt_sample_cdf', _lib.ptr(weights.detach()), len(self.dataset), _lib.ptr(self._cdf),
                  _lib.ptr(self._scratch))

    def state_dict(self):
        """`EpochLoader`'s state and the CDF the next batch draws from."""
        return dict(super().state_dict(), cdf=self._cdf.clone())

    def load_state_dict(self, state):
        cdf = state['cdf']
        if not isinstance(cdf, torch.Tensor) or cdf.dtype != torch.int64 or cdf.shape != self._cdf.shape:
            raise RuntimeError('dsnt: the state holds no int64 [%d] CDF' % self._cdf.shape[0])
        super().load_state_dict(state)
        self._cdf.copy_(cdf)

    def _order(self, epoch, first, count):
        idx = torch.empty(count, dtype=torch.int64, device=self.dataset.device)
        _lib.call('dsnt_sample_indices', _lib.ptr(self._cdf), len(self.dataset), self.seed & (2 ** 64 - 1),
                  int(epoch) & (2 ** 64 - 1), first, count, _lib.ptr(idx))
        return idx

    def indices(self, epoch=None):
        """The draws of `epoch` (default: the current one) over all ranks, int64 `[samples_per_epoch]` on the device."""
        return self._order(self.epoch if epoch is None else epoch, 0, self._positions())


_MAX_SIDE = 16384          # dsnt_crop_affine's bound on an image side
_CROP_ROWS = 8192          # samples per dsnt_crop_affine launch in DeviceDataset.from_pool (a launch takes <= 65535)


def box_matrix(center, side, device=None):
    """The bounding-box matrix of square boxes, f64 `[B, 3, 3]`: original-image pixels -> box coordinates in [-1, 1]
    (`n = (x - cx) * 2 / side`, the convention of `DeviceAugment`'s and `ImagePool.crop`'s `matrix`).  `center` `[B, 2]`
    (cx, cy) and `side` `[B]`, in pixels, on any device (default: `center`'s).  Entries: `2 / side` on the diagonal,
    `-2 * cx / side` and `-2 * cy / side` in the last column, 1 in the corner, computed in fp64 where the result lives
    (on the device for device tensors: no host round trip).  Any detector's box maps onto it, e.g. `center` = the box
    centre and `side` = 1.25 * max(width, height)."""
    c = torch.as_tensor(center, dtype=torch.float64, device=device)
    s = torch.as_tensor(side, dtype=torch.float64, device=c.device)
    if c.dim() != 2 or c.shape[1] != 2 or tuple(s.shape) != (c.shape[0],):
        raise RuntimeError('dsnt: box_matrix needs center [B, 2] and side [B], got %s and %s'
                           % (tuple(c.shape), tuple(s.shape)))
    m = torch.zeros(c.shape[0], 3, 3, dtype=torch.float64, device=c.device)
    m[:, 0, 0] = 2 / s
    m[:, 1, 1] = 2 / s
    m[:, 0, 2] = -2 * c[:, 0] / s
    m[:, 1, 2] = -2 * c[:, 1] / s
    m[:, 2, 2] = 1
    return m


def _image(i, a):
    """Image `i` of `ImagePool.from_images` as a numpy array or a device tensor, checked to be H x W x 3 uint8."""
    if not isinstance(a, (np.ndarray, torch.Tensor)):
        raise RuntimeError('dsnt: image %d must be an H x W x 3 uint8 numpy array or tensor, got %s (decode it and convert '
                           "a PIL image with np.asarray(img.convert('RGB')))" % (i, type(a)))
    a = _host_array('image %d' % i, a)
    dtype = str(a.dtype).replace('torch.', '')
    if a.ndim != 3 or a.shape[2] != 3 or dtype != 'uint8':
        raise RuntimeError("dsnt: image %d must be H x W x 3 uint8 (RGB), got shape %s of %s; convert with .convert('RGB') "
                           'and np.asarray' % (i, tuple(a.shape), dtype))
    if not (1 <= a.shape[0] <= _MAX_SIDE and 1 <= a.shape[1] <= _MAX_SIDE):
        raise RuntimeError('dsnt: image %d is %d x %d; sides must lie in [1, %d]' % (i, a.shape[0], a.shape[1], _MAX_SIDE))
    return a


class ImagePool:
    """Full RGB images resident on one device, to crop person boxes from (`crop`, `DeviceDataset.from_pool`,
    `inference.predict_boxes`).

    Fields: `data` uint8 `[total]`, the images one after another, each H x W x 3 (HWC, row-major); `offset` int64 `[N]`,
    the byte where image i starts; `hw` int32 `[N, 2]`, its (H, W).  `from_images` packs a list of decoded images;
    decoding (JPEG, PNG) stays with the caller.
    """

    def __init__(self, data, offset, hw):
        for name, t, dtype in (('data', data, torch.uint8), ('offset', offset, torch.int64), ('hw', hw, torch.int32)):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype:
                raise RuntimeError('dsnt: ImagePool.%s must be a %s tensor' % (name, dtype))
        for t in (data, offset, hw):
            _lib.ptr(t)          # refuses CPU and non-contiguous tensors
        N = offset.shape[0] if offset.dim() == 1 else -1
        if data.dim() != 1 or data.numel() < 1 or N < 1 or tuple(hw.shape) != (N, 2):
            raise RuntimeError('dsnt: ImagePool needs data [total], offset [N] and hw [N, 2], got %s, %s and %s'
                               % (tuple(data.shape), tuple(offset.shape), tuple(hw.shape)))
        if offset.device != data.device or hw.device != data.device:
            raise RuntimeError('dsnt: ImagePool fields must be on one device')
        self.data, self.offset, self.hw = data, offset, hw

    def __len__(self):
        return self.offset.shape[0]

    @property
    def device(self):
        return self.data.device

    @classmethod
    def from_images(cls, images, device='cuda', chunk_bytes=_STAGE_BYTES):
        """Pack a list of decoded RGB images: H x W x 3 uint8 numpy arrays, CPU tensors or device tensors, sides up to
        16384.  Host images go through one pinned staging buffer of at most `chunk_bytes`, a chunk of rows at a time,
        straight into the pool.  Synchronises with the device (it is a packing step)."""
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('dsnt: ImagePool lives on a HIP device, not %s (no CPU fallback)' % device)
        arrays = [_image(i, a) for i, a in enumerate(images)]
        if not arrays:
            raise RuntimeError('dsnt: ImagePool.from_images needs at least one image')
        sizes = np.array([a.shape[0] * a.shape[1] * 3 for a in arrays], np.int64)
        offset = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        hw = np.array([a.shape[:2] for a in arrays], np.int32)
        stage = _stage(arrays, chunk_bytes)
        with torch.cuda.device(device):
            data = torch.empty(int(sizes.sum()), dtype=torch.uint8, device=device)
            for a, o, n in zip(arrays, offset, sizes):
                _upload(a, torch.uint8, device, stage, dst=data[int(o):int(o + n)].view(tuple(a.shape)))
            offset_t, hw_t = (_upload(a, dt, device, stage) for a, dt in ((offset, torch.int64), (hw, torch.int32)))
        return cls(data, offset_t, hw_t)

    def _crop_into(self, idx, matrix, out, valid):
        """One dsnt_crop_affine launch: rows of `idx` / `matrix` into `out` uint8 [B, R, R, 3] and `valid` uint8 [B]."""
        B, R = out.shape[0], out.shape[1]
        _lib.call('dsnt_crop_affine', _lib.ptr(self.data), self.data.numel(), _lib.ptr(self.offset), _lib.ptr(self.hw),
                  len(self), _lib.ptr(idx), _lib.ptr(matrix), B, R, _lib.ptr(out), _lib.ptr(valid))

    def _rows(self, idx, matrix):
        """`idx` int64 [B] and `matrix` f64 [B, 3, 3] on the pool's device (dtype conversions run there)."""
        for name, t in (('idx', idx), ('matrix', matrix)):
            if not isinstance(t, torch.Tensor) or t.device != self.device:
                raise RuntimeError('dsnt: %s must be a tensor on the pool\'s device %s' % (name, self.device))
        if idx.dtype.is_floating_point or idx.dtype == torch.bool or idx.dim() != 1 or idx.numel() < 1:
            raise RuntimeError('dsnt: idx must be an integer tensor [B], got %s %s' % (idx.dtype, tuple(idx.shape)))
        B = idx.shape[0]
        if not matrix.dtype.is_floating_point or tuple(matrix.shape) != (B, 3, 3):
            raise RuntimeError('dsnt: matrix must be a floating-point [%d, 3, 3] tensor, got %s %s'
                               % (B, matrix.dtype, tuple(matrix.shape)))
        return idx.to(torch.int64).contiguous(), matrix.to(torch.float64).contiguous()

    def crop(self, idx, matrix, size=384):
        """Crops of boxes: sample b is image `idx[b]` resampled through `matrix[b]` (f64 `[B, 3, 3]`, image pixels ->
        [-1, 1]^2, e.g. `box_matrix`) to `size` x `size`.  Returns `(crops uint8 [B, size, size, 3], valid bool [B])`.
        Equal bit for bit to Pillow's `Image.transform((size, size), AFFINE, data, BILINEAR)` with the coefficients of
        `csrc/augment.hip`; not to torchdata's `load_cropped_image`, whose resampling is not this one.  A sample with
        an index outside the pool or a singular (or non-finite) matrix is all zero and not valid.  One launch on the
        current stream; nothing synchronises with the host.  B <= 65535, 1 <= size <= 8192."""
        idx, matrix = self._rows(idx, matrix)
        B, R = idx.shape[0], int(size)
        if B > 65535 or not 1 <= R <= 8192:
            raise RuntimeError('dsnt: crop takes B <= 65535 and 1 <= size <= 8192, got B=%d size=%d' % (B, R))
        out = torch.empty(B, R, R, 3, dtype=torch.uint8, device=self.device)
        valid = torch.empty(B, dtype=torch.uint8, device=self.device)
        self._crop_into(idx, matrix, out, valid)
        return out, valid.view(torch.bool)
