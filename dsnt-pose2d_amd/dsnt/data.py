"""Input-image contract of the pose models and the training-sample transform (reference `src/dsnt/data.py`).

`ImageSpecs` (`data.py:19-78`) is what the models expose (`model.image_specs`).  `convert` pools a float image to
`size` and normalises it (one HIP launch); `unconvert` undoes the normalisation and returns a PIL image.

`DeviceAugment` is `MPIIDataset.__getitem__` (`data.py:118-226`) for a whole batch on the GPU: from the
`R x R` uint8 crops the MPII loader returns (already on the device) to the model's input, the transformed
keypoints, their mask and the back-projection, in two launches on the current stream with no host round trip.
Reading the MPII files and parsing its annotations stay out of scope: the boundary is "source crops already
on the device".  The exact transform (Pillow's rotation, torchvision 0.2.0's centre crop) is documented in
`csrc/augment.hip`.
"""
import numpy as np
import torch

from . import _lib
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
    Values of given `params` are not checked on the host (that would synchronise): scale must lie in (1/R, 8].
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
        mean, std, flip = self._consts(dev)
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
        if J != flip.numel() and (draw or params is not None):
            raise RuntimeError('dsnt: with flips the keypoints need the %d MPII joints (inference.HFLIP_INDICES), got %d'
                               % (flip.numel(), J))
        if J != flip.numel():
            flip = torch.arange(J, device=dev)       # never applied: no sample is flipped
        S = self.image_specs.size
        pair = torch.empty(2 * B if flip_pair else B, 3, S, S, dtype=torch.float32, device=dev)
        _lib.call('dsnt_augment_fwd_pair' if flip_pair else 'dsnt_augment_fwd', _lib.ptr(src_u8), B, R, S, _lib.ptr(scale),
                  _lib.ptr(rot), _lib.ptr(hflip), _lib.ptr(gain), draw, self.seed & (2 ** 64 - 1),
                  int(step) & (2 ** 64 - 1), _lib.ptr(mean), _lib.ptr(std), _lib.ptr(pair))
        out = pair[:B]
        pc = torch.empty(B, J, 2, dtype=torch.float32, device=dev)
        pm = torch.empty(B, J, dtype=torch.float32, device=dev)
        tm = torch.empty(B, 2, 2, dtype=torch.float64, device=dev)
        tb = torch.empty(B, 1, 2, dtype=torch.float64, device=dev)
        _lib.call('dsnt_augment_keypoints', _lib.ptr(matrix), _lib.ptr(keypoints), _lib.ptr(kmask), B, J,
                  _lib.ptr(scale), _lib.ptr(rot), _lib.ptr(hflip), _lib.ptr(flip), 1 if self.train else 0,
                  _lib.ptr(pc), _lib.ptr(pm), _lib.ptr(tm), _lib.ptr(tb))
        sample = {'normalize': normalize, 'transform_b': tb, 'transform_m': tm, 'input': out, 'part_mask': pm,
                  'part_coords': pc, 'hflip': hflip.bool(),
                  'params': {'scale': scale, 'rot': rot, 'hflip': hflip, 'gain': gain}}
        if flip_pair:
            sample['input_pair'] = pair
        return sample
