"""Test-time prediction with horizontal-flip augmentation.

Mirror of the reference's `generate_predictions` (`/root/reference/src/dsnt/inference.py:12-68`): same
arguments and result (a CPU DoubleTensor `[len(dataset), 16, 2]` of joint positions in original-image
pixels), same quirks — flip augmentation needs `batch_size == 1` (`:15-16`), only the LAST stack's
heat-maps are averaged (`:40-42`), the flipped half is mirrored back and its joints are swapped
left<->right (`:43-45`) before `forward_part2` turns the mean logits into coordinates (`:47-48`), and the
coordinates are mapped back with `baddbmm(transform_b, coords, transform_m)` in fp64 (`:54-57`).
The progress bar and the tele meters are out of scope; `time_meter`, if given, only needs `.add(seconds)`.
The backbone and the DSNT head run on the HIP path (eval-mode BN from the running statistics).

`predict` and `predict_dataset` are the batched form of the same computation (any batch size, flip augmentation
included, nothing synchronising with the host): the mirrored twin of every input runs in the same forward, and one
launch (`flip_merge_head`, `dsnt_flip_merge_head`) merges the last stack's logits, runs the head and back-projects.

`predict_boxes` starts from full images instead of crops: person boxes of an `ImagePool` are cropped on the device
(`dsnt_crop_affine`), then evaluated as `predict` does, and the joints come back in the images' pixels.

`return_stats=True` on the three adds a confidence and a spread per joint, taken from the heat-map the coordinates come
from (see `STATS_DOC`); `calibration=` (an `evaluator.ScoreCalibration`) turns one of them into `p_correct`.

`readout='mode'` on the three replaces the global expectation (or, for 'gauss', the arg-max) by the centroid of the
map's dominant mode (`nn.heatmap_modes`, `dsnt_map_modes`): the read-out that does not land between the
two bumps of a bimodal map.  `return_modes=True` adds the two dominant modes per joint (see `MODES_DOC`).
"""
import ctypes
import time

import torch
from torch.utils.data import DataLoader

from . import _lib
from . import nn as dnn
from . import util as dutil

# MPII_Joint_Horizontal_Flips of `torchdata.mpii` (absent third-party package, reference data.py:15,97):
# the standard MPII order r-ankle, r-knee, r-hip, l-hip, l-knee, l-ankle, pelvis, thorax, upper neck,
# head top, r-wrist, r-elbow, r-shoulder, l-shoulder, l-elbow, l-wrist with left and right swapped.
HFLIP_INDICES = torch.LongTensor([5, 4, 3, 2, 1, 0, 6, 7, 8, 9, 15, 14, 13, 12, 11, 10])


def reverse_tensor(tensor, dim):
    """`util.reverse_tensor` (reference util.py:207-210)."""
    return tensor.flip(dim if dim >= 0 else tensor.dim() + dim)


def generate_predictions(model, dataset, use_flipped=True, batch_size=1, time_meter=None):
    """Generate predictions with the model"""
    if use_flipped:
        assert batch_size == 1, 'test-time flip augmentation only work with batch_size=1'

    model.cuda()
    model.eval()

    loader = DataLoader(dataset, batch_size, num_workers=0)
    preds = torch.zeros(len(dataset), 16, 2, dtype=torch.float64)

    pos = 0
    with torch.no_grad():
        for batch in loader:
            n = batch['input'].size(0)
            start = time.perf_counter()
            if use_flipped:
                sample = batch['input']
                in_var = torch.cat([sample, reverse_tensor(sample, -1)], 0).cuda()
                hm_var = model.forward_part1(in_var)
                if isinstance(hm_var, (list, tuple)):
                    hm_var = hm_var[-1]             # just the last heat-map of a stacked hourglass
                hm1, hm2 = hm_var.split(1)
                hm2 = reverse_tensor(hm2, -1)
                hm2 = hm2.index_select(-3, HFLIP_INDICES.to(hm2.device))
                hm = (hm1 + hm2) / 2
                out_var = model.forward_part2(hm)
            else:
                out_var = model(batch['input'].cuda())
            coords = model.compute_coords(out_var)
            orig_preds = torch.baddbmm(batch['transform_b'].double(), coords.double(),
                                       batch['transform_m'].double())
            if time_meter is not None:
                time_meter.add(time.perf_counter() - start)
            preds[pos:pos + n] = orig_preds
            pos += n
    return preds


# ------------------------------------------------------------------ batched evaluation
_STRATEGIES = {'dsnt': 0, 'gauss': 1}     # DSNT_FLIP_DSNT, DSNT_FLIP_GAUSS
_perm_cache = {}


def _host_perm(perm):
    key = tuple(int(v) for v in perm)
    arr = _perm_cache.get(key)
    if arr is None:
        arr = (ctypes.c_int * len(key))(*key)
        _perm_cache[key] = arr
    return arr


STATS_DOC = """The per-joint statistics dict (`return_stats=True`, `flip_merge_head(stats=True)`): device tensors
  * `peak` f32 `[B, J]`: the largest pixel of the joint's heat-map; `peak_index` int32 `[B, J]`: the first flat index
    `y * w + x` that holds it (-1 for a `predict_boxes` sample without a crop);
  * `mass` f32 `[B, J]`: the sum of the map (1 for softmax);
  * `mean` f32 `[B, J, 2]`: the DSNT expectation of the map.  For the 'dsnt' strategy these are the normalised
    coordinates: bit for bit from the fused flip launch, and to the last bit or two without flip, where the statistics
    come from `dsnt_heatmap_stats` on the stored map and the softmax head sums in another order.  For 'fc' the
    prediction comes from the linear layer and `mean` is NOT it;
  * `cov` f32 `[B, J, 3]`: `(vxx, vyy, vxy)` about that mean, normalised units;
  * `cov_image` f64 `[B, J, 2, 2]`: `transform_m^T . cov . transform_m`, the covariance in original-image pixels^2.
For the 'gauss' strategy the map is the raw merged heat-map, no distribution: `peak`, `peak_index` and `mass` describe it
as it is, and `mean`, `cov` and `cov_image` are NaN.  Nothing here is calibrated to [0, 1]: `peak` (confidence, higher is
better) and `sqrt(trace(cov_image))` (spread in pixels, lower is better) are the two quantities to threshold on, and
`evaluator.Reliability` on a validation set says where.  With `calibration=cal` (an `evaluator.ScoreCalibration` fitted
there) the dict gains
  * `p_correct` f32 `[B, J]`: `cal(stat_score(stats, cal.score))`, the validation set's P(joint within the PCKh threshold)
    at this score (`dsnt_score_lookup`; NaN for a `predict_boxes` sample without a crop)."""


MODES_DOC = """The per-joint modes dict (`return_modes=True`): what `nn.heatmap_modes(map, mode_radius, 2, transform_m,
transform_b)` gives on the map the prediction comes from, device tensors
  * `coords` f32 `[B, J, 2, 2]`: the normalised centroid of the dominant mode (`[:, :, 0]`) and of the runner-up
    (`[:, :, 1]`, typically the mirrored joint), and `image` f64 `[B, J, 2, 2]`: the same in original-image pixels;
  * `mass` f32 `[B, J, 2]`: the map's sum over each mode's window.  It is a score like any other: `mass[..., 0]` goes into
    `evaluator.Reliability` directly, as `evaluator.target_mass` does;
  * `index` int32 `[B, J, 2]`: the windows' centres `y * w + x`; -1 (and NaN elsewhere) where the map has no second mode, and
    for a `predict_boxes` sample without a crop."""


def _check_readout(model, readout):
    if readout not in ('mean', 'mode'):
        raise ValueError("dsnt: readout must be 'mean' or 'mode', not %r" % (readout,))
    if readout == 'mode' and model.output_strat == 'fc':
        raise ValueError("dsnt: readout='mode' reads the heat-map; the 'fc' strategy predicts from its linear layer, not "
                         'from the map')


def _calibrate(st, return_stats, calibration):
    """Add `p_correct` to the statistics dict in the list `st` (empty without `return_stats`)."""
    if calibration is None:
        return
    if not return_stats:
        raise ValueError('dsnt: calibration= needs return_stats=True (p_correct is returned in the statistics dict)')
    from .evaluator import stat_score
    st[0]['p_correct'] = calibration(stat_score(st[0], calibration.score))


def _cov_image(cov, tm):
    """`M^T S M` in fp64 for `cov` f32 `[B, J, 3]` = (vxx, vyy, vxy) and `tm` f64 `[B, 2, 2]`: `[B, J, 2, 2]`."""
    c = cov.double()
    S = torch.stack([c[..., 0], c[..., 2], c[..., 2], c[..., 1]], -1).view(*c.shape[:-1], 2, 2)
    M = tm.reshape(-1, 1, 2, 2)
    return M.transpose(-1, -2) @ (S @ M)


def _map_stats(hm, tm, distribution=True):
    """The statistics dict of materialised heat-maps `[B, J, h, w]` (`dsnt_heatmap_stats`, then `cov_image` by the fused
    launch's fp64 rule).  `distribution=False` (raw 'gauss' maps): mean, cov and cov_image are NaN."""
    st = dnn.heatmap_stats(hm)
    if not distribution:
        st['mean'] = torch.full_like(st['mean'], float('nan'))
        st['cov'] = torch.full_like(st['cov'], float('nan'))
    st['cov_image'] = _cov_image(st['cov'], tm)
    return st


def flip_merge_head(logits, transform_m, transform_b, strategy='dsnt', preact='softmax', perm=None, heatmaps=True,
                    stats=False):
    """The merge and head of flip test-time augmentation for a paired batch, in one launch (`dsnt_flip_merge_head`).

    `logits` f32 `[2B, J, h, w]`: the last stack's heat-map logits, rows `B..2B-1` those of the mirrored inputs.
    Merges `(L[b] + L[B+b][perm].flip(-1)) / 2` (inference.py:40-46 of the reference), then `strategy` 'dsnt'
    applies `preact` and the DSNT expectation (the values `forward_part2` + `compute_coords` give on the merged
    logits) and 'gauss' decodes the arg-max (`util.decode_heatmaps`).  `perm` defaults to `HFLIP_INDICES` (a host
    sequence; it is checked there, never read from the device).  Returns `(image_coords, coords, heatmaps)`: f64
    `[B, J, 2]` = `transform_b + coords @ transform_m`, the normalised f32 `[B, J, 2]`, and the merged heat-maps
    `[B, J, h, w]` (or None when `heatmaps=False`).  `transform_m` f64 `[B, 2, 2]`, `transform_b` f64 `[B, 1, 2]`.
    `stats=True` (`dsnt_flip_merge_head_stats`, the same launch) appends the statistics dict of `STATS_DOC`; the first
    three results keep their bits, and the heat-maps need not be stored for it."""
    if strategy not in _STRATEGIES:
        raise RuntimeError('dsnt: flip_merge_head supports the dsnt and gauss strategies, not %r' % (strategy,))
    if preact not in dnn.PREACT_MODES:
        raise Exception('unrecognised heatmap preactivation function: {}'.format(preact))
    x = _lib.f32(logits).contiguous()
    if x.dim() != 4 or x.size(0) % 2:
        raise RuntimeError('dsnt: flip_merge_head needs paired logits [2B, J, h, w], got %s' % (tuple(x.shape),))
    B, J, h, w = x.size(0) // 2, x.size(1), x.size(2), x.size(3)
    tm = transform_m.to(device=x.device, dtype=torch.float64).reshape(B, 2, 2).contiguous()
    tb = transform_b.to(device=x.device, dtype=torch.float64).reshape(B, 1, 2).contiguous()
    perm = HFLIP_INDICES.tolist() if perm is None else [int(v) for v in perm]
    if len(perm) != J:
        raise RuntimeError('dsnt: flip_merge_head: %d flip indices for %d joints' % (len(perm), J))
    mode = dnn.PREACT_MODES[preact]
    thr = -0.5 if mode == 1 else 0.0           # hm_preact's arguments (model.py:24-45)
    eps = 0.0 if mode == 0 else 1e-12
    coords = torch.empty(B, J, 2, device=x.device, dtype=torch.float32)
    img = torch.empty(B, J, 2, device=x.device, dtype=torch.float64)
    hm = torch.empty(B, J, h, w, device=x.device, dtype=torch.float32) if heatmaps else None
    if not stats:
        _lib.call('dsnt_flip_merge_head', _lib.ptr(x), B, J, h, w, _host_perm(perm), _STRATEGIES[strategy], mode, thr,
                  eps, _lib.ptr(tm), _lib.ptr(tb), _lib.ptr(hm), _lib.ptr(coords), _lib.ptr(img))
        return img, coords, hm
    packed = torch.empty(B * J, 7, device=x.device, dtype=torch.float32)
    index = torch.empty(B * J, device=x.device, dtype=torch.int32)
    cov_image = torch.empty(B, J, 2, 2, device=x.device, dtype=torch.float64)
    _lib.call('dsnt_flip_merge_head_stats', _lib.ptr(x), B, J, h, w, _host_perm(perm), _STRATEGIES[strategy], mode, thr,
              eps, _lib.ptr(tm), _lib.ptr(tb), _lib.ptr(hm), _lib.ptr(coords), _lib.ptr(img), _lib.ptr(packed),
              _lib.ptr(index), _lib.ptr(cov_image))
    st = dnn._stats_dict(packed, index, (B, J))
    st['cov_image'] = cov_image
    return img, coords, hm, st


def _last(out):
    return out[-1] if isinstance(out, (list, tuple)) else out


def _is_hourglass(model):
    from .model import HourglassHumanPoseModel
    return isinstance(model, HourglassHumanPoseModel)


def _predicted_map(model):
    """The heat-map the returned coordinates come from: the LAST stack's for an hourglass (`model.heatmaps` is the
    first stack's, a quirk kept from the reference)."""
    return model.heatmaps_array[-1] if _is_hourglass(model) else model.heatmaps


def _set_heatmaps(model, hm):
    if _is_hourglass(model):
        model.heatmaps_array = [hm]           # `model.heatmaps` is heatmaps_array[0]
    else:
        model.heatmaps = hm


def predict(model, inputs, transform_m, transform_b, use_flipped=True, paired=False, return_normalized=False,
            return_stats=False, calibration=None, readout='mean', mode_radius=3, return_modes=False):
    """Joint positions in original-image pixels for a batch, on the device: f64 `[B, J, 2]`.

    `inputs` f32 `[B, 3, S, S]` on the device, or with `paired=True` the `[2B, 3, S, S]` `input_pair` of
    `data.DeviceAugment(..., flip_pair=True)` (rows `B..2B-1` the mirrored inputs).  `transform_m` `[B, 2, 2]`,
    `transform_b` `[B, 1, 2]`.  Per sample this is what `generate_predictions(..., batch_size=1)` computes, at any
    batch size, for hourglass and ResNet models:
      * `use_flipped`: the pair (built here with ATen's flip unless `paired`) runs in one forward; for the 'dsnt'
        and 'gauss' strategies one `dsnt_flip_merge_head` launch merges the last stack's logits, runs the head and
        back-projects.  The 'fc' strategy falls back to the ATen merge (`flip`, `index_select`, add, divide) and
        `forward_part2`, then `baddbmm`.
      * otherwise: `forward`, the device-side `compute_coords` and `baddbmm`.
    The model is put in eval mode.  Nothing synchronises with the host.  `model.heatmaps` holds the (merged)
    heat-maps afterwards.  `return_normalized=True` returns `(image_coords, normalised f32 coords)`.
    `return_stats=True` appends the statistics dict of `STATS_DOC` to the result (coordinates unchanged bit for bit),
    still without a host synchronisation.  It describes the map the coordinates come from:
      * flip, 'dsnt' / 'gauss': from the fused launch itself (`dsnt_flip_merge_head_stats`);
      * flip, 'fc': `dsnt_heatmap_stats` on the post-activation map of the merged logits;
      * no flip: `dsnt_heatmap_stats` on the last stack's heat-maps (for an hourglass NOT `model.heatmaps`, which is the
        first stack's) after the forward.
    `calibration` (with `return_stats=True`): the dict also holds `p_correct`, one more launch; everything else keeps its
    bits.
    `readout='mode'`: the returned image and normalised coordinates are those of mode 0 of `nn.heatmap_modes(map,
    mode_radius)` on the map the prediction comes from: the merged map the fused launch stores with flip,
    `_predicted_map(model)` without.  One more launch (`dsnt_map_modes`), no host synchronisation; the statistics dict is
    untouched.  'gauss' is allowed (the window centroid of the raw map is a sub-pixel decode); 'fc' raises `ValueError`.
    `readout='mean'` (the default) is the behaviour described above, bit for bit.
    `return_modes=True` appends the dict of `MODES_DOC` (the two dominant modes) after the statistics dict, if any; the
    one launch then serves both (and the mode-0 read-out is copied out of it)."""
    _check_readout(model, readout)
    model.eval()
    S = 2 if (use_flipped and paired) else 1
    if inputs.size(0) % S:
        raise RuntimeError('dsnt: predict(paired=True) needs an input_pair [2B, 3, S, S], got %s' % (tuple(inputs.shape),))
    B = inputs.size(0) // S
    tm = transform_m.to(device=inputs.device, dtype=torch.float64)
    tb = transform_b.to(device=inputs.device, dtype=torch.float64).reshape(B, 1, 2)
    with torch.no_grad():
        if use_flipped:
            pair = inputs if paired else torch.cat([inputs, reverse_tensor(inputs, -1)], 0)
            logits = _last(model.forward_part1(pair))
            strat = model.output_strat
            if strat in _STRATEGIES:
                img, coords, hm, *st = flip_merge_head(logits, tm, tb, strat, model.preact, stats=return_stats)
                _set_heatmaps(model, hm)
            else:
                hm1, hm2 = logits.split(B)
                hm2 = reverse_tensor(hm2, -1).index_select(-3, HFLIP_INDICES.to(hm2.device))
                hm = (hm1 + hm2) / 2
                # a bare tensor would be iterated per sample by the hourglass head (the reference's batch-1 quirk)
                coords = _last(model.forward_part2([hm] if _is_hourglass(model) else hm)).detach().float()
                img = torch.baddbmm(tb, coords.double(), tm)
                st = [_map_stats(_predicted_map(model), tm)] if return_stats else []
        else:
            out = _last(model(inputs))
            coords = dutil.decode_heatmaps(out) if model.output_strat == 'gauss' else out.detach().float()
            img = torch.baddbmm(tb, coords.double(), tm)
            st = [_map_stats(_predicted_map(model), tm, model.output_strat != 'gauss')] if return_stats else []
        if readout == 'mode' or return_modes:
            # (with flip, `_set_heatmaps` has put the merged map the fused launch stored there)
            modes = dnn.heatmap_modes(_predicted_map(model), mode_radius, 2 if return_modes else 1, tm, tb)
            if readout == 'mode':       # (with one mode the views are contiguous as they are: no copy)
                img, coords = modes['image'][:, :, 0].contiguous(), modes['coords'][:, :, 0].contiguous()
    _calibrate(st, return_stats, calibration)
    res = (img, coords) if return_normalized else (img,)
    res += tuple(st)
    if return_modes:
        res += (modes,)
    return res if len(res) > 1 else res[0]


def predict_dataset(model, dataset, use_flipped=True, batch_size=32, time_meter=None, return_stats=False,
                    calibration=None, readout='mean', mode_radius=3, return_modes=False):
    """`generate_predictions` at any batch size: a CPU DoubleTensor `[len(dataset), J, 2]` of joint positions in
    original-image pixels, per sample what the batch-1 flip loop gives.  Predictions stay on the device until the
    one copy at the end; with a `time_meter` each batch is timed, which synchronises once per batch.
    `return_stats=True` returns `(predictions, stats)`: the statistics dict of `STATS_DOC` over the whole dataset as CPU
    tensors, concatenated on the device and copied once like the predictions; with `calibration`, `p_correct` among them.
    `readout` and `mode_radius` are `predict`'s; `return_modes=True` appends the modes dict of `MODES_DOC` over the whole
    dataset to the result, concatenated and copied the same way."""
    _check_readout(model, readout)
    model.cuda()
    model.eval()
    loader = DataLoader(dataset, batch_size, num_workers=0)
    preds, stats, modes = [], [], []
    for batch in loader:
        start = time.perf_counter()
        img = predict(model, batch['input'].cuda(), batch['transform_m'].cuda(), batch['transform_b'].cuda(),
                      use_flipped=use_flipped, return_stats=return_stats, calibration=calibration, readout=readout,
                      mode_radius=mode_radius, return_modes=return_modes)
        if return_stats or return_modes:
            img, *extra = img
            if return_stats:
                stats.append(extra[0])
            if return_modes:
                modes.append(extra[-1])
        if time_meter is not None:
            torch.cuda.synchronize()
            time_meter.add(time.perf_counter() - start)
        preds.append(img)
    if not preds:
        empty = torch.zeros(0, 16, 2, dtype=torch.float64)
        res = (empty,) + ({},) * (int(return_stats) + int(return_modes))
        return res if len(res) > 1 else empty
    res = (torch.cat(preds, 0).cpu(),)
    for dicts in ([stats] if return_stats else []) + ([modes] if return_modes else []):
        res += ({k: torch.cat([d[k] for d in dicts], 0).cpu() for k in dicts[0]},)
    return res if len(res) > 1 else res[0]


_box_augment = {}


def _box_augment_for(specs, mean, std, device):
    """The identity `DeviceAugment` of `predict_boxes`, one per (specs, statistics), with its constants on `device`
    uploaded once: a later call enqueues no host-to-device copy."""
    from .data import DeviceAugment
    key = (specs.size, specs.subtract_mean, specs.divide_stddev, tuple(float(v) for v in mean),
           tuple(float(v) for v in std))
    aug = _box_augment.get(key)
    if aug is None:
        aug = _box_augment[key] = DeviceAugment(specs, mean, std, use_aug=False, train=False)
    aug._consts(device)
    return aug


def predict_boxes(model, pool, idx, matrix, mean, std, use_flipped=True, crop_size=384, return_normalized=False,
                  return_stats=False, calibration=None, readout='mean', mode_radius=3, return_modes=False):
    """Joint positions in original-image pixels for person boxes in full images: f64 `[B, J, 2]` on the device.

    `pool` a `data.ImagePool`; sample b is image `idx[b]` (int64 `[B]`) with the box matrix `matrix[b]` (f64
    `[B, 3, 3]`, image pixels -> [-1, 1]^2, e.g. `data.box_matrix` of a detector's boxes), both on the pool's device.
    `mean` / `std`: the dataset statistics the model was trained with (used as `model.image_specs` says).  The chain:
    `pool.crop(idx, matrix, crop_size)`, then `DeviceAugment(use_aug=False, train=False)` of the crops
    (`flip_pair=use_flipped`), then `predict(..., paired=use_flipped)` with the keypoints kernel's `transform_m` /
    `transform_b` of `matrix`.  `predict` back-projects row vectors as `coords @ transform_m + transform_b`, the
    reference's convention, which is the inverse of `matrix` only when its 2 x 2 part is symmetric (axis-aligned
    boxes); here `transform_m` is passed transposed, so the result is `inverse(matrix) . [x, y, 1]` for any invertible
    matrix, and bit for bit what `predict` gives on axis-aligned boxes.  A sample without a crop (index outside the
    pool, singular matrix) comes out NaN.  Nothing synchronises with the host (the first call on a device uploads the
    normalisation constants).  `return_normalized=True` returns `(image_coords, normalised f32 coords)`.
    `return_stats=True` appends the statistics dict of `STATS_DOC`; `cov_image` follows the transposed `transform_m`, so
    it is in the image's pixels for any invertible box matrix, and a sample without a crop has NaN statistics (its
    `peak_index` is -1).  With `calibration` the dict also holds `p_correct`, NaN for such a sample.
    `readout`, `mode_radius` and `return_modes` are `predict`'s; the modes dict of a sample without a crop is NaN, its
    `index` -1."""
    _check_readout(model, readout)
    crops, valid = pool.crop(idx, matrix, crop_size)
    B, dev = crops.shape[0], crops.device
    aug = _box_augment_for(model.image_specs, mean, std, dev)
    J = HFLIP_INDICES.numel()
    kp = torch.zeros(B, J, 2, dtype=torch.float64, device=dev)
    km = torch.zeros(B, J, dtype=torch.float32, device=dev)
    hl = torch.ones(B, dtype=torch.float64, device=dev)
    m = matrix.to(torch.float64).contiguous()
    s = aug(crops, kp, km, m, hl, 0, flip_pair=use_flipped)
    tm = s['transform_m'].transpose(1, 2).contiguous()
    img, coords, *st = predict(model, s['input_pair'] if use_flipped else s['input'], tm, s['transform_b'],
                               use_flipped=use_flipped, paired=use_flipped, return_normalized=True,
                               return_stats=return_stats, calibration=calibration, readout=readout,
                               mode_radius=mode_radius, return_modes=return_modes)
    img = torch.where(valid.view(B, 1, 1), img, float('nan'))
    res = (img, torch.where(valid.view(B, 1, 1), coords, float('nan'))) if return_normalized else (img,)
    def mask(t):
        return torch.where(valid.view(B, *([1] * (t.dim() - 1))), t, -1 if t.dtype == torch.int32 else float('nan'))
    for d in st:            # the statistics dict, then the modes dict
        res += ({k: mask(v) for k, v in d.items()},)
    return res if len(res) > 1 else res[0]
