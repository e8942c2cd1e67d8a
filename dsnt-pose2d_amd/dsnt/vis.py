"""Looking at predictions on the device: skeleton and heat-map overlays for a whole batch in one launch.

The reference shows its output once per epoch on the host: `unconvert` and `util.draw_skeleton` per image, and the
wrist heat-maps through `ToPILImage` (`bin/train.py:455-483` of the reference).  `render_pose` does the three
for a batch with `dsnt_render_pose` (csrc/render.hip, formulas in DESIGN.md section 15): it reads the model input (or
uint8 crops, or nothing), the heat-maps and the coordinates where they are and writes uint8 `[B, H, W, 3]` pictures
on the current stream, without a host copy or a synchronisation.  `heatmap_image` is the reference's heat-map picture.
Device tensors only (no CPU fallback); text, image encoding and the GUI are not here.
"""
import ctypes as C
import functools

import torch

from . import _lib
from . import nn as dnn
from .evaluator import PCKhEvaluator
from .util import BONES, bone_colour

MAX_JOINTS = 64          # DSNT_RENDER_MAX_JOINTS
MAX_BONES = 32           # DSNT_RENDER_MAX_BONES
_BLACK, _F32, _U8 = 0, 1, 2
RED, BLUE = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)

# the reference's skeleton as a bone table: (j1, j2, (r, g, b)) with the colours in 0..255
DEFAULT_BONES = tuple((a, b, bone_colour(name)) for name, (a, b) in BONES.items())
# train.py:474-478: right wrist in the red channel, left wrist in the blue one
DEFAULT_HEAT_COLORS = {'rwrist': RED, 'lwrist': BLUE}


def _bone_table(bones, J):
    """`bones` checked against `J` joints as the two host arrays the entry point takes."""
    bones = list(DEFAULT_BONES if bones is None else bones)
    if not bones:
        raise RuntimeError('dsnt: an empty bone table draws nothing; leave coords out for no skeleton')
    if len(bones) > MAX_BONES:
        raise RuntimeError('dsnt: render_pose takes at most %d bones, got %d' % (MAX_BONES, len(bones)))
    joints, rgb = [], []
    for k, bone in enumerate(bones):
        try:
            j1, j2, colour = bone
            j1, j2, colour = int(j1), int(j2), [float(c) for c in colour]
        except (TypeError, ValueError):
            raise RuntimeError('dsnt: bone %d must be (j1, j2, (r, g, b)), got %r' % (k, bone))
        if not (0 <= j1 < J and 0 <= j2 < J):
            raise RuntimeError('dsnt: bone %d joins joints %d and %d, outside 0..%d' % (k, j1, j2, J - 1))
        if len(colour) != 3:
            raise RuntimeError('dsnt: bone %d must be (j1, j2, (r, g, b)), got %r' % (k, bone))
        joints += [j1, j2]
        rgb += colour
    return (C.c_int32 * len(joints))(*joints), (C.c_float * len(rgb))(*rgb), len(bones)


def _heat_table(heat_colors, J):
    """The per-joint colour table float [J][3] of a dict from joint name or index to RGB in [0, 1]."""
    if heat_colors is None:
        heat_colors = DEFAULT_HEAT_COLORS
    table = [0.0] * (3 * J)
    for key, colour in heat_colors.items():
        if isinstance(key, str):
            if key not in PCKhEvaluator.JOINT_NAMES:
                raise RuntimeError('dsnt: heat_colors names an unknown joint %r' % (key,))
            j = PCKhEvaluator.JOINT_NAMES.index(key)
        else:
            j = int(key)
        if not 0 <= j < J:
            raise RuntimeError('dsnt: heat_colors joint %r is outside 0..%d' % (key, J - 1))
        colour = [float(c) for c in colour]
        if len(colour) != 3 or not all(0.0 <= c <= 1.0 for c in colour):
            raise RuntimeError('dsnt: heat_colors[%r] must be an RGB triple in [0, 1], got %r' % (key, colour))
        table[3 * j:3 * j + 3] = colour
    return (C.c_float * len(table))(*table)


# the default tables are built once per joint count: building them costs more host time than the launch
_default_bone_table = functools.lru_cache(maxsize=None)(lambda J: _bone_table(None, J))
_default_heat_table = functools.lru_cache(maxsize=None)(lambda J: _heat_table(None, J))


def _tensor(name, t, dtype, shape):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError('dsnt: %s must be a tensor' % name)
    _lib.ptr(t.detach())          # refuses CPU (no CPU fallback) and non-contiguous tensors
    if t.dtype != dtype:
        raise RuntimeError('dsnt: %s must be %s, got %s' % (name, dtype, t.dtype))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError('dsnt: %s must have shape %s, got %s' % (name, tuple(shape), tuple(t.shape)))
    return t.detach()


def _render_args(canvas, coords, mask, mean, std, bones, width, joint_radius, pixel_coords, heatmaps, heat_colors,
                 heat_alpha, peak, out):
    """Everything `render_pose` does on the host before the launch: its arguments checked, and `(args, out, keep)` with
    `args` the argument list of `dsnt_render_pose` up to the stream, `out` the picture tensor and `keep` the tensors the
    pointers in `args` belong to.  (tools/bench_render.py builds it once to time the launch apart from this work.)"""
    if isinstance(canvas, torch.Tensor):
        if canvas.dtype == torch.uint8:
            kind = _U8
            if canvas.dim() != 4 or canvas.size(3) != 3:
                raise RuntimeError('dsnt: a uint8 canvas must be [B, H, W, 3], got %s' % (tuple(canvas.shape),))
            B, H, W = canvas.size(0), canvas.size(1), canvas.size(2)
        else:
            kind = _F32
            if canvas.dim() != 4 or canvas.size(1) != 3:
                raise RuntimeError('dsnt: a float canvas must be [B, 3, H, W], got %s' % (tuple(canvas.shape),))
            B, H, W = canvas.size(0), canvas.size(2), canvas.size(3)
        if kind == _U8 and (mean is not None or std is not None):
            raise RuntimeError('dsnt: mean and std un-normalise a float canvas; a uint8 canvas is taken as it is')
        canvas = _tensor('canvas', canvas, torch.uint8 if kind == _U8 else torch.float32, None)
        device = canvas.device
    else:
        kind, B = _BLACK, None
        try:
            H, W = (int(v) for v in canvas)
        except (TypeError, ValueError):
            raise RuntimeError('dsnt: canvas must be a tensor or (H, W), got %r' % (canvas,))
        if mean is not None or std is not None:
            raise RuntimeError('dsnt: mean and std un-normalise a float canvas; a black canvas has none')
        canvas = None
        lead = coords if coords is not None else heatmaps
        if not isinstance(lead, torch.Tensor) or lead.dim() < 1:
            raise RuntimeError('dsnt: a black canvas needs coords or heatmaps to take the batch size from')
        B, device = lead.size(0), lead.device
    if H < 1 or W < 1 or B < 1:
        raise RuntimeError('dsnt: render_pose needs B, H, W >= 1, got B=%d H=%d W=%d' % (B, H, W))
    if not float(width) > 0:
        raise RuntimeError('dsnt: render_pose needs width > 0, got %r' % (width,))

    J = 1
    if coords is not None:
        if not isinstance(coords, torch.Tensor) or coords.dim() != 3:
            raise RuntimeError('dsnt: coords must be a tensor [B, J, 2]')
        J = coords.size(1)
    elif heatmaps is not None:
        if not isinstance(heatmaps, torch.Tensor) or heatmaps.dim() != 4:
            raise RuntimeError('dsnt: heatmaps must be a tensor [B, J, h, w]')
        J = heatmaps.size(1)
    if not 1 <= J <= MAX_JOINTS:
        raise RuntimeError('dsnt: render_pose takes 1..%d joints, got %d' % (MAX_JOINTS, J))

    joints_arg = rgb_arg = None
    nbones = 0
    if coords is not None:
        coords = _tensor('coords', coords, torch.float32, (B, J, 2))
        if mask is not None:
            mask = _tensor('mask', mask, torch.float32, (B, J))
        joints_arg, rgb_arg, nbones = _default_bone_table(J) if bones is None else _bone_table(bones, J)
    elif mask is not None or bones is not None:
        raise RuntimeError('dsnt: mask and bones belong to a skeleton, which needs coords')

    heat_arg, h, w, stride = None, 0, 0, 1
    if heatmaps is not None:
        heatmaps = _tensor('heatmaps', heatmaps, torch.float32, None)
        if heatmaps.dim() != 4 or heatmaps.size(0) != B or heatmaps.size(1) != J:
            raise RuntimeError('dsnt: heatmaps must be [%d, %d, h, w], got %s' % (B, J, tuple(heatmaps.shape)))
        h, w = heatmaps.size(2), heatmaps.size(3)
        heat_arg = _default_heat_table(J) if heat_colors is None else _heat_table(heat_colors, J)
        if peak is None:
            peak = dnn.heatmap_stats(heatmaps)['peak']
        if not isinstance(peak, torch.Tensor):
            raise RuntimeError('dsnt: peak must be a tensor')
        if not peak.is_cuda:
            raise RuntimeError('dsnt: peak is on %s; render_pose runs on the HIP device only (no CPU fallback)' % peak.device)
        if peak.dtype != torch.float32 or tuple(peak.shape) != (B, J):
            raise RuntimeError('dsnt: peak must be float32 [%d, %d], got %s %s' % (B, J, peak.dtype, tuple(peak.shape)))
        peak = peak.detach()
        # a column of a statistics buffer (stride 7) is read in place
        s = peak.stride(1) if J > 1 else (peak.stride(0) if B > 1 else 1)
        if s >= 1 and (J == 1 or peak.stride(1) == s) and (B == 1 or peak.stride(0) == J * s):
            stride = s
        else:
            peak = peak.contiguous()
    elif peak is not None or heat_colors is not None:
        raise RuntimeError('dsnt: peak and heat_colors belong to a heat-map layer, which needs heatmaps')
    else:
        peak = None

    if out is None:
        out = torch.empty(B, H, W, 3, device=device, dtype=torch.uint8)
    else:
        _tensor('out', out, torch.uint8, (B, H, W, 3))
    for name, t in (('coords', coords), ('mask', mask), ('heatmaps', heatmaps), ('peak', peak), ('out', out)):
        if t is not None and t.device != device:
            raise RuntimeError('dsnt: %s is on %s, the canvas on %s' % (name, t.device, device))
    mean_arg = None if mean is None else (C.c_float * 3)(*[float(v) for v in mean])
    std_arg = None if std is None else (C.c_float * 3)(*[float(v) for v in std])
    args = (_lib.ptr(canvas), kind, mean_arg, std_arg, B, H, W, J,
            _lib.ptr(heatmaps), h, w, None if peak is None else peak.data_ptr(), stride, heat_arg, float(heat_alpha),
            _lib.ptr(coords), _lib.ptr(mask), 1 if pixel_coords else 0, joints_arg, rgb_arg, nbones, float(width),
            float(joint_radius), _lib.ptr(out))
    return args, out, (canvas, coords, mask, heatmaps, peak)


def render_pose(canvas, coords=None, mask=None, *, mean=None, std=None, bones=None, width=2.0, joint_radius=0.0,
                pixel_coords=False, heatmaps=None, heat_colors=None, heat_alpha=1.0, peak=None, out=None):
    """Pictures of a batch of poses: uint8 `[B, H, W, 3]` on the device, one launch (`dsnt_render_pose`).

    `canvas`: the model input f32 `[B, 3, H, W]` (un-normalised with `mean` / `std` per channel as `ImageSpecs.unconvert`
    does, byte for byte; both default to no normalisation), uint8 `[B, H, W, 3]` crops (`ImagePool.crop`), or `(H, W)`
    for black (the batch size then comes from `coords` or `heatmaps`).  `mean` / `std` with a uint8 or black canvas, a
    `width` that is not positive and an empty `bones` are errors, as is a layer's option without its layer.
    Skeleton, when `coords` f32 `[B, J, 2]` is given: normalised coordinates, or continuous pixels with
    `pixel_coords=True` (pixel `i` spans `[i, i + 1)`).  `bones` is a sequence of up to 32 `(j1, j2, (r, g, b))`, colours
    0..255, drawn in order as anti-aliased segments `width` pixels wide; the default is the reference's skeleton.  A bone
    with a non-finite end is skipped; with `mask` f32 `[B, J]`, a bone with a masked-out (0) end is grey.
    `joint_radius > 0` adds a disc on every joint a bone names, in that bone's colour.
    Heat-maps, when `heatmaps` f32 `[B, J, h, w]` is given: each joint of `heat_colors` (a dict from joint name or index
    to RGB in [0, 1]; default right wrist red, left wrist blue) is scaled by its `peak`, resampled bilinearly to the
    canvas, tinted and blended with `heat_alpha` under the skeleton.  `peak` f32 `[B, J]` is each map's maximum:
    `predict(..., return_stats=True)['peak']` or `nn.heatmap_stats(heatmaps)['peak']`, computed here when absent.
    `out`: an optional uint8 `[B, H, W, 3]` to write into (it may be a uint8 `canvas`)."""
    args, out, keep = _render_args(canvas, coords, mask, mean, std, bones, width, joint_radius, pixel_coords, heatmaps,
                                   heat_colors, heat_alpha, peak, out)
    _lib.call('dsnt_render_pose', *args)
    del keep
    return out


def heatmap_image(heatmaps, heat_colors=None):
    """The reference's heat-map picture (train.py:471-480) for a batch: uint8 `[B, h, w, 3]` with
    `255 * clamp(hm / hm.max(), 0, 1)` of each coloured joint in its channel — the right wrist red and the left wrist
    blue unless `heat_colors` says otherwise; a black canvas at the maps' own size with `heat_alpha` 1."""
    if not isinstance(heatmaps, torch.Tensor) or heatmaps.dim() != 4:
        raise RuntimeError('dsnt: heatmaps must be a tensor [B, J, h, w]')
    return render_pose((heatmaps.size(2), heatmaps.size(3)), heatmaps=heatmaps, heat_colors=heat_colors, heat_alpha=1.0)
