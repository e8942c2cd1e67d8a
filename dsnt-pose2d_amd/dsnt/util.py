"""The reference's `dsnt.util` surface (`src/dsnt/util.py`), complete.

On the HIP device: `encode_heatmaps`, `decode_heatmaps` and `get_preds` keep the names, arguments and results of
`util.py:129-198`; `heatmap_mse_loss` is the loss the `gauss` output strategy builds from them
(`model.py:147-156, 247-258`) with the target bump evaluated inside the kernel instead of
being rendered on the CPU and copied over every step.  Their tensors must be fp32 and resident on the HIP device (no CPU
fallback); results stay on the device — `compute_coords` moves them to the CPU as the reference does.  Unlike the
reference, `encode_heatmaps` does not shift and scale the caller's `coords` in place (`util.py:133-136`).

On the host: `BONES` and `draw_skeleton` (`util.py:16-67`), which paints one PIL image with Pillow, for callers ported
unchanged.  A batch is drawn on the device by `dsnt.vis.render_pose`, which takes its default bone table from here.
"""
import torch
from torch.autograd import Function

from ._lib import ptr, f32, call

# The skeleton's 15 bones as the pairs of MPII joints they join, limb by limb in drawing order: interface data, with the
# reference's keys, pairs and order so that ported callers and `draw_skeleton`'s pictures agree with it.  The side a
# name starts with is the bone's colour class.
_LIMBS = (
    ('right', ('lower_leg', 0, 1), ('upper_leg', 1, 2), ('pelvis', 2, 6)),
    ('left', ('lower_leg', 4, 5), ('upper_leg', 3, 4), ('pelvis', 3, 6)),
    ('center', ('lower_torso', 6, 7), ('upper_torso', 7, 8), ('head', 8, 9)),
    ('right', ('lower_arm', 10, 11), ('upper_arm', 11, 12), ('shoulder', 12, 8)),
    ('left', ('lower_arm', 14, 15), ('upper_arm', 13, 14), ('shoulder', 13, 8)),
)
BONES = {side + '_' + part: (j1, j2) for side, *parts in _LIMBS for part, j1, j2 in parts}
BONE_CLASS_COLOURS = {'center': (255, 0, 255), 'left': (0, 0, 255), 'right': (255, 0, 0)}
MASKED_COLOUR = (100, 100, 100)


def bone_colour(name):
    """The RGB colour of a bone by the prefix of its name: magenta centre, blue left, red right, white otherwise."""
    return BONE_CLASS_COLOURS.get(name.split('_', 1)[0], (255, 255, 255))


def draw_skeleton(img, coords, joint_mask=None):
    '''Draw the `BONES` over the PIL image `img`, on the host with Pillow (util.py:35-67): one-pixel lines between the
    0-based pixel coordinates `coords` [16, 2], blue on the left side, red on the right, magenta in the centre, and
    grey where `joint_mask` (optional, [16]) is 0 at either end.'''
    from PIL.ImageDraw import Draw
    pen = Draw(img)
    for name, (a, b) in BONES.items():
        masked = joint_mask is not None and (joint_mask[a] == 0 or joint_mask[b] == 0)
        ends = [float(coords[a][0]), float(coords[a][1]), float(coords[b][0]), float(coords[b][1])]
        pen.line(ends, fill=MASKED_COLOUR if masked else bone_colour(name))


def encode_heatmaps(coords, width, height, sigma=1):
    '''Convert normalised coordinates [B, J, 2] into heatmaps [B, J, height, width] (util.py:129-147).'''
    c = f32(coords).detach().contiguous()
    out = torch.empty(*c.shape[:-1], height, width, device=c.device, dtype=torch.float32)
    call('dsnt_encode_heatmaps', ptr(c), ptr(out), c.numel() // 2, height, width, float(sigma))
    return out


def decode_heatmaps(heatmaps, use_neighbours=True):
    '''Convert heatmaps [B, J, H, W] into normalised coordinates [B, J, 2] (util.py:172-198).'''
    hm = f32(heatmaps).detach().contiguous()
    height, width = hm.size(-2), hm.size(-1)
    out = torch.empty(*hm.shape[:-2], 2, device=hm.device, dtype=torch.float32)
    rows = hm.numel() // (height * width)
    call('dsnt_decode_heatmaps', ptr(hm), ptr(out), rows, height, width, 1 if use_neighbours else 0)
    return out


def get_preds(heatmaps):
    '''Arg-max pixel coordinates (x, y) as floats, (0, 0) where the maximum is not positive (util.py:150-169).'''
    height, width = heatmaps.size(-2), heatmaps.size(-1)
    c = decode_heatmaps(heatmaps, use_neighbours=False)
    px = torch.round((c[..., 0] + 1) * (width / 2) - 0.5)
    py = torch.round((c[..., 1] + 1) * (height / 2) - 0.5)
    return torch.stack([px, py], -1)


class _HeatmapMSE(Function):
    """mean((hm - encode_heatmaps(target))^2) over every element, target never materialised."""

    @staticmethod
    def forward(ctx, hm, target, sigma):
        x = f32(hm).contiguous()
        t = f32(target).detach().contiguous()
        height, width = x.size(-2), x.size(-1)
        rows = x.numel() // (height * width)
        if t.numel() != rows * 2:
            raise RuntimeError('heatmap_mse_loss: target %s does not match heat-maps %s' % (tuple(t.shape), tuple(x.shape)))
        per_row = torch.empty(rows, device=x.device, dtype=torch.float32)
        call('dsnt_heatmap_mse_fwd', ptr(x), ptr(t), ptr(per_row), rows, height, width, float(sigma))
        ctx.save_for_backward(x, t)
        ctx.sigma = float(sigma)
        return per_row.sum() / x.numel()

    @staticmethod
    def backward(ctx, g):
        x, t = ctx.saved_tensors
        height, width = x.size(-2), x.size(-1)
        rows = x.numel() // (height * width)
        gs = g.to(torch.float32).reshape(1).contiguous()
        dx = torch.empty_like(x)
        call('dsnt_heatmap_mse_bwd', ptr(x), ptr(t), ptr(gs), ptr(dx), rows, height, width, ctx.sigma)
        return dx, None, None


def heatmap_mse_loss(heatmaps, target_coords, sigma=1):
    """`nn.functional.mse_loss(heatmaps, encode_heatmaps(target_coords, W, H, sigma))` (model.py:150-156)."""
    return _HeatmapMSE.apply(heatmaps, target_coords, sigma)
