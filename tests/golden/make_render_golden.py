"""Golden skeletons of the reference's `util.draw_skeleton` (Pillow's one-pixel lines), for dsnt.util.draw_skeleton and
the restatement of dsnt_render_pose (tests/render_ref.py).

    python tests/golden/make_render_golden.py        # writes tests/golden/render.npz

The reference's function is loaded through tests/refimport.py and paints black canvases of 64 x 64 and 37 x 53
(H x W) with Pillow (12.2 here), three samples each.  Joints are PCG64 draws in continuous pixel units; per sample two
joints lie off the canvas, two coincide, and about a quarter are masked out.  Stored: the coordinates f32 [3, 16, 2],
the masks f32 [3, 16] and the painted images uint8 [3, H, W, 3] of both canvases — data only.

Pillow truncates a coordinate to its pixel and walks a Bresenham line between the two pixels, so a painted pixel's
centre lies off the exact segment by up to the truncation plus half a step.  Worst distance over this fixture, from the
centre of a painted pixel to the nearest segment of its colour class (pixel i spans [i, i + 1)): 0.93 px.  A
restatement `width` of 3 has positive coverage below 2.0 px, so it covers every painted pixel (tests/test_render_cpu.py).
"""
import os
import sys

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), 'dsnt-pose2d_amd')]

import refimport  # noqa: E402
import render_ref  # noqa: E402

CANVASES = {'64x64': (64, 64), '37x53': (37, 53)}       # (H, W)
B, J = 3, 16


def case(name):
    H, W = CANVASES[name]
    r = np.random.Generator(np.random.PCG64([41, H, W]))
    coords = r.uniform(1.0, [W - 1.0, H - 1.0], (B, J, 2))
    mask = (r.random((B, J)) >= 0.25).astype(np.float32)
    for b in range(B):
        off = r.choice(J, 2, replace=False)
        coords[b, off[0]] = [-r.uniform(3, 15), r.uniform(0, H)]                 # left of the canvas
        coords[b, off[1]] = [r.uniform(0, W), H + r.uniform(3, 15)]              # below it
        coords[b, 11] = coords[b, 10]                                            # right_lower_arm has no length
    return coords.astype(np.float32), mask


def worst_distance(ref_util, coords, mask, img):
    """Largest distance from a painted pixel centre to the nearest segment of its colour (render_ref's convention)."""
    from dsnt.util import bone_colour
    H, W = img.shape[:2]
    px = coords.astype(np.float64)
    worst = 0.0
    for colour in {tuple(c) for c in img.reshape(-1, 3).tolist()} - {(0, 0, 0)}:
        near = np.full((H, W), np.inf)
        for name, (j1, j2) in ref_util.BONES.items():
            masked = mask[j1] == 0 or mask[j2] == 0
            if ((100, 100, 100) if masked else bone_colour(name)) == colour:
                near = np.minimum(near, render_ref.segment_distance(H, W, px[j1], px[j2]))
        worst = max(worst, float(near[(img == np.array(colour, np.uint8)).all(2)].max()))
    return worst


def main():
    ref_util = refimport.load_reference_module('dsnt.util')
    assert ref_util is not None, 'the reference is not on this machine'
    out, worst = {'names': np.array(sorted(CANVASES))}, 0.0
    for name, (H, W) in CANVASES.items():
        coords, mask = case(name)
        imgs = []
        for b in range(B):
            img = Image.new('RGB', (W, H))
            ref_util.draw_skeleton(img, torch.from_numpy(coords[b]), torch.from_numpy(mask[b]))
            imgs.append(np.asarray(img).copy())
            worst = max(worst, worst_distance(ref_util, coords[b], mask[b], imgs[-1]))
        out[name + '.coords'], out[name + '.mask'], out[name + '.image'] = coords, mask, np.stack(imgs)
    path = os.path.join(HERE, 'render.npz')
    np.savez_compressed(path, **out)
    print('%s: %d bytes, worst painted-pixel distance %.2f px' % (path, os.path.getsize(path), worst))


if __name__ == '__main__':
    main()
