"""numpy restatement of dsnt_render_pose (csrc/render.hip; formulas in DESIGN.md section 15), one sample at a time.

fp64 throughout, except the model-input canvas, whose steps are the fp32 ones of `ImageSpecs.unconvert`
(`x * std + mean`, `* 255`, clamp, each rounded).  `render` returns the picture before truncation, so a caller can see
how far a value is from a byte boundary; `to_bytes` is the output rule.
"""
import numpy as np

GREY = (100.0, 100.0, 100.0)


def canvas_f32(x, mean=None, std=None):
    """Base values [H, W, 3] (fp32) of a model input x f32 [3, H, W]."""
    x = np.asarray(x, np.float32)
    mean = np.zeros(3, np.float32) if mean is None else np.asarray(mean, np.float32)
    std = np.ones(3, np.float32) if std is None else np.asarray(std, np.float32)
    un = (x * std[:, None, None]).astype(np.float32) + mean[:, None, None]
    v = un.astype(np.float32) * np.float32(255)
    v = np.where(np.isnan(v), np.float32(0), np.clip(v, 0, 255))
    return np.ascontiguousarray(v.astype(np.float32).transpose(1, 2, 0))


def to_bytes(value):
    """clamp to [0, 255] and truncate toward zero."""
    return np.clip(value, 0, 255).astype(np.uint8)


def pixels(coords, H, W, pixel_coords=False):
    """coords [J, 2] in continuous pixel units (pixel i spans [i, i + 1))."""
    c = np.asarray(coords, np.float64)
    if pixel_coords:
        return c.copy()
    return np.stack([(c[:, 0] + 1) * W / 2, (c[:, 1] + 1) * H / 2], 1)


def segment_distance(H, W, p1, p2):
    """[H, W]: distance of every pixel centre to the segment p1-p2 (a point when they coincide)."""
    cx = np.arange(W, dtype=np.float64)[None, :] + 0.5
    cy = np.arange(H, dtype=np.float64)[:, None] + 0.5
    ex, ey = p2[0] - p1[0], p2[1] - p1[1]
    ee = ex * ex + ey * ey
    qx, qy = cx - p1[0], cy - p1[1]
    t = np.clip((qx * ex + qy * ey) / ee, 0, 1) if ee > 0 else np.zeros((H, W))
    return np.hypot(qx - t * ex, qy - t * ey)


def coverage(H, W, p1, p2, reach):
    return np.clip(reach - segment_distance(H, W, p1, p2), 0, 1)


def bone_layers(H, W, px, mask, bones, width, joint_radius=0.0):
    """The skeleton as a list of (coverage [H, W], rgb) in drawing order: bones in table order, then discs in joint order."""
    layers = []
    finite = np.isfinite(px).all(1)
    masked = np.zeros(len(px), bool) if mask is None else (np.asarray(mask) == 0)
    for j1, j2, rgb in bones:
        if finite[j1] and finite[j2]:
            colour = GREY if (masked[j1] or masked[j2]) else tuple(float(c) for c in rgb)
            layers.append((coverage(H, W, px[j1], px[j2], width / 2 + 0.5), colour))
    if joint_radius > 0:
        for j in range(len(px)):
            named = [rgb for j1, j2, rgb in bones if j in (j1, j2)]
            if finite[j] and named:
                colour = GREY if masked[j] else tuple(float(c) for c in named[0])
                layers.append((coverage(H, W, px[j], px[j], joint_radius + 0.5), colour))
    return layers


def bilinear(hm, H, W):
    """hm [h, w] sampled at the H x W pixel centres: src = (dst + 0.5) * h / H - 0.5, edge-clamped."""
    hm = np.asarray(hm, np.float64)
    h, w = hm.shape
    if (h, w) == (H, W):
        return hm.copy()
    sy = np.clip((np.arange(H) + 0.5) * h / H - 0.5, 0, h - 1)
    sx = np.clip((np.arange(W) + 0.5) * w / W - 0.5, 0, w - 1)
    ya, xa = np.floor(sy).astype(int), np.floor(sx).astype(int)
    yb, xb = np.minimum(ya + 1, h - 1), np.minimum(xa + 1, w - 1)
    fy, fx = (sy - ya)[:, None], (sx - xa)[None, :]
    top = hm[ya][:, xa] * (1 - fx) + hm[ya][:, xb] * fx
    bot = hm[yb][:, xa] * (1 - fx) + hm[yb][:, xb] * fx
    return top * (1 - fy) + bot * fy


def heat(heatmaps, peak, colours, H, W):
    """heat_c [H, W, 3] = clamp(sum_j v_j colour_jc, 0, 1) over the joints of `colours` ({index: rgb in [0, 1]})."""
    total = np.zeros((H, W, 3))
    for j in sorted(colours):
        rgb = np.asarray(colours[j], np.float64)
        if not rgb.any():
            continue
        pk = float(peak[j])
        if not (np.isfinite(pk) and pk > 0):
            continue
        with np.errstate(invalid='ignore', over='ignore'):
            v = bilinear(heatmaps[j], H, W) / pk
        v = np.where(np.isnan(v), 0.0, np.clip(v, 0, 1))
        total += v[:, :, None] * rgb
    return np.clip(total, 0, 1)


def render(base, coords=None, mask=None, bones=(), width=2.0, joint_radius=0.0, pixel_coords=False, heatmaps=None,
           peak=None, heat_colours=None, heat_alpha=1.0):
    """(value [H, W, 3] fp64 before truncation, touched [H, W] bool) of one sample.  `base` [H, W, 3] holds the canvas
    values (zeros for black, the bytes of a uint8 canvas, `canvas_f32` of a model input); `touched` marks the pixels
    where a layer has positive coverage or heat."""
    value = np.asarray(base, np.float64).copy()
    H, W = value.shape[:2]
    touched = np.zeros((H, W), bool)
    if heatmaps is not None:
        hc = heat(heatmaps, peak, heat_colours, H, W)
        value = value + (255 - value) * (heat_alpha * hc)
        touched |= (heat_alpha * hc).any(2)
    if coords is not None:
        for cov, rgb in bone_layers(H, W, pixels(coords, H, W, pixel_coords), mask, bones, width, joint_radius):
            value = value * (1 - cov[:, :, None]) + np.asarray(rgb)[None, None, :] * cov[:, :, None]
            touched |= cov > 0
    return value, touched
