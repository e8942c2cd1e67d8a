"""The device pose renderer on the MI355X (`render_pose_kernel`, csrc/render.hip, through dsnt.vis.render_pose and
heatmap_image) against the numpy restatement tests/render_ref.py.

Shapes: B = 3, J = 16, canvases 64 x 64 and 37 x 53 (H x W; 53 is no multiple of the 4-pixel group or the 64-pixel tile,
so rows start off a dword and end in a ragged group), heat-maps 16 x 16 and 5 x 7.

Two kinds of check.  Bit for bit: where the output is defined by fp32 steps rounded one by one (the un-normalised canvas,
an untouched uint8 canvas, the reference's heat-map picture).  Within one grey level of the restatement everywhere:
the device computes in fp32 what the restatement computes in fp64 and the output is truncated, so an error far below one
level (coordinates below 2^7 carry 2^-17 px, coverage and heat are ratios of such numbers) moves a byte by at most one.
"""
import numpy as np
import pytest
import torch

import golden_util
import render_ref

pytestmark = pytest.mark.gpu

B, J = 3, 16
CANVASES = {'64x64': (64, 64), '37x53': (37, 53)}
HEATMAPS = {'16x16': (16, 16), '5x7': (5, 7)}
MEAN, STD = (0.44, 0.45, 0.40), (0.25, 0.26, 0.27)
HEAT = {10: (1.0, 0.0, 0.0), 15: (0.0, 0.0, 1.0), 3: (0.3, 1.0, 0.6)}


def _bones():
    from dsnt import vis
    return vis.DEFAULT_BONES


def _rng(*key):
    return np.random.Generator(np.random.PCG64([77] + [int(k) for k in key]))


def _golden(name):
    g = golden_util.load('render')
    return g[name + '.coords'], g[name + '.mask']


def _model_input(H, W, seed):
    """f32 [B, 3, H, W] whose un-normalised values lie inside [0, 1) (so `unconvert`'s uint8 cast is defined)."""
    u = _rng(seed, H, W).random((B, 3, H, W))
    return ((u - np.array(MEAN)[None, :, None, None]) / np.array(STD)[None, :, None, None]).astype(np.float32)


def _u8_canvas(H, W, seed):
    return _rng(seed, H, W).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def _bumps(h, w, seed):
    """f32 [B, J, h, w]: one Gaussian bump per map, cut to exact zeros away from it, peaks of different heights."""
    r = _rng(seed, h, w)
    cx, cy = r.uniform(0, w, (B, J, 1, 1)), r.uniform(0, h, (B, J, 1, 1))
    xs, ys = np.arange(w)[None, None, None, :] + 0.5, np.arange(h)[None, None, :, None] + 0.5
    g = np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2 * (0.12 * max(h, w)) ** 2)) * r.uniform(0.01, 3.0, (B, J, 1, 1))
    return np.where(g > 0.2 * g.max(axis=(2, 3), keepdims=True), g, 0.0).astype(np.float32)


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _reference(base, coords=None, mask=None, heatmaps=None, peak=None, **kw):
    """(bytes [B, H, W, 3], touched [B, H, W]) of the restatement over a batch."""
    if heatmaps is not None and peak is None:
        peak = heatmaps.reshape(B, J, -1).max(2)
    out = [render_ref.render(base[b], None if coords is None else coords[b], None if mask is None else mask[b],
                             heatmaps=None if heatmaps is None else heatmaps[b], peak=None if peak is None else peak[b],
                             **kw) for b in range(B)]
    return np.stack([render_ref.to_bytes(v) for v, _ in out]), np.stack([t for _, t in out])


def _assert_one_level(got, want, what):
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape, (what, got.dtype, got.shape)
    diff = np.abs(got.cpu().numpy().astype(np.int32) - want.astype(np.int32))
    print('%s: max |byte difference| %d, differing bytes %d of %d' % (what, diff.max(), int((diff > 0).sum()), diff.size))
    assert diff.max() <= 1, (what, int(diff.max()), int((diff > 1).sum()))


# ------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize('name', CANVASES)
def test_model_input_canvas_is_unconverts_bytes(name):
    from dsnt import vis
    from dsnt.data import ImageSpecs

    class Stats:
        MEAN, STDDEV = MEAN, STD
    H, W = CANVASES[name]
    x = _model_input(H, W, 1)
    got = vis.render_pose(_cuda(x), mean=MEAN, std=STD)
    assert got.dtype == torch.uint8 and got.shape == (B, H, W, 3) and got.is_cuda
    specs = ImageSpecs(max(H, W), True, True)
    for b in range(B):
        want = np.asarray(specs.unconvert(torch.from_numpy(x[b]), Stats))
        assert np.array_equal(got[b].cpu().numpy(), want), (b, np.abs(got[b].cpu().numpy().astype(int) - want).max())
    # no normalisation given: x * 1 + 0; values beyond [0, 1] clamp, NaN is black
    y = x.copy()
    y[0, 0, 0, :3] = [np.nan, 7.0, -7.0]
    got = vis.render_pose(_cuda(y)).cpu().numpy()
    want = np.clip(np.nan_to_num(y, nan=0.0) * np.float32(255), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)
    assert np.array_equal(got, want) and got[0, 0, :3, 0].tolist() == [0, 255, 0]


@pytest.mark.parametrize('name', CANVASES)
def test_uint8_canvas_with_layers(name):
    """A uint8 canvas keeps its bytes wherever the restatement has zero coverage and zero heat, and is within one level
    of it everywhere; writing into the canvas itself gives the same picture."""
    from dsnt import vis
    H, W = CANVASES[name]
    canvas = _u8_canvas(H, W, 2)
    coords, mask = _golden(name)
    hm = _bumps(16, 16, 3)
    kw = dict(bones=_bones(), width=2.0, pixel_coords=True, heat_alpha=0.6)
    want, touched = _reference(canvas, coords, mask, heatmaps=hm, heat_colours=HEAT, **kw)
    dev = _cuda(canvas)
    got = vis.render_pose(dev, _cuda(coords), _cuda(mask), heatmaps=_cuda(hm), heat_colors=HEAT, **kw)
    assert torch.equal(dev.cpu(), torch.from_numpy(canvas))                   # the canvas is only read
    assert 0.1 < touched.mean() < 0.9                                         # both kinds of pixel are there
    assert np.array_equal(got.cpu().numpy()[~touched], canvas[~touched])
    _assert_one_level(got, want, 'uint8 canvas ' + name)
    again = vis.render_pose(dev, _cuda(coords), _cuda(mask), heatmaps=_cuda(hm), heat_colors=HEAT, out=dev, **kw)
    assert again.data_ptr() == dev.data_ptr() and torch.equal(again, got)


@pytest.mark.parametrize('size', HEATMAPS)
def test_heatmap_image_is_the_references_picture(size):
    from dsnt import vis
    h, w = HEATMAPS[size]
    logits = torch.from_numpy(_rng(4, h, w).normal(0, 3, (B, J, h * w)).astype(np.float32))
    hm = torch.softmax(logits, -1).view(B, J, h, w)
    got = vis.heatmap_image(hm.cuda())
    assert got.dtype == torch.uint8 and got.shape == (B, h, w, 3)
    for b in range(B):
        lw, rw = hm[b, 15], hm[b, 10]
        lw, rw = (lw / lw.max()).clamp(0, 1), (rw / rw.max()).clamp(0, 1)
        want = torch.stack([rw, torch.zeros_like(lw), lw]).mul(255).byte().permute(1, 2, 0)
        assert torch.equal(got[b].cpu(), want), (b, (got[b].cpu().int() - want.int()).abs().max().item())
    assert (got[..., 0].flatten(1).max(1).values == 255).all().item()       # the peak pixel is full red


# ------------------------------------------------------------------ within one grey level of the restatement
@pytest.mark.parametrize('width', [1.0, 2.0, 5.0])
@pytest.mark.parametrize('name', CANVASES)
def test_golden_skeletons(name, width):
    from dsnt import vis
    H, W = CANVASES[name]
    coords, mask = _golden(name)
    kw = dict(bones=_bones(), width=width, pixel_coords=True)
    want, touched = _reference(np.zeros((B, H, W, 3)), coords, mask, **kw)
    got = vis.render_pose((H, W), _cuda(coords), _cuda(mask), **kw)
    _assert_one_level(got, want, 'golden %s width %g' % (name, width))
    assert not got.cpu().numpy()[~touched].any() and want.any()
    # the default table is the reference's skeleton
    assert torch.equal(vis.render_pose((H, W), _cuda(coords), _cuda(mask), width=width, pixel_coords=True), got)


@pytest.mark.parametrize('name', CANVASES)
def test_skeleton_edge_cases(name):
    """Normalised coordinates with bones wholly and partly off the canvas, a zero-length bone, a NaN and an infinite
    joint, masked joints, and joint discs, over a model-input canvas."""
    from dsnt import vis
    H, W = CANVASES[name]
    r = _rng(5, H, W)
    coords = r.uniform(-0.95, 0.95, (B, J, 2)).astype(np.float32)
    coords[:, 0] = [-1.6, 0.2]            # right_lower_leg: partly off the canvas
    coords[:, 4] = [1.3, -1.4]            # left_lower_leg, left_upper_leg: partly off
    coords[:, 13] = [0.3, 2.5]
    coords[:, 14] = [1.8, 2.2]            # left_upper_arm: wholly off, left_lower_arm: partly
    coords[:, 11] = coords[:, 10]         # right_lower_arm: no length
    coords[0, 7, 0] = np.nan              # both torso bones of sample 0 skipped
    coords[1, 9, 1] = np.inf
    mask = (r.random((B, J)) >= 0.3).astype(np.float32)
    mask[2, 7] = 0.0
    x = _model_input(H, W, 6)
    base = np.stack([render_ref.canvas_f32(x[b], MEAN, STD) for b in range(B)])
    for radius in (0.0, 2.5):
        kw = dict(bones=_bones(), width=2.0, joint_radius=radius)
        want, _ = _reference(base, coords, mask, **kw)
        got = vis.render_pose(_cuda(x), _cuda(coords), _cuda(mask), mean=MEAN, std=STD, **kw)
        _assert_one_level(got, want, 'edge cases %s radius %g' % (name, radius))
    # without a mask nothing is grey: another picture, same bar
    want_nomask, _ = _reference(base, coords, None, **kw)
    assert (want_nomask != want).any()
    _assert_one_level(vis.render_pose(_cuda(x), _cuda(coords), mean=MEAN, std=STD, **kw), want_nomask, 'no mask ' + name)


@pytest.mark.parametrize('size', HEATMAPS)
@pytest.mark.parametrize('name', CANVASES)
def test_upsampled_heatmaps_under_a_skeleton(name, size):
    from dsnt import vis
    H, W = CANVASES[name]
    h, w = HEATMAPS[size]
    coords, mask = _golden(name)
    hm = _bumps(h, w, 7)
    x = _model_input(H, W, 8)
    base = np.stack([render_ref.canvas_f32(x[b], MEAN, STD) for b in range(B)])
    kw = dict(bones=_bones(), width=2.0, pixel_coords=True, heat_alpha=0.6)
    want, _ = _reference(base, coords, mask, heatmaps=hm, heat_colours=HEAT, **kw)
    got = vis.render_pose(_cuda(x), _cuda(coords), _cuda(mask), mean=MEAN, std=STD, heatmaps=_cuda(hm), heat_colors=HEAT, **kw)
    _assert_one_level(got, want, 'heat %s onto %s' % (size, name))
    # heat-maps alone, on black, named joints
    want, _ = _reference(np.zeros((B, H, W, 3)), heatmaps=hm, heat_colours={10: (1, 0, 0), 15: (0, 0, 1)}, heat_alpha=0.6)
    got = vis.render_pose((H, W), heatmaps=_cuda(hm), heat_alpha=0.6)
    _assert_one_level(got, want, 'heat alone %s onto %s' % (size, name))


def test_dead_peaks_give_no_heat():
    """A peak of 0, a negative, a NaN and an infinite peak: that joint adds nothing; the others are scaled by the peak
    that is passed, whatever the map holds."""
    from dsnt import vis
    H, W = CANVASES['37x53']
    hm = _bumps(5, 7, 9)
    peak = hm.reshape(B, J, -1).max(2)
    peak[0, 10], peak[1, 10], peak[2, 10], peak[0, 15] = 0.0, np.nan, np.inf, -1.0
    peak[1, 15] *= 2.0
    hm[0, 10] = 0.0                        # an all-zero map, whose peak really is 0
    canvas = _u8_canvas(H, W, 10)
    want, touched = _reference(canvas, heatmaps=hm, peak=peak, heat_colours={10: (1, 0, 0), 15: (0, 0, 1)})
    got = vis.render_pose(_cuda(canvas), heatmaps=_cuda(hm), peak=_cuda(peak))
    _assert_one_level(got, want, 'dead peaks')
    assert not touched[0].any() and np.array_equal(got[0].cpu().numpy(), canvas[0])
    assert (got.cpu().numpy()[2, :, :, 0] == canvas[2, :, :, 0]).all()       # red (joint 10) dead in sample 2
    # computed inside, the peak of the all-zero map is 0 and the others are the maxima
    want, _ = _reference(canvas, heatmaps=hm, heat_colours={10: (1, 0, 0), 15: (0, 0, 1)})
    _assert_one_level(vis.render_pose(_cuda(canvas), heatmaps=_cuda(hm)), want, 'peak computed inside')


def test_custom_table_of_32_bones():
    from dsnt import vis
    H, W = CANVASES['37x53']
    r = _rng(11)
    bones = [(int(a), int(b), tuple(int(c) for c in r.integers(0, 256, 3))) for a, b in r.integers(0, J, (32, 2))]
    coords = r.uniform(-1, 1, (B, J, 2)).astype(np.float32)
    canvas = _u8_canvas(H, W, 12)
    for kw in (dict(width=3.0), dict(width=1.5, joint_radius=1.0)):
        want, _ = _reference(canvas, coords, None, bones=bones, **kw)
        _assert_one_level(vis.render_pose(_cuda(canvas), _cuda(coords), bones=bones, **kw), want, '32 bones %r' % (kw,))
    with pytest.raises(RuntimeError, match='at most 32 bones'):
        vis.render_pose(_cuda(canvas), _cuda(coords), bones=bones + bones[:1])


# ------------------------------------------------------------------ in the prediction chain
def test_peak_from_predict_equals_peak_computed_inside():
    from dsnt import inference, synthetic, vis
    from dsnt.model import build_mpii_pose_model
    model = build_mpii_pose_model(base='hg1', output_strat='dsnt', reg='js')
    synthetic.fill_state_dict(model, seed=0)
    model.cuda().eval()
    x, _, _ = synthetic.batch(B, size=64, seed=3, mask_p=1.0)
    x = x.cuda()
    tm = torch.eye(2, dtype=torch.float64).repeat(B, 1, 1).cuda()
    tb = torch.zeros(B, 1, 2, dtype=torch.float64).cuda()
    _, coords, stats = inference.predict(model, x, tm, tb, return_normalized=True, return_stats=True)
    hm = model.heatmaps
    assert hm.shape == (B, J, 16, 16) and stats['peak'].shape == (B, J)
    kw = dict(mean=synthetic.IMAGE_MEAN, std=(0.25, 0.26, 0.27), heatmaps=hm, heat_alpha=0.6, joint_radius=1.5)
    passed = vis.render_pose(x, coords, peak=stats['peak'], **kw)
    inside = vis.render_pose(x, coords, **kw)
    assert torch.equal(passed, inside)
    assert torch.equal(vis.render_pose(x, coords, peak=stats['peak'].contiguous(), **kw), inside)
    assert (passed != vis.render_pose(x, mean=kw['mean'], std=kw['std'])).any().item()       # the layers are there


def test_render_enqueues_on_the_current_stream_without_a_copy_or_a_synchronisation():
    from dsnt import vis
    H, W = CANVASES['37x53']
    coords, mask = _golden('37x53')
    hm = _bumps(5, 7, 13)
    dev = [_cuda(a) for a in (_u8_canvas(H, W, 14), coords, mask, hm)]
    peak = dev[3].flatten(2).max(2).values
    kw = dict(pixel_coords=True, heatmaps=dev[3], peak=peak, heat_alpha=0.6, joint_radius=2.0)
    first = vis.render_pose(dev[0], dev[1], dev[2], **kw)
    vis.render_pose(dev[0], dev[1], dev[2], pixel_coords=True, heatmaps=dev[3])        # first call of heatmap_stats too
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        second = vis.render_pose(dev[0], dev[1], dev[2], **kw)
        third = vis.render_pose(dev[0], dev[1], dev[2], pixel_coords=True, heatmaps=dev[3], heat_alpha=0.6, joint_radius=2.0)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(second, first) and torch.equal(third, first)
    # on a side stream the launch is ordered behind that stream's work: it sees the canvas a long chain there fills last
    side = torch.cuda.Stream()
    canvas = torch.zeros_like(dev[0])
    busy = torch.zeros(1 << 26, device='cuda')
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(10):
            busy.add_(1.0)
        canvas.copy_(dev[0])
        got = vis.render_pose(canvas, dev[1], dev[2], **kw)
    side.synchronize()
    assert torch.equal(got, first)
