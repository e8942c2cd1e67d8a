"""CPU checks of the device pose renderer (dsnt_render_pose, dsnt.vis, dsnt.util.draw_skeleton): the numpy restatement
(tests/render_ref.py) against the reference's Pillow skeletons and against answers worked out by hand, the argument
checks of the entry point (they run before anything is launched), and the host side of dsnt.vis and dsnt.util."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_util
import render_ref

CANVASES = ('64x64', '37x53')
RED, BLUE, MAGENTA = (255, 0, 0), (0, 0, 255), (255, 0, 255)


def _default_bones():
    from dsnt import vis
    return vis.DEFAULT_BONES


# ------------------------------------------------------------------ (a) the restatement against the reference
@pytest.mark.parametrize('name', CANVASES)
def test_restatement_covers_every_pixel_pillow_paints(name):
    """Every pixel the reference's draw_skeleton paints in a colour has positive coverage, at width 3, from a bone of
    that colour class in the restatement.  No pixel is exempt (the generator's docstring has the measured margin)."""
    g = golden_util.load('render')
    coords, mask, image = g[name + '.coords'], g[name + '.mask'], g[name + '.image']
    bones = _default_bones()
    painted = 0
    for b in range(len(image)):
        H, W = image[b].shape[:2]
        px = render_ref.pixels(coords[b], H, W, pixel_coords=True)
        by_colour = {}
        for cov, rgb in render_ref.bone_layers(H, W, px, mask[b], bones, width=3.0):
            by_colour[rgb] = np.maximum(by_colour.get(rgb, 0.0), cov)
        colours = {tuple(float(v) for v in c) for c in image[b].reshape(-1, 3).tolist()} - {(0.0, 0.0, 0.0)}
        assert colours <= set(by_colour), (colours, set(by_colour))
        assert (100.0, 100.0, 100.0) in colours                        # the fixture has masked bones
        for colour in colours:
            where = (image[b] == np.array(colour, np.uint8)).all(2)
            painted += int(where.sum())
            assert (by_colour[colour][where] > 0).all(), (b, colour, int((by_colour[colour][where] <= 0).sum()))
    assert painted > 300


# ------------------------------------------------------------------ (b) known answers of the restatement
def test_horizontal_bone_through_pixel_centres():
    base = np.zeros((7, 12, 3))
    coords = np.array([[2.5, 3.5], [9.5, 3.5]])
    value, touched = render_ref.render(base, coords, bones=[(0, 1, RED)], width=2.0, pixel_coords=True)
    assert (value[3, 2:10, 0] == 255).all() and (value[2, 2:10, 0] == 127.5).all() and (value[4, 2:10, 0] == 127.5).all()
    assert (value[1, :, :] == 0).all() and (value[5, :, :] == 0).all() and (value[:, :, 1:] == 0).all()
    # the caps: the end pixel's neighbour is 1 px away (coverage 0.5), the next one 2 px (none)
    assert value[3, 1, 0] == 127.5 and value[3, 0, 0] == 0 and value[3, 10, 0] == 127.5 and value[3, 11, 0] == 0
    assert touched[2:5, 2:10].all() and not touched[0].any() and not touched[6].any()
    assert (render_ref.to_bytes(value)[2, 2:10] == np.array([127, 0, 0], np.uint8)).all()
    # normalised coordinates map to the same pixels: u = (x + 1) W / 2
    norm = np.stack([coords[:, 0] * 2 / 12 - 1, coords[:, 1] * 2 / 7 - 1], 1)
    again, _ = render_ref.render(base, norm, bones=[(0, 1, RED)], width=2.0)
    assert np.abs(again - value).max() < 1e-9


def test_masked_end_is_grey_and_nan_joint_draws_nothing():
    base = np.full((5, 8, 3), 10.0)
    coords = np.array([[1.5, 2.5], [6.5, 2.5], [np.nan, 1.0]])
    value, _ = render_ref.render(base, coords, mask=np.array([1.0, 0.0, 1.0]), bones=[(0, 1, RED)], pixel_coords=True)
    assert (value[2, 1:7] == 100).all()
    value, touched = render_ref.render(base, coords, bones=[(0, 2, RED), (2, 2, BLUE)], joint_radius=2.0, pixel_coords=True)
    assert (value[:, 4:] == 10).all() and not touched[:, 4:].any()          # only joint 0's disc, no bone
    assert tuple(value[2, 1]) == (255, 0, 0) and touched[2, 1]              # in the red of the first bone that names it


def test_table_order_decides_overlaps():
    base = np.zeros((9, 9, 3))
    coords = np.array([[1.5, 4.5], [7.5, 4.5], [4.5, 1.5], [4.5, 7.5]])
    first, _ = render_ref.render(base, coords, bones=[(0, 1, RED), (2, 3, BLUE)], pixel_coords=True)
    second, _ = render_ref.render(base, coords, bones=[(2, 3, BLUE), (0, 1, RED)], pixel_coords=True)
    assert tuple(first[4, 4]) == (0, 0, 255) and tuple(second[4, 4]) == (255, 0, 0)
    assert tuple(first[4, 2]) == (255, 0, 0) and tuple(first[2, 4]) == (0, 0, 255)
    # where the later bone covers half, the earlier one shows through by half
    assert tuple(first[4, 3]) == (127.5, 0, 127.5)
    # a zero-length bone is a point
    dot, _ = render_ref.render(base, coords, bones=[(0, 0, MAGENTA)], width=1.0, pixel_coords=True)
    assert tuple(dot[4, 1]) == (255, 0, 255) and dot.sum() == 2 * 255


def test_bilinear_2x2_to_4x4_by_hand():
    hm = np.array([[0.0, 4.0], [8.0, 12.0]])
    # src = (dst + 0.5) / 2 - 0.5 = -0.25, 0.25, 0.75, 1.25 -> clamped to 0, 0.25, 0.75, 1
    f = np.array([0.0, 0.25, 0.75, 1.0])
    want = (hm[0, 0] * (1 - f)[None, :] + hm[0, 1] * f[None, :]) * (1 - f)[:, None] + \
        (hm[1, 0] * (1 - f)[None, :] + hm[1, 1] * f[None, :]) * f[:, None]
    got = render_ref.bilinear(hm, 4, 4)
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], [0, 1, 3, 4]) and np.array_equal(got[:, 0], [0, 2, 6, 8]) and got[1, 1] == 3
    assert np.array_equal(render_ref.bilinear(hm, 2, 2), hm)
    # the heat layer on black: 255 * clamp(v) * colour, v = sample / peak; a dead peak gives no heat
    value, _ = render_ref.render(np.zeros((4, 4, 3)), heatmaps=hm[None], peak=[12.0], heat_colours={0: (1.0, 0.0, 0.5)})
    assert np.allclose(value[:, :, 0], 255 * want / 12) and np.allclose(value[:, :, 2], 127.5 * want / 12)
    for dead in (0.0, -1.0, np.nan, np.inf):
        value, touched = render_ref.render(np.full((4, 4, 3), 7.0), heatmaps=hm[None], peak=[dead], heat_colours={0: (1, 0, 0)})
        assert (value == 7).all() and not touched.any()
    # value = base + (255 - base) * alpha * heat
    value, _ = render_ref.render(np.full((2, 2, 3), 55.0), heatmaps=hm[None], peak=[12.0], heat_colours={0: (1, 1, 1)},
                                 heat_alpha=0.5)
    assert np.allclose(value[1, 1], 55 + 200 * 0.5) and np.allclose(value[0, 0], 55)


def test_model_input_canvas_is_unconverts_bytes():
    from dsnt.data import ImageSpecs
    from dsnt import synthetic

    class Stats:
        MEAN, STDDEV = synthetic.IMAGE_MEAN, (0.25, 0.26, 0.27)
    r = np.random.default_rng(0)
    x = ((r.random((3, 9, 11)) - np.array(Stats.MEAN)[:, None, None]) / np.array(Stats.STDDEV)[:, None, None]).astype(np.float32)
    want = np.asarray(ImageSpecs(9, True, True).unconvert(torch.from_numpy(x), Stats))
    assert np.array_equal(render_ref.to_bytes(render_ref.canvas_f32(x, Stats.MEAN, Stats.STDDEV)), want)


# ------------------------------------------------------------------ (c) the entry point, dsnt.vis and dsnt.util
def _call(**kw):
    """dsnt_render_pose with every pointer a plausible non-null address and every size valid, except `kw`."""
    from dsnt import _lib
    lib = _lib.load()
    dev = C.c_void_p(1 << 20)                      # never dereferenced: a failed check launches nothing
    a = dict(canvas=dev, kind=1, mean=(C.c_float * 3)(0, 0, 0), stdv=(C.c_float * 3)(1, 1, 1), B=2, H=8, W=8, J=16,
             heatmaps=dev, h=4, w=4, peak=dev, peak_stride=1, heat_rgb=(C.c_float * 48)(*([1.0] * 48)), heat_alpha=1.0,
             coords=dev, mask=dev, pixel_coords=0, bone_joints=(C.c_int32 * 4)(0, 1, 1, 2),
             bone_rgb=(C.c_float * 6)(*([255.0] * 6)), nbones=2, width=2.0, joint_radius=0.0, out=dev)
    assert set(kw) <= set(a)
    a.update(kw)
    rc = lib.dsnt_render_pose(*a.values(), None)
    return rc, lib.dsnt_last_error().decode()


def test_abi_is_declared_and_bound():
    from dsnt import _lib
    lib = _lib.load()
    assert lib.dsnt_version() >= 123
    assert hasattr(lib, 'dsnt_render_pose') and len(_lib.SIGNATURES['dsnt_render_pose']) == 25


@pytest.mark.parametrize('kw', [dict(out=None), dict(peak=None), dict(coords=None), dict(heat_rgb=None),
                                dict(bone_joints=None), dict(canvas=None)])
def test_null_pointers_are_code_3(kw):
    rc, msg = _call(**kw)
    assert rc == 3 and 'dsnt_render_pose' in msg and 'null' in msg, (rc, msg)


@pytest.mark.parametrize('kw', [dict(H=0), dict(W=0), dict(h=0), dict(w=-1), dict(J=0), dict(J=65), dict(nbones=33),
                                dict(bone_joints=(C.c_int32 * 4)(0, 1, 1, 16)), dict(bone_joints=(C.c_int32 * 4)(-1, 1, 1, 2)),
                                dict(width=0.0), dict(width=-1.0), dict(width=float('nan')), dict(kind=3), dict(kind=-1)])
def test_bad_shapes_are_code_1(kw):
    rc, msg = _call(**kw)
    assert rc == 1 and 'dsnt_render_pose' in msg, (rc, msg)


def test_absent_layers_need_none_of_their_arguments():
    """Without heat-maps or bones their other arguments are not looked at: the call passes every check and records."""
    from dsnt import _lib
    lib = _lib.load()
    lst = lib.dsnt_list_create()
    assert lib.dsnt_list_begin(lst) == 0
    try:
        rc, msg = _call(heatmaps=None, peak=None, heat_rgb=None, h=0, w=0, nbones=0, coords=None, bone_joints=None,
                        bone_rgb=None, width=0.0, J=0, kind=0, canvas=None, mean=None, stdv=None)
        assert rc == 0, msg
        assert lib.dsnt_list_size(lst) == 1          # recorded by the launch list, nothing launched
        assert _call(out=None)[0] == 3 and lib.dsnt_list_size(lst) == 1
    finally:
        lib.dsnt_list_end()
        lib.dsnt_list_destroy(lst)


def test_vis_refuses_cpu_tensors():
    from dsnt import vis
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        vis.render_pose(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        vis.render_pose(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 16, 2))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        vis.render_pose((8, 8), torch.zeros(1, 16, 2))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        vis.heatmap_image(torch.zeros(1, 16, 8, 8))


def test_vis_refuses_options_that_would_do_nothing():
    from dsnt import vis
    with pytest.raises(RuntimeError, match='mean and std'):
        vis.render_pose(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), mean=(0.5, 0.5, 0.5))
    with pytest.raises(RuntimeError, match='mean and std'):
        vis.render_pose((8, 8), torch.zeros(1, 16, 2), std=(0.5, 0.5, 0.5))
    for width in (0.0, -1.0, float('nan')):
        with pytest.raises(RuntimeError, match='width > 0'):
            vis.render_pose((8, 8), heatmaps=torch.zeros(1, 16, 8, 8), width=width)
    with pytest.raises(RuntimeError, match='empty bone table'):
        vis._bone_table([], 16)


def test_bone_table_is_checked_on_the_host():
    from dsnt import util, vis
    assert len(vis.DEFAULT_BONES) == 15 and [b[:2] for b in vis.DEFAULT_BONES] == list(util.BONES.values())
    assert {b[2] for b in vis.DEFAULT_BONES} == {RED, BLUE, MAGENTA}
    assert vis.DEFAULT_BONES[0] == (0, 1, RED) and vis.DEFAULT_BONES[3] == (4, 5, BLUE) and vis.DEFAULT_BONES[6] == (6, 7, MAGENTA)
    joints, rgb, n = vis._bone_table(None, 16)
    assert n == 15 and list(joints)[:4] == [0, 1, 1, 2] and list(rgb)[:3] == [255.0, 0.0, 0.0]
    with pytest.raises(RuntimeError, match='outside 0..15'):
        vis._bone_table([(0, 16, RED)], 16)
    with pytest.raises(RuntimeError, match='outside 0..3'):
        vis._bone_table(None, 4)
    with pytest.raises(RuntimeError, match='at most 32 bones'):
        vis._bone_table([(0, 1, RED)] * 33, 16)
    with pytest.raises(RuntimeError, match=r'\(j1, j2, \(r, g, b\)\)'):
        vis._bone_table([(0, 1)], 16)
    table = vis._heat_table(None, 16)
    assert list(table)[30:33] == [1.0, 0.0, 0.0] and list(table)[45:48] == [0.0, 0.0, 1.0] and sum(table) == 2.0
    assert list(vis._heat_table({3: (0.5, 0.25, 1.0)}, 4))[9:] == [0.5, 0.25, 1.0]
    with pytest.raises(RuntimeError, match='unknown joint'):
        vis._heat_table({'elbow': RED}, 16)
    with pytest.raises(RuntimeError, match=r'in \[0, 1\]'):
        vis._heat_table({0: RED}, 16)


@pytest.mark.parametrize('name', CANVASES)
def test_draw_skeleton_paints_the_golden_images(name):
    from PIL import Image
    from dsnt import util
    g = golden_util.load('render')
    coords, mask, image = g[name + '.coords'], g[name + '.mask'], g[name + '.image']
    for b in range(len(image)):
        H, W = image[b].shape[:2]
        img = Image.new('RGB', (W, H))
        util.draw_skeleton(img, torch.from_numpy(coords[b]), torch.from_numpy(mask[b]))
        assert np.array_equal(np.asarray(img), image[b]), b
    # without a mask no bone is grey
    img = Image.new('RGB', (W, H))
    util.draw_skeleton(img, coords[0])
    assert not (np.asarray(img) == 100).all(2).any() and np.asarray(img).any()
