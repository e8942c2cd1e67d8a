"""`dsnt_map_modes` on the device against the numpy restatement (tests/modes_ref.py): `index`, `mass` and `coords` bit for
bit.  No margin applies: the window scores are separately rounded fp32 adds in a fixed order, the choice of a mode is a
comparison of those, and the window sums are fp64 operations in a fixed order, all of which the restatement repeats.
`image` is held to `tb + coords.double() @ tm` in ATen within 8 x 2^-53 (|tb| + |c_x M| + |c_y M|) per component: three
roundings each side of terms no larger than that sum."""
import ctypes as C

import numpy as np
import pytest
import torch

import modes_ref as ref

pytestmark = pytest.mark.gpu


def _np(out):
    """The dict of `heatmap_modes` as numpy arrays over flat rows: [n, K, ...]."""
    K = out['index'].shape[-1]
    return {k: v.cpu().numpy().reshape(-1, K, *v.shape[out['index'].dim():]) for k, v in out.items()}


def _same_bits(got, want):
    """Equal bit for bit (signed zeros told apart); a NaN only against a NaN."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind != 'f':
        return np.array_equal(got, want)
    bits = {4: np.int32, 8: np.int64}[got.dtype.itemsize]
    nan = np.isnan(got)
    return np.array_equal(nan, np.isnan(want)) and np.array_equal(got.view(bits)[~nan], want.view(bits)[~nan])


def _check(got, want, K, what):
    for k in ('index', 'mass', 'coords'):
        g, w = got[k], np.ascontiguousarray(want[k][:, :K])
        assert _same_bits(g, w), (what, k, np.argwhere(~((g == w) | ((g != g) & (w != w))))[:4].tolist())


def _device_maps(h, w):
    return torch.from_numpy(ref.seeded_maps(h, w).copy()).cuda().view(ref.N_ROWS // 16, 16, h, w)


def _device_transforms():
    tm, tb = ref.seeded_transforms()
    return torch.from_numpy(tm.copy()).cuda(), torch.from_numpy(tb.copy()).cuda()


def _image_ok(out, tm, tb):
    B = tm.size(0)
    c = out['coords'].double()
    M = tm.view(B, 1, 1, 2, 2)
    want = tb.view(B, 1, 1, 2) + (c.unsqueeze(-2) @ M).squeeze(-2)
    bar = 8 * 2.0 ** -53 * (tb.view(B, 1, 1, 2).abs() + (c[..., 0:1] * M[..., 0, :]).abs() + (c[..., 1:2] * M[..., 1, :]).abs())
    nan = torch.isnan(c).any(-1, keepdim=True).expand_as(want)
    got = out['image']
    assert torch.equal(torch.isnan(got), nan) and torch.equal(torch.isnan(want), nan)
    assert ((got - want).abs() <= bar)[~nan].all().item(), ((got - want).abs() / bar)[~nan].max().item()


# ------------------------------------------------------------------ the seeded maps of every shape, radius and count
@pytest.mark.parametrize('r', ref.RADII)
@pytest.mark.parametrize('h,w', ref.SHAPES)
def test_map_modes_bit_equal_to_the_restatement(h, w, r):
    import dsnt.nn as dn
    hm = _device_maps(h, w)
    tm, tb = _device_transforms()
    want = ref.seeded_modes(h, w, r)
    for K in ref.COUNTS:
        out = dn.heatmap_modes(hm, r, K, tm, tb)
        assert out['coords'].shape == (3, 16, K, 2) and out['mass'].shape == out['index'].shape == (3, 16, K)
        assert out['index'].dtype == torch.int32 and out['image'].dtype == torch.float64
        got = _np(out)
        _check(got, want, K, (h, w, r, K))
        _image_ok(out, tm, tb)
        # the restatement's own image, formed as the kernel forms it: the same bits
        assert _same_bits(got['image'], np.ascontiguousarray(want['image'][:, :K]))
    again = _np(dn.heatmap_modes(hm, r, 4, tm, tb))              # two runs of the kernel agree bit for bit
    assert all(_same_bits(again[k], got[k]) for k in got)
    plain = dn.heatmap_modes(hm, r, 4)                            # without transforms: no image, the rest unchanged
    assert set(plain) == {'coords', 'mass', 'index'} and all(_same_bits(_np(plain)[k], got[k]) for k in plain)


@pytest.mark.parametrize('h,w', ref.SHAPES)
def test_one_row(h, w):
    """A grid of one workgroup, J = 1: the bimodal map of the shape alone."""
    import dsnt.nn as dn
    p = ref.seeded_maps(h, w)[24:25]
    got = _np(dn.heatmap_modes(torch.from_numpy(p.copy()).cuda().view(1, h, w), 1, 2))
    _check(got, ref.modes(p, 1, 2), 2, (h, w))


def test_more_rows_than_a_16_bit_grid():
    import dsnt.nn as dn
    n, h, w = 65537, 5, 9
    p = ref.softmax_maps(n, h, w, 3.0, np.random.RandomState(5))
    p[-1] = 0.0
    p[-1, 4, 8] = 1.0                                             # the last row is recognisable
    tm, tb = np.tile(np.eye(2) * 100.0, (n, 1, 1)), np.arange(2.0 * n).reshape(n, 2)
    out = dn.heatmap_modes(torch.from_numpy(p).cuda().view(n, 1, h, w), 1, 2, torch.from_numpy(tm).cuda(),
                           torch.from_numpy(tb).cuda())
    got, want = _np(out), ref.modes(p, 1, 2, 1, tm, tb)
    _check(got, want, 2, 'rows=65537')
    assert _same_bits(got['image'], want['image'])                # sample b = row / J with J = 1: every row its own offset
    assert got['index'][-1].tolist() == [3 * 9 + 7, 0]


# ------------------------------------------------------------------ loads: 16-byte and scalar place the same values
@pytest.mark.parametrize('h,w', [(16, 16), (64, 64), (64, 128)])
def test_unaligned_base_pointer_agrees_with_the_aligned_one(h, w):
    import dsnt.nn as dn
    hm = _device_maps(h, w)
    buf = torch.empty(hm.numel() + 1, device='cuda')
    off = buf[1:].view_as(hm)
    off.copy_(hm)
    assert hm.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4 and off.is_contiguous()
    a, b = _np(dn.heatmap_modes(hm, 3, 4)), _np(dn.heatmap_modes(off, 3, 4))
    assert all(_same_bits(a[k], b[k]) for k in a)
    _check(b, ref.seeded_modes(h, w, 3), 4, (h, w))


# ------------------------------------------------------------------ radius 0 is the peak pixel
@pytest.mark.parametrize('h,w', ref.SHAPES)
def test_radius_zero_is_the_peak_of_heatmap_stats(h, w):
    import dsnt.nn as dn
    p = ref.seeded_maps(h, w)
    clean = torch.from_numpy(p[~np.isnan(p).any((1, 2))]).cuda()
    modes, stats = dn.heatmap_modes(clean[:, None], 0, 1), dn.heatmap_stats(clean)
    assert torch.equal(modes['index'][:, 0, 0], stats['peak_index'])
    assert torch.equal(modes['mass'][:, 0, 0], stats['peak'])    # (float)(double) p of one pixel is p


# ------------------------------------------------------------------ interface
def test_leading_dimensions_no_grad_and_refusals():
    import dsnt.nn as dn
    p = ref.seeded_maps(16, 16)[:24]
    hm = torch.from_numpy(p.copy()).cuda().view(2, 3, 4, 16, 16).requires_grad_()
    out = dn.heatmap_modes(hm)                                    # radius 3, two modes
    assert out['coords'].shape == (2, 3, 4, 2, 2) and out['mass'].shape == out['index'].shape == (2, 3, 4, 2)
    assert not any(v.requires_grad for v in out.values())
    _check(_np(out), {k: v[:24] for k, v in ref.seeded_modes(16, 16, 3).items()}, 2, 'leading dimensions')
    with pytest.raises(RuntimeError, match='dsnt_map_modes: map 64x129 outside 1..8192 pixels'):
        dn.heatmap_modes(torch.zeros(1, 1, 64, 129, device='cuda'))
    with pytest.raises(RuntimeError, match='for 6 samples'):
        dn.heatmap_modes(hm, transform_m=torch.zeros(5, 2, 2), transform_b=torch.zeros(5, 1, 2))


def test_launch_list_records_and_replays_the_call():
    from dsnt import _lib
    lib = _lib.load()
    h, w, r, K = 63, 65, 3, 4
    hm = _device_maps(h, w)
    tm, tb = _device_transforms()
    n = ref.N_ROWS

    def buffers():
        return (torch.full((n, K, 2), 7.0, device='cuda'), torch.full((n, K), 7.0, device='cuda'),
                torch.full((n, K), 7, device='cuda', dtype=torch.int32),
                torch.full((n, K, 2), 7.0, device='cuda', dtype=torch.float64))

    def args(bufs):
        coords, mass, index, image = bufs
        return (hm.data_ptr(), n, 16, h, w, r, K, tm.data_ptr(), tb.data_ptr(), coords.data_ptr(), mass.data_ptr(),
                index.data_ptr(), image.data_ptr())

    direct, replayed = buffers(), buffers()
    _lib.call('dsnt_map_modes', *args(direct))
    lst = lib.dsnt_list_create()
    try:
        assert lib.dsnt_list_begin(lst) == 0
        try:
            assert lib.dsnt_map_modes(*args(replayed), C.c_void_p(0)) == 0          # `stream` = lane 0
        finally:
            lib.dsnt_list_end()
        assert lib.dsnt_list_size(lst) == 1
        torch.cuda.synchronize()
        assert all((b == 7).all().item() for b in replayed)                          # recorded, not launched
        streams = (C.c_void_p * 1)(torch.cuda.current_stream().cuda_stream)
        assert lib.dsnt_list_replay(lst, -1, streams, 1) == 0
        torch.cuda.synchronize()
    finally:
        lib.dsnt_list_destroy(lst)
    for a, b in zip(direct, replayed):
        assert _same_bits(a.cpu().numpy(), b.cpu().numpy())
    got = dict(zip(('coords', 'mass', 'index'), (t.cpu().numpy() for t in replayed[:3])))
    _check(got, ref.seeded_modes(h, w, r), K, 'replayed')
