"""Heat-map mass at the target on the device (`target_mass_kernel`, csrc/pckh.hip, through `dsnt_target_mass`) and
`dsnt.evaluator.target_mass` against the numpy restatement of tests/confusion_ref.py.

The bound is derived, not measured: the restatement is the exact sum (math.fsum) rounded to fp32 once; the device sums
at most 2^24 fp32 values in fp64, whose error (at most 2^24 roundings of 2^-53 relative each: 2^-29 of the sum of the
magnitudes, and the maps are non-negative) is far below half an fp32 ulp (2^-25 relative), and rounds that to fp32: the
two can differ by the double rounding alone, one fp32 ulp.  Which pixels a disc holds is exact: tests/test_confusion_cpu.py
holds every pixel centre of every seeded case 1e-9 relative clear of the edge of every disc.

Maps: 8 x 8 (64 pixels: fewer 4-pixel groups than threads), 5 x 7 (w % 4 != 0: scalar loads, groups that cross rows, a
last group of three), 64 x 64 (four trips of the threads) and 16 x 260 (five trips, the last one partial).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import confusion_ref as ref
import score_ref
from dsnt._lib import call, ptr

pytestmark = pytest.mark.gpu

THR = ref.THR


@functools.lru_cache(maxsize=None)
def reference(shape):
    """(args, mirror, out, pixels) of a seeded shape: restated once, shared by the tests, never written to."""
    args, mirror = ref.mass_shape_case(*shape), ref.mirror_of(shape[1])
    return (args, mirror) + ref.restate_mass(*args, mirror)[:2]


def on_device(args, mirror, thr=THR, offset=0):
    """One `dsnt_target_mass` call on numpy (hm, target, m, b, mask, head) -> f32 [B, J, 2] as numpy, 8 guard floats
    behind it checked.  `offset`: the maps start that many floats into their allocation (1: not 16-byte aligned)."""
    B, J, h, w = args[0].shape
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
    assert dev[0].dtype == dev[1].dtype == dev[4].dtype == torch.float32 and dev[2].dtype == dev[5].dtype == torch.float64
    if offset:
        room = torch.zeros(dev[0].numel() + offset, device='cuda')
        room[offset:] = dev[0].reshape(-1)
        dev[0] = room[offset:].view(B, J, h, w)
        assert dev[0].data_ptr() % 16 == 4 * offset and dev[0].is_contiguous()
    out = torch.full((B * J * 2 + 8,), -7.0, device='cuda')
    call('dsnt_target_mass', *[ptr(t) for t in dev], thr, (C.c_int * J)(*mirror), ptr(out), B, J, h, w)
    out = out.cpu()
    assert (out[B * J * 2:] == -7.0).all().item()
    return out[:B * J * 2].view(B, J, 2).numpy()


def within_one_ulp(got, want):
    """Both NaN, or `got` is `want` or one of its two fp32 neighbours."""
    lo, hi = np.nextafter(want, np.float32(-np.inf)), np.nextafter(want, np.float32(np.inf))
    return (np.isnan(got) & np.isnan(want)) | ((got >= lo) & (got <= hi))


@pytest.mark.parametrize('shape', ref.MASS_SHAPES, ids=['%dx%d-%dx%d' % s for s in ref.MASS_SHAPES])
def test_mass_matches_restatement(shape):
    args, mirror, want, pixels = reference(shape)
    got = on_device(args, mirror)
    assert got.dtype == want.dtype == np.float32
    assert np.array_equal(np.isnan(got), pixels < 0)            # the NaN pattern, exactly
    both = pixels >= 0
    with np.errstate(invalid='ignore'):
        ulps = np.abs(got[both].astype(np.float64) - want[both]) / np.spacing(np.maximum(want[both], np.float32(1e-30)))
    print('%s: %d discs, %d without a pixel, largest difference %.2f ulp' % (shape, both.sum(), (pixels == 0).sum(),
                                                                              ulps.max() if ulps.size else 0.0))
    assert (got[pixels == 0] == 0).all()                        # exactly 0 where the disc holds no pixel
    assert within_one_ulp(got, want).all()
    # bit-reproducible, and the same bits from maps that are not 16-byte aligned (scalar loads, the same order)
    assert np.array_equal(on_device(args, mirror), got, equal_nan=True)
    assert np.array_equal(on_device(args, mirror, offset=1), got, equal_nan=True)
    # the bimodal map: a good part of its mass at its own target, a good part at its mirror's
    assert got[0, 0, 0] > 0.2 and got[0, 0, 1] > 0.2


@pytest.mark.parametrize('shape', [(3, 16, 64, 64), (3, 2, 5, 7), (1, 16, 16, 260)], ids=lambda s: '%dx%d-%dx%d' % s)
def test_all_ones_map_counts_the_pixels(shape):
    args, mirror, _, pixels = reference(shape)
    got = on_device((np.ones(shape, np.float32),) + args[1:], mirror)
    assert np.array_equal(np.isnan(got), pixels < 0) and np.array_equal(got[pixels >= 0], pixels[pixels >= 0].astype(np.float32))
    assert pixels.max() > 64 or shape[2] * shape[3] < 64        # more than one pixel per thread somewhere


def test_edges_of_the_rule():
    """Identity-like transform x -> 8 x + 8 on an 8 x 8 map (pixel centres at 1, 3, ..., 15 in both axes), head length 5,
    in numbers that are exact: a disc of radius 2.5 round (5, 5) holds five centres; radius 2 reaches its four neighbours
    exactly (<=); a disc wholly outside the map and one between the centres hold none; a threshold of 0 holds the centre
    it sits on."""
    hm = np.arange(128, dtype=np.float32).reshape(1, 2, 8, 8)
    m, b, head = np.array([[[8.0, 0.0], [0.0, 8.0]]]), np.array([[8.0, 8.0]]), np.array([5.0])
    at = lambda x, y: [(x - 8) / 8, (y - 8) / 8]
    cross = lambda k: hm[0, k, 2, 2] + hm[0, k, 1, 2] + hm[0, k, 3, 2] + hm[0, k, 2, 1] + hm[0, k, 2, 3]
    mask = np.ones((1, 2), np.float32)

    def run(t0, t1, thr=0.5, mask=mask, mirror=(1, 0), head=head):
        target = np.array([[t0, t1]], np.float32)
        got = on_device((hm, target, m, b, mask, head), list(mirror), thr)
        want = ref.restate_mass(hm, target, m, b, mask, head, list(mirror), thr)[0]
        assert np.array_equal(got, want, equal_nan=True)
        return got[0]
    got = run(at(5, 5), at(100, 5))                             # the second target: wholly outside
    assert got.tolist() == [[cross(0), 0.0], [0.0, cross(1)]]
    got = run(at(5, 5), at(100, 5), head=np.array([4.0]))       # radius 2: the neighbours are at 2 / 4 = 0.5 exactly
    assert got.tolist() == [[cross(0), 0.0], [0.0, cross(1)]]
    got = run(at(5, 5), at(6, 6), thr=0.25)                     # radius 1.25: the centre alone; none round (6, 6)
    assert got.tolist() == [[hm[0, 0, 2, 2], 0.0], [0.0, hm[0, 1, 2, 2]]]
    got = run(at(5, 5), at(6, 6), thr=0.0)                      # radius 0: the centre it sits on
    assert got.tolist() == [[hm[0, 0, 2, 2], 0.0], [0.0, hm[0, 1, 2, 2]]]
    # no partner, a partner that is not annotated, a joint that is not counted; NaN targets of masked joints
    got = run(at(5, 5), at(5, 5), mirror=(0, 1))
    assert got[:, 0].tolist() == [cross(0), cross(1)] and np.isnan(got[:, 1]).all()
    got = run(at(5, 5), [np.nan, np.nan], mask=np.array([[1, 0.5]], np.float32))
    assert got[0, 0] == cross(0) and np.isnan(got[0, 1]) and np.isnan(got[1]).all()
    got = run(at(5, 5), [np.nan, np.nan])                       # annotated and NaN: no comparison holds
    assert got.tolist()[0] == [cross(0), 0.0] and got.tolist()[1] == [0.0, cross(1)]


def test_wrapper_and_reliability_fed_the_mass():
    """`evaluator.target_mass` is the entry point's output, from inputs it has to convert; as the score of `Reliability`
    the table is the host restatement's (tests/score_ref.py) of the same scores."""
    from dsnt.evaluator import Reliability, target_mass
    shape = (3, 16, 64, 64)
    args, mirror, want, pixels = reference(shape)
    hm, target, m, b, mask, head = args
    direct = on_device(args, mirror)
    t = lambda a: torch.from_numpy(a).cuda()
    mass = target_mass(t(hm).double(), t(target).double(), t(mask), t(head).float().double(), t(m), t(b).reshape(3, 1, 2))
    assert mass.dtype == torch.float32 and mass.is_cuda and tuple(mass.shape) == (3, 16, 2)
    head32 = head.astype(np.float32).astype(np.float64)
    assert np.array_equal(mass.cpu().numpy(), on_device((hm, target, m, b, mask, head32), mirror), equal_nan=True)
    assert np.array_equal(target_mass(t(hm), t(target), t(mask), t(head), t(m), t(b), mirror=mirror).cpu().numpy(), direct,
                          equal_nan=True)
    none = target_mass(t(hm), t(target), t(mask), t(head), t(m), t(b), mirror=range(16)).cpu().numpy()
    assert np.array_equal(none[..., 0], direct[..., 0], equal_nan=True) and np.isnan(none[..., 1]).all()
    # composition: misses that held at least half their mass at the truth are row 1 less its hits
    pred = ref.mass_pred(target)
    edges, thr = score_ref.f32([0.5]), score_ref.THR1
    rel = Reliability(edges, thresholds=thr)
    score = target_mass(t(hm), t(target), t(mask), t(head), t(m), t(b))[..., 0]
    rel.add_normalized(t(pred), t(target), t(mask), t(head), t(m), t(b), score)
    table = score_ref.restate(pred, target, m, b, mask, head, direct[..., 0], edges, thr)
    assert np.array_equal(rel.counts().numpy(), table) and table.sum() == (mask == 1).sum()
    assert table[:, 2].sum() == 0 and table[:, 0].sum() > 0 and table[:, 1].sum() > 0       # no counted joint is unscored
    rate, support = rel.accuracy(0.5, 'all')
    assert support[1] * (1 - rate[1]) == pytest.approx(table[:, 1, 1].sum())
