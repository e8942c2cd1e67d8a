"""Pin the oracle to every known-answer vector the reference's tests hold for the path.

Each test restates the expected values of a reference test (cited) and checks the
ORACLE (`oracle/dsnt_oracle`) against them.  The reference's harness runs with
default dtype double and tolerance 1e-5 (`tests/common.py:18,72`); same here.
"""
import pytest
import torch

from dsnt_oracle import nn as onn
from dsnt_oracle.evaluator import PCKhEvaluator

TOL = 1e-5


@pytest.fixture(autouse=True)
def _double_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    torch.manual_seed(0)
    yield
    torch.set_default_dtype(old)


SIMPLE_INPUT = [[[[0.0, 0.0, 0.0, 0.0, 0.0],
                  [0.0, 0.0, 0.0, 0.1, 0.0],
                  [0.0, 0.0, 0.1, 0.6, 0.1],
                  [0.0, 0.0, 0.0, 0.1, 0.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0]]]]
# d MSE(dsnt(h), (0.5,0.5)) / dh: 0.48 at the top-left, -0.04 per column, -0.20 per row
SIMPLE_GRAD = [[[[0.48 - 0.04 * c - 0.20 * r for c in range(5)] for r in range(5)]]]


def test_dsnt_forward_backward():  # reference tests/test_nn.py:10-50
    h = torch.tensor(SIMPLE_INPUT, requires_grad=True)
    out = onn.dsnt(h)
    assert (out.detach() - torch.tensor([[[0.4, 0.0]]])).abs().max() <= TOL
    torch.nn.functional.mse_loss(out, torch.tensor([[[0.5, 0.5]]])).backward()
    assert (h.grad - torch.tensor(SIMPLE_GRAD)).abs().max() <= TOL


def test_dsnt_batchless():  # tests/test_nn.py:52-66
    h = torch.tensor(SIMPLE_INPUT[0], requires_grad=True)
    out = onn.dsnt(h)
    assert out.shape == (1, 2)
    assert (out.detach() - torch.tensor([[0.4, 0.0]])).abs().max() <= TOL
    torch.nn.functional.mse_loss(out, torch.tensor([[0.5, 0.5]])).backward()
    assert (h.grad - torch.tensor(SIMPLE_GRAD[0])).abs().max() <= TOL


def test_euclidean_loss():  # tests/test_nn.py:86-109
    a = torch.tensor([[[3.0, 4], [3, 4]], [[3, 4], [3, 4]]], requires_grad=True)
    loss = onn.euclidean_loss(a, torch.zeros(2, 2, 2))
    loss.backward()
    assert abs(loss.item() - 5.0) <= TOL
    assert (a.grad - torch.tensor([0.15, 0.20]).expand(2, 2, 2)).abs().max() <= TOL


def test_euclidean_loss_mask():  # tests/test_nn.py:111-130
    out = torch.tensor([[[0.0, 0], [1, 1], [0, 0]], [[1, 1], [0, 0], [0, 0]]])
    mask = torch.tensor([[1.0, 0, 1], [0, 1, 1]])
    assert abs(onn.euclidean_loss(out, torch.zeros(2, 3, 2), mask).item()) <= TOL


def test_thresholded_softmax_forward():  # tests/test_nn.py:134-149
    got = onn.thresholded_softmax(torch.tensor([2.0, 1, 3]), 1.5)
    assert (got - torch.tensor([0.26894142, 0, 0.73105858])).abs().max() <= TOL
    got = onn.thresholded_softmax(torch.tensor([[2.0, 1, 3], [4, 0, 0]]), 1.5)
    want = torch.tensor([[0.26894142, 0, 0.73105858], [1, 0, 0]])
    assert (got - want).abs().max() <= TOL


@pytest.mark.parametrize('shape', [(20,), (3, 20)])
def test_thresholded_softmax_gradcheck(shape):  # tests/test_nn.py:140-154
    x = torch.randn(*shape, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: onn.thresholded_softmax(t, 0), (x,))


def test_make_gauss():  # tests/test_nn.py:158-167
    want = torch.tensor([[0.0030, 0.0133, 0.0219, 0.0133, 0.0030],
                         [0.0133, 0.0596, 0.0983, 0.0596, 0.0133],
                         [0.0219, 0.0983, 0.1621, 0.0983, 0.0219],
                         [0.0133, 0.0596, 0.0983, 0.0596, 0.0133],
                         [0.0030, 0.0133, 0.0219, 0.0133, 0.0030]])
    got = onn.make_gauss(torch.tensor([0.0, 0.0]), 5, 5, sigma=0.4)
    assert (got - want).abs().max() <= 1e-4


@pytest.mark.parametrize('loss_fn,shift_mean', [
    (onn.kl_reg_loss, True), (onn.mse_reg_loss, True), (onn.js_reg_loss, True),
    (onn.variance_reg_loss, False)])
def test_reg_loss_minimum(loss_fn, shift_mean):  # tests/test_nn.py:170-239
    mean, std = torch.tensor([0.0, 0.0]), 0.4

    def calc(m, s):
        return loss_fn(onn.make_gauss(m, 5, 5, sigma=s), mean, std, mask=None).item()

    lo = calc(mean, std)
    assert abs(lo) <= 1e-3
    assert calc(mean, std + 0.2) > lo + 1e-3
    assert calc(mean, std - 0.2) > lo + 1e-3
    if shift_mean:
        assert calc(mean + 0.1, std) > lo + 1e-3
        assert calc(mean - 0.1, std) > lo + 1e-3


def test_kl_reg_loss_mask():  # tests/test_nn.py:204-224
    t = torch.zeros(2, 4, 4)
    t[0, 2, 3] = t[0, 3, 2] = 0.1
    t[0, 3, 3] = 0.8
    t[1, 0, 0] = 0.8
    t[1, 0, 1] = t[1, 1, 0] = 0.1
    got = onn.kl_reg_loss(t, torch.tensor([[1.0, 1], [0, 0]]), 1, torch.tensor([1.0, 0]))
    assert abs(got.item() - 1.2228811717796824) <= TOL


def test_pckh_distance():  # tests/test_evaluator.py:8-16
    d = PCKhEvaluator.calculate_pckh_distance(
        torch.tensor([951.84, 580.64]), torch.tensor([804.0, 711]), 117.962)
    assert abs(float(d) - 1.6709) <= 1e-4


def test_pckh_add():  # tests/test_evaluator.py:18-39
    ev = PCKhEvaluator(threshold=0.5)
    pred = torch.tensor([[[951.84, 580.64]], [[317.76, 406.75]], [[float('inf')] * 2]])
    target = torch.tensor([[[804.0, 711]], [[317, 412]], [[float('nan')] * 2]])
    ev.add(pred, target, torch.tensor([[1.0], [1], [0]]),
           torch.tensor([117.962, 44.046, 78.481]))
    assert ev.meters['all'].value()[0] == 0.5


# ---------------------------------------------------------------- heat-map ("gauss") strategy: util.py
from dsnt_oracle import util as outil  # noqa: E402

_G = [0.00034, 0.01111, 0.13534, 0.60653, 1.00000, 0.60653, 0.13534, 0.01111, 0.00034]   # exp(-d^2/2), d=-4..4


def test_draw_gaussian():  # tests/test_util.py:8-24
    expected = torch.tensor([[[_G[i] * _G[j] for j in range(9)] for i in range(9)]], dtype=torch.float32)
    actual = torch.zeros(1, 9, 9, dtype=torch.float32)
    outil.draw_gaussian(actual, 4, 4, 1, normalize=False)
    assert (expected - actual).abs().max().item() <= 1.5e-5     # the table is rounded to 5 decimals


_CLIPPED = [[0.00000, 0.00000, 0.00000, 0.00000, 0.00000],
            [0.01111, 0.00674, 0.00150, 0.00012, 0.00000],
            [0.13534, 0.08208, 0.01832, 0.00150, 0.00000],
            [0.60653, 0.36788, 0.08208, 0.00674, 0.00000],
            [1.00000, 0.60653, 0.13534, 0.01111, 0.00000]]


def test_draw_gaussian_clipped():  # tests/test_util.py:26-38
    actual = torch.zeros(1, 5, 5, dtype=torch.float32)
    outil.draw_gaussian(actual, 0, 4, 1, normalize=False, clip_size=7)
    assert (torch.tensor([_CLIPPED], dtype=torch.float32) - actual).abs().max().item() <= TOL


def test_encode_heatmaps():  # tests/test_util.py:40-53
    coords = torch.tensor([[[-0.8, 0.8]]], dtype=torch.float32)
    actual = outil.encode_heatmaps(coords, 5, 5)
    assert actual.dtype == torch.float32
    assert (torch.tensor([[_CLIPPED]], dtype=torch.float32) - actual).abs().max().item() <= TOL
    assert torch.equal(coords, torch.tensor([[[-0.8, 0.8]]], dtype=torch.float32))   # works on a copy


def test_decode_heatmaps():  # tests/test_util.py:55-64
    heatmaps = torch.tensor([[[[0.0, 0.9], [0.0, 0.1]]]], dtype=torch.float32)
    actual = outil.decode_heatmaps(heatmaps)
    assert (torch.tensor([[[0.5, -0.5]]], dtype=torch.float32) - actual).abs().max().item() <= 1e-7


def test_decode_heatmaps_use_neighbours():  # tests/test_util.py:66-77
    heatmaps = torch.tensor([[[[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.9, 0.1, 0.0],
                               [0.0, 0.1, 0.0, 0.0]]]], dtype=torch.float32)
    actual = outil.decode_heatmaps(heatmaps, use_neighbours=True)
    assert (torch.tensor([[[-0.125, 0.375]]], dtype=torch.float32) - actual).abs().max().item() <= 1e-7


# ---------------------------------------------------------------- hand-derived answers off the square map
# (none in the reference's tests: get_preds' `idx / height` differs from the true row as soon as H != W, util.py:161)
_ULP2 = 2.4e-7        # the expected values are fp64 arithmetic rounded to fp32; the chain of fp32 steps lands within two
                      # ulp of a value below 2 (a pixel is 0.2 or more on these maps)


def _map(h, w, cells):
    hm = torch.zeros(1, 1, h, w, dtype=torch.float32)
    for (r, c), v in cells.items():
        hm[0, 0, r, c] = v
    return hm


def _f32(rows):
    return torch.tensor([[list(r) for r in rows]], dtype=torch.float32)


def test_decode_wide_map():
    """H=5, W=9, 9.0 at [3, 7]: idx = 34, x = 34 % 9 = 7, y = 34 // 5 = 6, past the last row, so no neighbour step."""
    hm = _map(5, 9, {(3, 7): 9.0})
    assert torch.equal(outil.get_preds(hm), _f32([(7.0, 6.0)]))
    for nb in (True, False):
        got = outil.decode_heatmaps(hm, use_neighbours=nb)
        assert (got - _f32([(7.5 * 2 / 9 - 1, 6.5 * 2 / 5 - 1)])).abs().max().item() <= _ULP2      # (0.66667, 1.6)


def test_decode_tall_map():
    """H=9, W=5, 9.0 at [7, 2]: idx = 37, x = 37 % 5 = 2, y = 37 // 9 = 4 while the true row is 7.  (2, 4) is interior,
    so the neighbour step reads ROW 4: hm[4, 3] - hm[4, 1] = 1 > 0 and hm[5, 2] - hm[3, 2] = -2 < 0."""
    hm = _map(9, 5, {(7, 2): 9.0, (4, 3): 1.0, (3, 2): 2.0})
    assert torch.equal(outil.get_preds(hm), _f32([(2.0, 4.0)]))
    got = outil.decode_heatmaps(hm, use_neighbours=False)
    assert (got - _f32([(2.5 * 2 / 5 - 1, 4.5 * 2 / 9 - 1)])).abs().max().item() <= _ULP2           # (0, 0)
    got = outil.decode_heatmaps(hm, use_neighbours=True)
    assert (got - _f32([(2.75 * 2 / 5 - 1, 4.25 * 2 / 9 - 1)])).abs().max().item() <= _ULP2         # (0.1, -0.05556)


def test_decode_nan_is_the_maximum():
    """torch.max propagates NaN: the maximum is NaN, `maxval.gt(0)` is false and the prediction is pixel (0, 0), whatever
    else the map holds."""
    hm = _map(6, 6, {(2, 3): float('nan'), (4, 4): 50.0})
    assert torch.equal(outil.get_preds(hm), _f32([(0.0, 0.0)]))
    for nb in (True, False):
        got = outil.decode_heatmaps(hm, use_neighbours=nb)
        assert (got - _f32([(-5 / 6, -5 / 6)])).abs().max().item() <= _ULP2


# target, bump centre (x, y) and window columns / rows on a 5 x 9 map (W/2 = 4.5, H/2 = 2.5; util.py:132-144 and
# draw_gaussian with radius 3.5):
#   (-1, 1):   px = 0 * 4.5 - 0.5 = -0.5 -> round-half-even -> 0;  py = 2 * 2.5 - 0.5 = 4.5 -> 4
#   (0, 0):    px = 4.5 - 0.5 = 4;  py = 2.5 - 0.5 = 2
#   (1.2, 0):  px = 2.2 * 4.5 - 0.5 = 9.4 -> 9, one pixel right of the map; 9 < 8 + 3.5, so drawn, clipped to columns
#              ceil(9 - 3.5) = 6 .. 8
#   (2.0, 0):  px = 3 * 4.5 - 0.5 = 13 >= 8 + 3.5: skipped
_ENCODE_5x9 = [((-1.0, 1.0), (0, 4), range(0, 4), range(1, 5)),
               ((0.0, 0.0), (4, 2), range(1, 8), range(0, 5)),
               ((1.2, 0.0), (9, 2), range(6, 9), range(0, 5)),
               ((2.0, 0.0), (13, 2), range(0, 0), range(0, 0))]


def test_encode_heatmaps_wide_map():
    import math
    coords = torch.tensor([[list(t) for t, _, _, _ in _ENCODE_5x9]], dtype=torch.float32)
    got = outil.encode_heatmaps(coords, 9, 5)
    assert got.shape == (1, 4, 5, 9)
    for j, (_, (cx, cy), cols, rows) in enumerate(_ENCODE_5x9):
        want = torch.zeros(5, 9, dtype=torch.float32)
        for r in rows:
            for c in cols:
                want[r, c] = math.exp(-((c - cx) ** 2 + (r - cy) ** 2) / 2)
        assert torch.equal(got[0, j] != 0, want != 0), j
        assert (got[0, j] - want).abs().max().item() <= 1e-6, j
