"""The `fc` output strategy (`fc2_fwd_kernel` / `fc2_bwd_kernel`, csrc/head_ops.hip) and the PCKh hit test (`pckh_kernel`,
csrc/pckh.hip) called directly, against fp64 restatements.

fc: `out = hm @ W.T + b` per (image, joint) row, weights at nn.Linear's scale (uniform in +-1/sqrt(hw)), heat-maps from a
softmax.  Bar: 2e-5 of the largest entry of each fp64 result (the gradient bar of tests/test_head_gpu.py).  `gw` is a
sequential fp32 sum over the rows: the same sum in numpy fp32, with two roundings per term where the kernel's fma has one,
is within 4.4e-7 of the largest entry at 130 rows, a margin of 46.

PCKh: hits and valid must equal the numpy restatement exactly; every case keeps d / head away from the threshold by far
more than an fp64 rounding, except the boundary cases, whose values are exact.
"""
import numpy as np
import pytest
import torch

from dsnt._lib import call, ptr

pytestmark = pytest.mark.gpu

HW = {16: (4, 4), 49: (7, 7), 255: (15, 17), 256: (16, 16), 257: (1, 257), 1000: (25, 40), 4096: (64, 64)}
ROWS = [1, 48, 130]
BAR = 2e-5


def _within(got, want, what):
    err = (got.detach().cpu().double() - want).abs().max().item()
    scale = want.abs().max().item()
    print('%s: err %.3e, %.3e of the largest entry' % (what, err, err / scale))
    assert err <= BAR * scale, (what, err, scale)


_fc_cache = {}


def _fc_case(hw, rows):
    """Inputs and the fp64 forward and autograd results, computed once per (hw, rows)."""
    if (hw, rows) not in _fc_cache:
        h, w = HW[hw]
        g = torch.Generator().manual_seed(hw * 1000 + rows)
        hm = torch.softmax(torch.randn(rows, hw, generator=g) * 2, -1).view(rows, h, w)
        bound = hw ** -0.5
        weight = (torch.rand(2, hw, generator=g) * 2 - 1) * bound
        bias = (torch.rand(2, generator=g) * 2 - 1) * bound
        gout = torch.randn(rows, 2, generator=g)
        hd = hm.double().view(rows, hw).requires_grad_()
        wd, bd = weight.double().requires_grad_(), bias.double().requires_grad_()
        out = hd @ wd.T + bd
        out.backward(gout.double())
        _fc_cache[hw, rows] = {'hm': hm, 'w': weight, 'b': bias, 'g': gout, 'out': out.detach(),
                               'out_nobias': (hd @ wd.T).detach(), 'ghm': hd.grad.view(rows, h, w), 'gw': wd.grad,
                               'gb': bd.grad}
    return _fc_cache[hw, rows]


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('hw', sorted(HW))
def test_fc_forward(hw, rows):
    import dsnt.nn as dn
    c = _fc_case(hw, rows)
    hm, w, b = c['hm'].cuda(), c['w'].cuda(), c['b'].cuda()
    out = dn.fc_coords(hm, w, b)
    assert out.shape == (rows, 2)
    _within(out, c['out'], 'fc fwd hw=%d rows=%d' % (hw, rows))
    _within(dn.fc_coords(hm, w, None), c['out_nobias'], 'fc fwd, no bias')
    # the ABI call with bias = NULL, into a buffer with a guard behind it
    buf = torch.full((rows * 2 + 8,), -7.0, device='cuda')
    call('dsnt_fc2_fwd', ptr(hm), ptr(w), None, ptr(buf), rows, hw)
    _within(buf[:rows * 2].view(rows, 2), c['out_nobias'], 'dsnt_fc2_fwd, b = NULL')
    assert (buf[rows * 2:] == -7.0).all().item()


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('hw', sorted(HW))
def test_fc_backward(hw, rows):
    import dsnt.nn as dn
    c = _fc_case(hw, rows)
    what = 'hw=%d rows=%d' % (hw, rows)
    hm, w, b, g = c['hm'].cuda(), c['w'].cuda(), c['b'].cuda(), c['g'].cuda()

    def bwd(want_ghm, want_gb):
        """dsnt_fc2_bwd into guarded buffers; NULL for the outputs not wanted."""
        ghm = torch.full((rows * hw + 8,), -7.0, device='cuda') if want_ghm else None
        gw = torch.full((2 * hw + 8,), -7.0, device='cuda')
        gb = torch.full((2 + 8,), -7.0, device='cuda') if want_gb else None
        call('dsnt_fc2_bwd', ptr(g), ptr(hm), ptr(w), ptr(ghm), ptr(gw), ptr(gb), rows, hw)
        for t, n in ((ghm, rows * hw), (gw, 2 * hw), (gb, 2)):
            assert t is None or (t[n:] == -7.0).all().item()
        return (None if ghm is None else ghm[:rows * hw].view_as(hm), gw[:2 * hw].view(2, hw),
                None if gb is None else gb[:2])
    ghm, gw, gb = bwd(True, True)
    _within(ghm, c['ghm'], 'ghm ' + what)
    _within(gw, c['gw'], 'gw ' + what)
    _within(gb, c['gb'], 'gb ' + what)
    none, gw2, gb2 = bwd(False, True)                  # ghm = NULL: an input that needs no gradient
    assert none is None and torch.equal(gw2, gw) and torch.equal(gb2, gb)
    ghm3, gw3, none = bwd(True, False)                 # gb = NULL: no bias
    assert none is None and torch.equal(gw3, gw) and torch.equal(ghm3, ghm)
    assert torch.equal(bwd(True, True)[1], gw)         # the rows are summed in order: the same bits every time
    # the autograd function makes the same calls
    hg, wg, bg = hm.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    dn.fc_coords(hg, wg, bg).backward(g)
    assert torch.equal(hg.grad, ghm) and torch.equal(wg.grad, gw) and torch.equal(bg.grad, gb)
    wg.grad = None
    dn.fc_coords(hm, wg, None).backward(g)             # heat-maps without a gradient, no bias
    assert torch.equal(wg.grad, gw)


# ------------------------------------------------------------------ PCKh
def pckh_ref(pred, target, m, b, mask, head, thr):
    """`pckh_kernel` in numpy fp64: bmm(x, m) + b on row vectors (train.py:243-258), the distance over the head length,
    a hit when it is <= the fp32 threshold, and only where the mask equals 1 (oracle/dsnt_oracle/evaluator.py:62)."""
    with np.errstate(all='ignore'):
        d = pckh_distance(pred, target, m, b, head)
        valid = mask == 1
        return (valid & (d <= _thr32(thr))).astype(np.float32), valid.astype(np.float32)


def _thr32(thr):
    """The threshold as the kernel holds it: an fp32 argument, compared in fp64 (0.2 moves by 1.5e-8 relative)."""
    return float(np.float32(thr))


def pckh_distance(pred, target, m, b, head):
    p = np.einsum('bji,bik->bjk', pred.astype(np.float64), m) + b[:, None, :]
    t = np.einsum('bji,bik->bjk', target.astype(np.float64), m) + b[:, None, :]
    return np.sqrt((p[..., 0] - t[..., 0]) ** 2 + (p[..., 1] - t[..., 1]) ** 2) / head[:, None]


def pckh_dev(pred, target, m, b, mask, head, thr):
    B, J = mask.shape
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (pred, target, m, b, mask, head)]
    assert dev[0].dtype == dev[1].dtype == dev[4].dtype == torch.float32 and dev[2].dtype == dev[5].dtype == torch.float64
    hits = torch.full((B * J + 8,), -7.0, device='cuda')
    valid = torch.full((B * J + 8,), -7.0, device='cuda')
    call('dsnt_pckh', *[ptr(t) for t in dev], float(thr), ptr(hits), ptr(valid), B, J)
    assert (hits[B * J:] == -7.0).all().item() and (valid[B * J:] == -7.0).all().item()
    return hits[:B * J].view(B, J).cpu().numpy(), valid[:B * J].view(B, J).cpu().numpy()


def _identity(B):
    return np.tile(np.eye(2), (B, 1, 1)), np.zeros((B, 2))


def test_pckh_threshold_boundary():
    """m = I, b = 0, |(3, 4) - (0, 0)| = 5 and head 10: d = 0.5 exactly, a hit at threshold 0.5; one ulp less head: a miss."""
    one = np.ones((1, 1), np.float32)
    m, b = _identity(1)
    p, t = np.array([[[3.0, 4.0]]], np.float32), np.zeros((1, 1, 2), np.float32)
    for pred, target in ((p, t), (t, p)):
        for head, want in ((10.0, 1.0), (np.nextafter(10.0, 0.0), 0.0), (np.nextafter(10.0, 20.0), 1.0)):
            head = np.array([head])
            hits, valid = pckh_dev(pred, target, m, b, one, head, 0.5)
            assert pckh_ref(pred, target, m, b, one, head, 0.5)[0][0, 0] == want
            assert hits[0, 0] == want and valid[0, 0] == 1.0, (head, hits, valid)


def _pckh_case(B, J, seed):
    """Targets in normalised coordinates, predictions beside them so that about half are hits, a non-symmetric transform
    per image, and masks of 0, 1, 0.5 and 2."""
    r = np.random.default_rng(seed)
    target = r.uniform(-0.9, 0.9, (B, J, 2)).astype(np.float32)
    pred = (target + r.normal(0, 0.2, (B, J, 2))).astype(np.float32)
    m = np.array([[150.0, 90.0], [-20.0, 60.0]]) + r.uniform(-10, 10, (B, 2, 2))       # far from symmetric
    b = r.uniform(0, 400, (B, 2))
    head = r.uniform(40, 120, B)
    mask = r.choice(np.array([0, 1, 1, 1, 0.5, 2], np.float32), (B, J))
    return pred, target, m, b, mask, head


@pytest.mark.parametrize('B,J', [(37, 7), (1, 1), (16, 16), (70, 16), (257, 1)])
def test_pckh_matches_restatement(B, J):
    """259 and 257 joints leave three threads and one in the second workgroup; 70 x 16 needs five workgroups."""
    args = _pckh_case(B, J, seed=B * 100 + J)
    m, b = args[2], args[3]
    d = pckh_distance(args[0], args[1], m, b, args[5])
    for thr in (0.5, 0.2):
        assert np.abs(d / _thr32(thr) - 1).min() > 1e-9        # no joint within an fp64 rounding of the threshold
        want_h, want_v = pckh_ref(*args, thr)
        hits, valid = pckh_dev(*args, thr)
        assert np.array_equal(valid, want_v) and np.array_equal(hits, want_h), (B, J, thr)
        print('B=%d J=%d thr=%g: %d valid, %d hits' % (B, J, thr, want_v.sum(), want_h.sum()))
        if B * J >= 256:
            assert 0.1 < want_h.sum() / want_v.sum() < 0.9 and 0.3 < want_v.mean() < 0.7       # the case tests both outcomes
    # a transposed multiply gives other hits on these inputs, so the comparison above tells the two apart
    wrong = pckh_ref(args[0], args[1], m.transpose(0, 2, 1), b, args[4], args[5], 0.5)[0]
    assert B * J < 256 or (wrong != pckh_ref(*args, 0.5)[0]).sum() >= 5


def test_pckh_mask_values_and_oracle_meters():
    """Mask 0, 1, 0.5 and 2: only 1 counts, the rule of the oracle's evaluator (`joint_mask[b, j] == 1`).  The per-joint
    and group meters of the oracle, fed the back-projected coordinates, hold the kernel's counts."""
    from dsnt_oracle.evaluator import PCKhEvaluator
    pred, target, m, b, mask, head = _pckh_case(16, 16, seed=5)
    mask[0, :4] = [0, 1, 0.5, 2]
    hits, valid = pckh_dev(pred, target, m, b, mask, head, 0.5)
    assert valid[0, :4].tolist() == [0, 1, 0, 0] and np.array_equal(valid, (mask == 1).astype(np.float32))
    assert np.array_equal(hits, pckh_ref(pred, target, m, b, mask, head, 0.5)[0])
    tm, tb = torch.from_numpy(m), torch.from_numpy(b)[:, None]
    ev = PCKhEvaluator(0.5)
    ev.add(torch.baddbmm(tb, torch.from_numpy(pred).double(), tm), torch.baddbmm(tb, torch.from_numpy(target).double(), tm),
           torch.from_numpy(mask), torch.from_numpy(head))
    for j, name in enumerate(PCKhEvaluator.JOINT_NAMES):
        assert ev.meters[name].n == valid[:, j].sum() and ev.meters[name].total == hits[:, j].sum(), name
    assert ev.meters['all'].n == valid.sum() and ev.meters['all'].total == hits.sum()


def test_pckh_non_finite_coordinates():
    """NaN and inf coordinates are ordinary values: never a hit; counted as valid exactly when the mask is 1.  A zero head
    length with a non-zero distance is a miss, and the joints beside all of these are untouched."""
    nan, inf = float('nan'), float('inf')
    bad = [((nan, 0.0), (0.0, 0.0)), ((0.0, 0.0), (0.0, nan)), ((inf, 0.0), (0.0, 0.0)), ((0.0, 0.0), (-inf, 0.0)),
           ((inf, inf), (inf, inf)), ((nan, nan), (nan, nan))]
    B, J = len(bad), 4                     # joint 0: bad under mask 0; joint 1: bad under mask 1; joints 2, 3: a hit, a miss
    pred, target = np.zeros((B, J, 2), np.float32), np.zeros((B, J, 2), np.float32)
    for n, (p, t) in enumerate(bad):
        pred[n, 0] = pred[n, 1] = p
        target[n, 0] = target[n, 1] = t
    pred[:, 2] = (3.0, 4.0)                # d = 5 / 10
    pred[:, 3] = (6.0, 8.0)                # d = 10 / 10
    mask = np.tile(np.array([0, 1, 1, 1], np.float32), (B, 1))
    m, b = _identity(B)
    head = np.full(B, 10.0)
    hits, valid = pckh_dev(pred, target, m, b, mask, head, 0.5)
    assert np.array_equal(valid, mask) and np.array_equal(hits, np.tile(np.array([0, 0, 1, 0], np.float32), (B, 1)))
    want_h, want_v = pckh_ref(pred, target, m, b, mask, head, 0.5)
    assert np.array_equal(hits, want_h) and np.array_equal(valid, want_v)
    head[:] = 0.0                          # d = inf for joints 2 and 3
    hits, valid = pckh_dev(pred, target, m, b, mask, head, 0.5)
    assert np.array_equal(valid, mask) and not hits.any()
    assert np.array_equal(hits, pckh_ref(pred, target, m, b, mask, head, 0.5)[0])
