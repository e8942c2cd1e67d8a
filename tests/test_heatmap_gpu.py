"""HIP heat-map ("gauss") strategy vs the oracle and the reference's known answers (SURVEY 8 f-4:
`/root/reference/src/dsnt/util.py:129-198`, `/root/reference/src/dsnt/model.py:147-161, 247-269`).

Tolerances: target bumps 1e-6 absolute (device expf vs libm expf), losses 1e-5 relative, gradients 1e-5 relative
to the largest entry; decoding is index / sign arithmetic and must be exactly equal on the same heat-maps.
"""
import pytest
import torch
import torch.nn.functional as F

from dsnt import synthetic

pytestmark = pytest.mark.gpu

_CLIPPED = [[0.00000, 0.00000, 0.00000, 0.00000, 0.00000],
            [0.01111, 0.00674, 0.00150, 0.00012, 0.00000],
            [0.13534, 0.08208, 0.01832, 0.00150, 0.00000],
            [0.60653, 0.36788, 0.08208, 0.00674, 0.00000],
            [1.00000, 0.60653, 0.13534, 0.01111, 0.00000]]


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def test_known_answers(dev):
    from dsnt import util as du
    # tests/test_util.py:40-53
    coords = torch.tensor([[[-0.8, 0.8]]], device=dev)
    enc = du.encode_heatmaps(coords, 5, 5)
    assert (enc.cpu() - torch.tensor([[_CLIPPED]])).abs().max().item() <= 1e-5
    assert torch.equal(coords.cpu(), torch.tensor([[[-0.8, 0.8]]]))
    # tests/test_util.py:55-64
    hm = torch.tensor([[[[0.0, 0.9], [0.0, 0.1]]]], device=dev)
    assert (du.decode_heatmaps(hm).cpu() - torch.tensor([[[0.5, -0.5]]])).abs().max().item() <= 1e-7
    # tests/test_util.py:66-77
    hm = torch.tensor([[[[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.9, 0.1, 0.0], [0.0, 0.1, 0.0, 0.0]]]],
                      device=dev)
    assert (du.decode_heatmaps(hm, use_neighbours=True).cpu() - torch.tensor([[[-0.125, 0.375]]])).abs().max().item() <= 1e-7


@pytest.mark.parametrize('H,W,sigma', [(64, 64, 1.0), (16, 12, 1.25), (7, 9, 2.0)])
def test_encode_matches_oracle(dev, H, W, sigma):
    from dsnt import util as du
    from dsnt_oracle import util as ou
    coords = synthetic.tensor('hm.coords%d' % H, (5, 16, 2), seed=21, kind='uniform') * 1.15   # some off the map
    coords[0, 0] = torch.tensor([-1.0, 1.0]); coords[0, 1] = torch.tensor([0.0, 0.0])       # .5 pixel ties
    want = ou.encode_heatmaps(coords, W, H, sigma)
    got = du.encode_heatmaps(coords.to(dev), W, H, sigma).cpu()
    assert got.shape == want.shape == (5, 16, H, W)
    assert (got - want).abs().max().item() <= 1e-6
    assert torch.equal(got == 0, want == 0)


def test_mse_loss_and_gradient(dev):
    from dsnt import util as du
    from dsnt_oracle import util as ou
    hm = synthetic.tensor('hm.pred', (3, 16, 64, 64), seed=22) * 0.2
    coords = synthetic.tensor('hm.tgt', (3, 16, 2), seed=22, kind='uniform')
    ho = hm.clone().requires_grad_()
    lo = F.mse_loss(ho, ou.encode_heatmaps(coords, 64, 64, 1.0))
    (lo * 3.0).backward()
    hg = hm.to(dev).requires_grad_()
    lg = du.heatmap_mse_loss(hg, coords.to(dev), 1.0)
    (lg * 3.0).backward()
    assert abs(lg.item() - lo.item()) <= 1e-5 * abs(lo.item())
    assert (hg.grad.cpu() - ho.grad).abs().max().item() <= 1e-5 * ho.grad.abs().max().item()
    with pytest.raises(RuntimeError):
        du.heatmap_mse_loss(hg, coords[:2].to(dev), 1.0)
    with pytest.raises(RuntimeError):
        du.encode_heatmaps(coords, 64, 64)          # CPU tensor: no fallback


def test_decode_matches_oracle(dev):
    from dsnt import util as du
    from dsnt_oracle import util as ou
    hm = synthetic.tensor('hm.dec', (4, 16, 64, 64), seed=23)
    hm[0, 0].zero_()                                  # maximum not positive
    hm[0, 1] = -hm[0, 1].abs() - 1                    # all negative
    hm[0, 2, 0, 17] = 50.0                            # border row
    hm[0, 3, 20, 20] = 50.0; hm[0, 3, 20, 19] = hm[0, 3, 20, 21] = 1.0      # equal neighbours
    hm[0, 4, 30, 30] = hm[0, 4, 31, 5] = 50.0         # tie: first index wins
    hm[0, 5, 63, 63] = 50.0                           # corner
    for nb in (True, False):
        want = ou.decode_heatmaps(hm, use_neighbours=nb)
        got = du.decode_heatmaps(hm.to(dev), use_neighbours=nb).cpu()
        assert torch.equal(got, want)
    assert torch.equal(du.get_preds(hm.to(dev)).cpu(), ou.get_preds(hm))
    small = synthetic.tensor('hm.dec2', (2, 3, 16, 16), seed=24)
    assert torch.equal(du.decode_heatmaps(small.to(dev)).cpu(), ou.decode_heatmaps(small))


@pytest.mark.parametrize('base', ['hg2', 'resnet18'])
def test_gauss_strategy_train_step(dev, base):
    """The builder's default strategy for hourglass models (model.py:346): loss, every gradient direction and the
    decoded coordinates against the oracle."""
    from dsnt.model import build_mpii_pose_model
    from dsnt_oracle import model as omodel
    from dsnt_oracle import util as ou
    kw = {} if base.startswith('hg') else {'output_strat': 'gauss', 'dilate': 2}
    m = build_mpii_pose_model(base=base, **kw)
    o = omodel.build_mpii_pose_model(base=base, **kw)
    assert m.output_strat == o.output_strat == 'gauss'
    synthetic.fill_state_dict(m, seed=0)
    synthetic.fill_state_dict(o, seed=0)
    m.to(dev).train()
    o.train()
    size = 128 if base.startswith('hg') else 224
    x, t, k = synthetic.batch(2, size=size, seed=1, mask_p=0.9)
    out = m(x.to(dev))
    loss = m.forward_loss(out, t.to(dev), k.to(dev))
    loss.backward()
    oo = o(x)
    lo = o.forward_loss(oo, t, k)
    lo.backward()
    assert abs(loss.item() - lo.item()) <= 2e-5 * max(1.0, abs(lo.item()))
    gm = torch.cat([p.grad.reshape(-1).cpu() for p in m.parameters()]).double()
    go = torch.cat([p.grad.reshape(-1) for p in o.parameters()]).double()
    # (ReLU on, batch 2: one mask bit flipped between two correct fp32 implementations moves the flat gradient by ~1e-4 in
    # cosine — tests/test_model_gpu.py::_NoRelu; the flip-tolerant bar of the other ReLU-on tests)
    assert float(gm @ go / (gm.norm() * go.norm())) > 0.999
    last = out[-1] if isinstance(out, list) else out
    coords = m.compute_coords(out)
    assert coords.device.type == 'cpu' and coords.shape == (2, 16, 2)
    assert torch.equal(coords, ou.decode_heatmaps(last.detach().cpu()))       # same maps -> same decoding
    # against the oracle's own maps the arg-max may flip between near-equal pixels; most joints agree
    agree = (coords - o.compute_coords(oo)).abs().amax(-1) <= 1e-6
    assert agree.float().mean().item() >= 0.9


# ------------------------------------------------------------------ decode off the square map, ties across waves, NaN
DECODE_SHAPES = [(5, 9), (9, 5), (12, 20), (16, 12), (7, 7), (3, 3), (1, 8), (2, 2), (66, 66)]
NAN = float('nan')


def _interior_x(i, w):
    return 0 < i % w < w - 1


def _planted_maxima(h, w):
    """Flat indices to plant a lone maximum at.  The decoded row is `idx // h` (util.py:161), not `idx // w`: on a wide
    map it reaches and passes h - 1 (the `yi < h - 1` guard is all that keeps the neighbour reads inside the row), on a
    tall map it is an interior row while the pixel lies in the last one."""
    hw = h * w
    idx = {0, hw - 1, hw // 2, (h - 1) * w + w // 2}
    if w > h:
        idx.add(next(i for i in range(h * (h - 1), hw) if _interior_x(i, w)))          # idx // h == h - 1
        idx.update(i for i in (h * h + 1, h * h + 2, hw - 2) if i < hw and _interior_x(i, w))   # idx // h > h - 1
    return sorted(i for i in idx if 0 <= i < hw)


# (first, second) flat indices of two equal maxima.  Thread t reads t, t + 256, ...; a wave is 64 threads: 70 | 259 sit in
# waves 1 | 0 and trips 0 | 1, 130 | 300 in waves 2 | 0, 3 | 259 in one thread, 197 | 257 in waves 3 | 0 (the four-wave
# merge meets the later index first), 5 | 70 and 9 | 40 are for the maps below 256 pixels.
_TIES = [(70, 259), (130, 300), (3, 259), (197, 257), (1000, 4000), (5, 70), (9, 40), (1, 2)]


def _equal_neighbours_index(h, w):
    """A flat index whose decoded pixel (i % w, i // h) is interior and whose true pixel (i % w, i // w) is none of that
    pixel's four neighbours, so that planting them leaves the maximum alone; the middle pixel where there is none."""
    ok = [i for i in range(h * w) if _interior_x(i, w) and 0 < i // h < h - 1 and abs(i // w - i // h) != 1]
    return ok[len(ok) // 2] if ok else (h // 2) * w + w // 2


def _decode_rows(h, w):
    """[1, R, h, w] planted rows first, random rows last, and what each row is."""
    hw = h * w
    g = torch.Generator().manual_seed(h * 100 + w)
    rows, what = [], []

    def add(r, name):
        rows.append(r.reshape(h, w))
        what.append(name)
    for i in _planted_maxima(h, w):
        r = torch.randn(hw, generator=g)
        r[i] = 50.0
        add(r, 'max at %d' % i)
    for a, b in _TIES:
        if b < hw:
            r = torch.randn(hw, generator=g)
            r[a] = r[b] = 50.0
            add(r, 'tie %d %d' % (a, b))
    # equal neighbours (sign 0) around the DECODED pixel (x = i % w, y = i // h)
    i = _equal_neighbours_index(h, w)
    r = torch.zeros(h, w)
    r.view(-1)[i] = 50.0
    x, y = i % w, i // h
    if 0 < x < w - 1 and 0 < y < h - 1:
        r[y, x - 1] = r[y, x + 1] = 1.0
        r[y - 1, x] = r[y + 1, x] = 2.0
    add(r, 'equal neighbours at %d' % i)
    add(torch.zeros(hw), 'all zero')
    add(-torch.randn(hw, generator=g).abs() - 1, 'all negative')
    add(torch.full((hw,), float('-inf')), 'all -inf')
    # NaN rows: the finite maximum sits in the middle
    mid = hw // 2
    for name, nans in (('NaN before the maximum', [0] if mid > 0 else []), ('NaN after the maximum', [hw - 1]),
                       ('two NaNs', [hw - 1, min(hw - 1, mid + 1)]), ('NaN in another wave', [min(hw - 1, 200)])):
        r = torch.randn(hw, generator=g)
        r[mid] = 50.0
        r[nans] = NAN
        add(r, name)
    add(torch.full((hw,), NAN), 'all NaN')
    for k in range(8):
        add(torch.randn(hw, generator=g), 'random %d' % k)
    return torch.stack(rows)[None], what


def test_decode_cases_hold_what_they_claim():
    """The planted indices above do land where the comments say, for the shapes they are meant for."""
    for h, w in ((5, 9), (12, 20), (1, 8)):
        ys = [i // h for i in _planted_maxima(h, w) if _interior_x(i, w)]
        assert (h - 1 in ys or h == 1) and any(y > h - 1 for y in ys), (h, w, ys)
    for h, w in ((9, 5), (16, 12)):
        i = (h - 1) * w + w // 2
        assert i in _planted_maxima(h, w) and 0 < i // h < h - 1 and i // w == h - 1 and _interior_x(i, w)
    assert sum(b < 66 * 66 for _, b in _TIES) == len(_TIES) and sum(b < 12 * 20 for _, b in _TIES) >= 3
    for h, w in DECODE_SHAPES:          # sign 0 in x and in y wherever the map has an interior pixel, square or not
        hm, what = _decode_rows(h, w)
        i = _equal_neighbours_index(h, w)
        r = hm[0, what.index('equal neighbours at %d' % i)]
        x, y = i % w, i // h
        assert r.argmax().item() == i and r.max().item() == 50.0
        if min(h, w) >= 3:
            assert r[y, x - 1] == r[y, x + 1] == 1.0 and r[y - 1, x] == r[y + 1, x] == 2.0, (h, w, i)


@pytest.mark.parametrize('H,W', DECODE_SHAPES)
def test_decode_matches_oracle_off_the_square_map(dev, H, W):
    from dsnt import util as du
    from dsnt_oracle import util as ou
    hm, what = _decode_rows(H, W)
    for nb in (True, False):
        want = ou.decode_heatmaps(hm, use_neighbours=nb)
        got = du.decode_heatmaps(hm.to(dev), use_neighbours=nb).cpu()
        bad = (got != want).any(-1)[0].nonzero().flatten().tolist()
        for r in bad:
            print('%dx%d nb=%d row %d (%s): got %s want %s' % (H, W, nb, r, what[r], got[0, r].tolist(), want[0, r].tolist()))
        assert torch.equal(got, want), [what[r] for r in bad]
    assert torch.equal(du.get_preds(hm.to(dev)).cpu(), ou.get_preds(hm))


def test_decode_known_answers_off_the_square_map(dev):
    """The hand-derived answers of tests/test_oracle_known_answers.py, through the device."""
    from dsnt import util as du

    def one(h, w, cells):
        hm = torch.zeros(1, 1, h, w)
        for (r, c), v in cells.items():
            hm[0, 0, r, c] = v
        return hm.to(dev)
    ulp2 = 2.4e-7
    hm = one(5, 9, {(3, 7): 9.0})                                # idx 34: x = 34 % 9 = 7, y = 34 // 5 = 6
    assert du.get_preds(hm).cpu().tolist() == [[[7.0, 6.0]]]
    for nb in (True, False):
        got = du.decode_heatmaps(hm, use_neighbours=nb).cpu()
        assert (got - torch.tensor([[[7.5 * 2 / 9 - 1, 6.5 * 2 / 5 - 1]]])).abs().max().item() <= ulp2
    hm = one(9, 5, {(7, 2): 9.0, (4, 3): 1.0, (3, 2): 2.0})      # idx 37: x = 2, y = 37 // 9 = 4; neighbours of ROW 4
    assert du.get_preds(hm).cpu().tolist() == [[[2.0, 4.0]]]
    got = du.decode_heatmaps(hm, use_neighbours=False).cpu()
    assert (got - torch.tensor([[[0.0, 0.0]]])).abs().max().item() <= ulp2
    got = du.decode_heatmaps(hm, use_neighbours=True).cpu()
    assert (got - torch.tensor([[[2.75 * 2 / 5 - 1, 4.25 * 2 / 9 - 1]]])).abs().max().item() <= ulp2
    hm = one(6, 6, {(2, 3): NAN, (4, 4): 50.0})                  # torch.max: NaN is the maximum -> pixel (0, 0)
    assert du.get_preds(hm).cpu().tolist() == [[[0.0, 0.0]]]
    for nb in (True, False):
        got = du.decode_heatmaps(hm, use_neighbours=nb).cpu()
        print('NaN map decodes to', got.tolist())
        assert (got - torch.tensor([[[-5 / 6, -5 / 6]]])).abs().max().item() <= ulp2


def test_encode_known_answers_off_the_square_map(dev):
    import math
    from dsnt import util as du
    # target, bump centre, window columns and rows on a 5 x 9 map: derived in tests/test_oracle_known_answers.py
    cases = [((-1.0, 1.0), (0, 4), range(0, 4), range(1, 5)), ((0.0, 0.0), (4, 2), range(1, 8), range(0, 5)),
             ((1.2, 0.0), (9, 2), range(6, 9), range(0, 5)), ((2.0, 0.0), (13, 2), range(0, 0), range(0, 0))]
    got = du.encode_heatmaps(torch.tensor([[list(c[0]) for c in cases]], device=dev), 9, 5).cpu()
    assert got.shape == (1, 4, 5, 9)
    for j, (_, (cx, cy), cols, rows) in enumerate(cases):
        want = torch.zeros(5, 9)
        for r in rows:
            for c in cols:
                want[r, c] = math.exp(-((c - cx) ** 2 + (r - cy) ** 2) / 2)
        assert torch.equal(got[0, j] != 0, want != 0), j
        assert (got[0, j] - want).abs().max().item() <= 1e-6, j


# ------------------------------------------------------------------ encode and the MSE loss, row by row
MSE_SHAPES = [(64, 64, 1.0), (7, 7, 1.0), (4, 4, 1.0), (5, 9, 1.25), (28, 28, 2.0), (17, 15, 1.0), (16, 16, 1.0)]
TRAINED_NOISE = 1e-3


def _pixel_to_coord(p, size):
    return (p + 0.5) * 2.0 / size - 1.0


def _mse_targets(h, w):
    """[2, 16, 2]: 18 planted targets and 14 uniform ones (some off the map), as (x, y)."""
    mx, my = _pixel_to_coord(w // 2, w), _pixel_to_coord(h // 2, h)
    t = [(_pixel_to_coord(x, w), _pixel_to_coord(y, h)) for x in (0, w - 1) for y in (0, h - 1)]       # corner pixels
    for d in (3, 4):           # 3 px outside: the window is one column or row; 4 px outside (> 3.5): skipped
        t += [(_pixel_to_coord(-d, w), my), (_pixel_to_coord(w - 1 + d, w), my),
              (mx, _pixel_to_coord(-d, h)), (mx, _pixel_to_coord(h - 1 + d, h))]
    t += [(0.0, 0.0), (-1.0, 1.0)]                                                                 # .5 pixel ties
    t += [(1.15, 1.15), (-1.15, -1.15), (1.15, -1.15), (-1.15, 0.3)]
    rest = synthetic.tensor('hm.rows%dx%d' % (h, w), (32 - len(t), 2), seed=25, kind='uniform') * 1.15
    return torch.cat([torch.tensor(t, dtype=torch.float32), rest]).view(2, 16, 2)


@pytest.fixture(scope='module')
def mse_cases():
    """Per shape: targets, the oracle's encoding of them, and the two kinds of heat-map (computed once, left alone)."""
    from dsnt_oracle import util as ou
    out = {}
    for h, w, sigma in MSE_SHAPES:
        g = torch.Generator().manual_seed(h * 100 + w)
        t = _mse_targets(h, w)
        enc = ou.encode_heatmaps(t, w, h, sigma)
        out[h, w] = {'target': t, 'enc': enc, 'random': torch.randn(2, 16, h, w, generator=g) * 0.2,
                     'trained': enc + TRAINED_NOISE * torch.randn(2, 16, h, w, generator=g)}
    return out


def test_mse_targets_hold_what_they_claim(mse_cases):
    """Per shape: four corner bumps, four bumps clipped to one column or row, four skipped at 4 px, by the oracle."""
    for (h, w), c in mse_cases.items():
        nz = (c['enc'].view(32, h, w) != 0)
        assert all(nz[k].any() for k in range(4))
        for k, axis in ((4, 0), (5, 0), (6, 1), (7, 1)):              # x outside: one column; y outside: one row
            assert nz[k].any() and nz[k].any(axis).sum().item() == 1, (h, w, k)
        assert not nz[8:12].any()


@pytest.mark.parametrize('H,W,sigma', MSE_SHAPES)
def test_encode_planted_targets(dev, mse_cases, H, W, sigma):
    from dsnt import util as du
    c = mse_cases[H, W]
    got = du.encode_heatmaps(c['target'].to(dev), W, H, sigma).cpu()
    assert (got - c['enc']).abs().max().item() <= 1e-6
    assert torch.equal(got == 0, c['enc'] == 0)


@pytest.mark.parametrize('kind', ['random', 'trained'])
@pytest.mark.parametrize('H,W,sigma', MSE_SHAPES)
def test_mse_rows_and_gradient(dev, mse_cases, H, W, sigma, kind):
    """per_row, the total and the gradient of every row against the oracle's encoding taken to fp64.

    Bars: 1e-5 relative for per_row (with a floor of 1e-7 absolute on the trained maps, where a row's loss is about
    H W 1e-6 and the bump's own fp32 rounding is all there is left) and for the total; 1e-5 of a row's largest entry for
    the gradient.  Plain fp32 ATen on these inputs is within 1.7e-7 relative of fp64 per row (a margin of 61)."""
    from dsnt import util as du
    from dsnt._lib import call, ptr
    c = mse_cases[H, W]
    hm, t, enc = c[kind], c['target'], c['enc']
    diff = hm.double() - enc.double()
    want_rows = (diff ** 2).sum((-1, -2)).view(32)
    want_loss = want_rows.sum().item() / hm.numel()
    x, td = hm.to(dev), t.to(dev)
    per_row = torch.empty(32, device=dev)
    call('dsnt_heatmap_mse_fwd', ptr(x), ptr(td), ptr(per_row), 32, H, W, float(sigma))
    err = (per_row.cpu().double() - want_rows).abs()
    bar = 1e-5 * want_rows
    if kind == 'trained':
        bar = bar.clamp_min(1e-7)
    k = int((err - bar).argmax())
    print('%dx%d %s per_row: worst row %d err %.3e bar %.3e (rel %.3e)' % (H, W, kind, k, err[k], bar[k],
                                                                             (err / want_rows).max()))
    assert (err <= bar).all(), (k, err[k].item(), bar[k].item())
    xg = x.clone().requires_grad_()
    loss = du.heatmap_mse_loss(xg, td, sigma)
    print('%dx%d %s loss: %.9e want %.9e rel %.3e' % (H, W, kind, loss.item(), want_loss,
                                                      abs(loss.item() - want_loss) / want_loss))
    assert abs(loss.item() - want_loss) <= 1e-5 * want_loss
    for gscale in (3.0, -0.75):
        want_g = (gscale * 2.0 / hm.numel() * diff).view(32, -1)
        gs = torch.tensor([gscale], device=dev)
        dhm = torch.empty_like(x)
        call('dsnt_heatmap_mse_bwd', ptr(x), ptr(td), ptr(gs), ptr(dhm), 32, H, W, float(sigma))
        gerr = (dhm.cpu().double().view(32, -1) - want_g).abs().amax(-1)
        gbar = 1e-5 * want_g.abs().amax(-1)
        k = int((gerr / gbar).argmax())
        print('%dx%d %s gradient x %g: worst row %d err %.3e bar %.3e' % (H, W, kind, gscale, k, gerr[k], gbar[k]))
        assert (gerr <= gbar).all(), (gscale, k, gerr[k].item(), gbar[k].item())
        xg.grad = None
        (du.heatmap_mse_loss(xg, td, sigma) * gscale).backward()
        assert torch.equal(xg.grad, dhm)
