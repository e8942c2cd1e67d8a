"""HIP DSNT head against the fp64 oracle on trained-regime heat-maps and on the dispatch paths no other test reaches.

Inputs, oracle runners and the yardstick are tests/head_regimes.py: seven regimes (diffuse, peaked, edge, onehot, bimodal,
offset, straddle) x ten shapes (fast JS form, per-slot JS, VEC == 1, tab == false, > 4096 pixels) x reg none / js / kl /
mse / var x with and without a mask, 64 rows each.  The logit gradient is measured as
ratio_r = max_i |g_i - g64_i| / (2^-24 S_r).  K_ref[reg] is the worst ratio of the fp32 oracle over the same matrix,
taken in the same run (both oracles on the CPU), and the HIP path must stay within 4 K_ref[reg].  The two wide maps set
K_ref; every other shape is held to 4 K_narrow[reg], the same figure over the matrix without them (`_bound`).  Values
keep the suite's bounds: coords 2e-6, heat-maps 2e-6 with row sums within 1e-5, dist / reg_row / loss
1e-5 max(1, |value|).

MEASURED (MI355X; worst ratio over masks and routes per regulariser and regime: the eight narrow shapes, and as edge*
the edge regime on the two wide maps, which sets K_ref; each cell fp32 oracle / HIP) -- see DESIGN.md section 13:
  reg   K_narrow/bound  K_ref/bound | diffuse     peaked      edge        edge*       onehot      bimodal     offset      straddle
  none    45.2 / 181     287.6 / 1150 | 22.7/12.6   45.2/35.9   30.6/18.1   288/330     0/0         34.7/17.6   25.6/7.93   43.7/43.7
  js      44.1 / 176     239.2 / 957  | 44.1/22.6   13.4/37.6   23.4/43.6   239/276     0/0         18.5/26.9   13.5/44.4   28.1/27.9
  kl      45.6 / 182      45.6 / 182  | 45.6/7.08   4.57/27.9   4.61/50.4   4.6/5.4     0/0         3.6/6.19    39.2/17.5   6.8/14.9
  mse     53.5 / 214     188.1 / 752  | 53.5/25.4   40.4/48.9   21.9/25     188/216     0/0         31.5/19.9   26.7/30.2   43.9/25.3
  var     53.7 / 215      81.4 / 326  | 44.7/22     29.2/39.3   37.6/21.3   81.4/28.1   0/0         10.3/16     53.7/27.5   37.8/23.2
  Value errors stay below 0.1 of their bounds everywhere (coords, heat-maps, dist, reg_row, loss).  On the wide maps
  dist is down to 1.3e-3.  4096 rows: worst |row sum| = 73.5 x 2^-24 S_r, 0.033 of the tighter bound of that test.

SENSITIVITY (a scratch copy of head_loss.hip with one change, built into a library outside the tree, one run each through
tools/mutate_head.py; nothing of it is committed):
  (a) `far` 1e-30f -> 1e-12f: NOT caught, 167 passed, worst ratio / bound 0.29 as without the change.  It cannot be
      caught in fp32: where the shortcut now fires wrongly, d reg / d p is off by (1/2) ln(1 + q / p) and
      p ln(1 + q / p) <= q < 1e-12, so a gradient moves by at most 1e-12 w_row: at most 8e-4 of 2^-24 S_r on the rows
      of 64x64, 28x28 and 16x16 (fp64 evaluation of the kernel's formula with both thresholds); reg_row loses
      sum q |log q - log m| <= 256 x 1e-12 x 40 = 1e-8 per wave, below one ulp of its ~0.5.  A threshold
      of 1e-12 would be as exact as 1e-30; no bound that fp32 can meet tells them apart.
  (b) `elem` without `- m * rcp(m + REG_EPS)`: caught, 5 failed: test_fused_route[64-64-js], [64-48-js], [28-28-js] and
      test_misaligned_base_pointers[64-64-js], [28-28-js] (its aligned control); ratio up to 1.2e7 = 6.9e4 x bound
      (28x28 edge), 9.2e3 x bound at 64x64 (straddle).  Not at 16x16, 14x14 or VEC == 1: a row that takes `elem` for
      every pixel only gains a constant in dL/dp, which the softmax backward removes.
  (c) x and y exchanged where tab == false: caught, 15 failed: test_fused_route[4-1024-*] and [8-512-*] for all five
      regularisers and test_single_row[4-1024-*]; ratio 1.8e4 to 3.2e4 x bound.  No test of another shape fails.
"""
import functools

import numpy as np
import pytest
import torch

import head_regimes as hr

pytestmark = pytest.mark.gpu

FACTOR = 4.0                                     # HIP ratio <= FACTOR * K_ref[reg]
UNFUSED_SHAPES = ((64, 64), (7, 7))
DEV = 'cuda:0'


def _f64(t, *shape):
    return t.detach().double().cpu().reshape(*shape).numpy()


def _hip_public(x, t, m, reg, sigma, coeff, unfused):
    """The public routes.  fused: dn.head_forward + dn.head_loss, first backward (dsnt_head_loss_grad; above 4096
    pixels dsnt_head_loss_rows + dsnt_head_bwd); second: a second backward through the same graph (dsnt_head_bwd);
    unfused: dn.hm_preact -> dn.dsnt -> dn.euclidean_loss + dn.*_reg_loss."""
    import dsnt.nn as dn
    rows = x.shape[0]
    td, md = t.to(DEV), None if m is None else m.to(DEV)
    ld = x.to(DEV).requires_grad_()
    hm, co = dn.head_forward(ld)
    loss = dn.head_loss(ld, hm.detach(), co.detach(), td, md, reg, sigma, coeff)
    g1, = torch.autograd.grad(loss, ld, retain_graph=True)
    g2, = torch.autograd.grad(loss, ld)
    out = {'fused': dict(coords=_f64(co, rows, 2), p=_f64(hm, rows, -1), loss=float(loss.detach()), g=_f64(g1, rows, -1)),
           'second': dict(g=_f64(g2, rows, -1))}
    if unfused:
        lu = x.to(DEV).requires_grad_()
        hmu = dn.hm_preact(lu, 'softmax')
        cou = dn.dsnt(hmu)
        lossu = dn.euclidean_loss(cou, td, md)
        if reg != 'none':
            fn = {'js': dn.js_reg_loss, 'kl': dn.kl_reg_loss, 'mse': dn.mse_reg_loss, 'var': dn.variance_reg_loss}[reg]
            lossu = lossu + coeff * fn(hmu, td, sigma, md)
        gu, = torch.autograd.grad(lossu, lu)
        out['unfused'] = dict(coords=_f64(cou, rows, 2), p=_f64(hmu, rows, -1), loss=float(lossu.detach()),
                              g=_f64(gu, rows, -1))
    return out


def _shifted(n, shift):
    """A contiguous view of n floats starting `shift` floats into a zeroed buffer, and the buffer (its other elements
    are canaries: they must still be zero afterwards)."""
    buf = torch.zeros(n + 8, device=DEV)
    v = buf[shift:shift + n]
    assert v.data_ptr() % 16 == 4 * (shift % 4)
    return v, buf


def _hip_cabi(x, t, m, reg, sigma, coeff, shift=0):
    """The C ABI with logits, heat-maps and both gradients `shift` floats off a 16-byte boundary: dsnt_head_fwd,
    dsnt_head_loss_grad (per-row dist / reg_row and the gradient), dsnt_head_loss_reduce, then dsnt_head_loss_rows +
    dsnt_masked_avg_bwd + dsnt_head_bwd on the same heat-maps."""
    import dsnt.nn as dn
    from dsnt._lib import call, ptr
    rows, h, w = x.shape[0], x.shape[-2], x.shape[-1]
    n = rows * h * w
    kind = dn.REG_KINDS.get(reg, -1)
    (lg, b0), (hm, b1), (g0, b2), (gb, b3) = (_shifted(n, shift) for _ in range(4))
    lg.copy_(x.flatten().to(DEV))
    td = t.to(DEV).contiguous()
    md = None if m is None else m.to(DEV).contiguous()
    new = lambda k: torch.empty(k, device=DEV)
    coords, dist, dist2, out, out2, g_dist = new(rows * 2), new(rows), new(rows), new(3), new(3), new(rows)
    regr, regr2 = (new(rows), new(rows)) if kind >= 0 else (None, None)
    call('dsnt_head_fwd', ptr(lg), ptr(hm), ptr(coords), rows, h, w)
    den = dn.mask_denominator(md, rows, torch.device(DEV))
    res = {}
    if h * w <= 4096:
        call('dsnt_head_loss_grad', ptr(hm), ptr(coords), ptr(td), ptr(md), ptr(den), ptr(dist), ptr(regr), ptr(g0),
             rows, h, w, sigma, kind, coeff)
        call('dsnt_head_loss_reduce', ptr(dist), ptr(regr), ptr(md), ptr(den), coeff, ptr(out), ptr(out[1:]), rows)
        res['grad'] = dict(coords=_f64(coords, rows, 2), p=_f64(hm, rows, -1), dist=_f64(dist, rows),
                           reg_row=None if regr is None else _f64(regr, rows), loss=float(out[0]), g=_f64(g0, rows, -1))
    call('dsnt_head_loss_rows', ptr(hm), ptr(coords), ptr(td), ptr(dist2), ptr(regr2), rows, h, w, sigma, kind)
    call('dsnt_head_loss_reduce', ptr(dist2), ptr(regr2), ptr(md), ptr(den), coeff, ptr(out2), ptr(out2[1:]), rows)
    call('dsnt_masked_avg_bwd', ptr(torch.ones(1, device=DEV)), ptr(md), ptr(out2[1:]), ptr(g_dist), rows)
    g_reg = (g_dist * coeff) if kind >= 0 else None
    call('dsnt_head_bwd', ptr(hm), ptr(coords), ptr(td), ptr(dist2), ptr(g_dist), ptr(g_reg), ptr(gb), rows, h, w,
         sigma, kind)
    res['rows_bwd'] = dict(coords=_f64(coords, rows, 2), p=_f64(hm, rows, -1), dist=_f64(dist2, rows),
                           reg_row=None if regr2 is None else _f64(regr2, rows), loss=float(out2[0]), g=_f64(gb, rows, -1))
    torch.cuda.synchronize()
    for b in (b0, b1, b2, b3):                                           # nothing written outside the views
        assert float(b[:shift].abs().sum()) == 0.0 and float(b[shift + n:].abs().sum()) == 0.0
    return res


def _figures(got, o64, S):
    """{'ratio': worst ratio_r, value errors / bound ...} of one route's output against the fp64 oracle."""
    fig = {'ratio': float(hr.ratio_rows(got['g'], o64['g'], S).max())}
    if 'coords' in got:
        full = dict(got)
        full.setdefault('dist', o64['dist'])
        fig.update(hr.value_errors(full, o64))
        if 'dist' not in got:
            del fig['dist']
    return fig


@functools.lru_cache(maxsize=None)
def _sweep(reg):
    """The whole matrix for one regulariser: (K_ref, {(h, w): {(regime, use_mask): {route: figures}}}).  K_ref needs
    every shape, so the first test of a regulariser runs them all and the others read the result."""
    k_ref, res = 0.0, {}
    coeff = hr.coeff_of(reg)
    for regime, h, w, use_mask in hr.matrix():
        x, t, m = hr.make(regime, h, w)
        m = m if use_mask else None
        sigma = hr.sigma_of(h, w)
        o64 = hr.oracle(x, t, m, reg, sigma, coeff, torch.float64)
        o32 = hr.oracle(x, t, m, reg, sigma, coeff, torch.float32)
        S = hr.scale_rows(o64['p'], o64['v'])
        ref = float(hr.ratio_rows(o32['g'], o64['g'], S).max())
        k_ref = max(k_ref, ref)
        hip = _hip_public(x, t, m, reg, sigma, coeff, (h, w) in UNFUSED_SHAPES)
        hip['rows'] = _hip_cabi(x, t, m, reg, sigma, coeff)['rows_bwd']    # dist / reg_row of dsnt_head_loss_rows
        figs = {route: _figures(got, o64, S) for route, got in hip.items()}
        figs['ref'] = {'ratio': ref}
        res.setdefault((h, w), {})[(regime, use_mask)] = figs
    return k_ref, res


WIDE = ((4, 1024), (8, 512))


def _bound(reg, h, w):
    """(K, FACTOR * K) for a shape.  The issue's K_ref[reg] is the fp32 oracle's worst ratio over the whole matrix; it is
    set by the two wide maps (dist = 1.3e-3 on a 1024-wide map), and fp32 is 5 to 20 times better on every other shape.
    So that the other shapes do not borrow their allowance from an unrelated one, they are held to the same construction
    over the matrix without the wide maps, K_narrow[reg] <= K_ref[reg]; the wide maps keep K_ref[reg]."""
    k_ref, res = _sweep(reg)
    if (h, w) in WIDE:
        return k_ref, FACTOR * k_ref
    k = max(f['ref']['ratio'] for shape, cases in res.items() if shape not in WIDE for f in cases.values())
    assert k <= k_ref
    return k, FACTOR * k


def _check(reg, h, w, routes):
    _, res = _sweep(reg)
    k_ref, bound = _bound(reg, h, w)
    bad = []
    for regime in hr.REGIMES:
        line = []
        for route in routes:
            figs = [res[(h, w)][(regime, um)][route] for um in (True, False) if route in res[(h, w)][(regime, um)]]
            if not figs:
                continue
            worst = {k: max(f[k] for f in figs) for k in figs[0]}
            line.append('%s %s' % (route, ' '.join('%s=%.3g' % kv for kv in worst.items())))
            if route == 'ref':
                continue
            if not worst['ratio'] <= bound:
                bad.append((regime, route, 'ratio', worst['ratio'], bound))
            bad += [(regime, route, k, v) for k, v in worst.items() if k != 'ratio' and not v <= 1.0]
        print('%dx%d %-4s %-8s K_ref=%.1f | %s' % (h, w, reg, regime, k_ref, ' | '.join(line)))
    assert not bad, bad


@pytest.mark.parametrize('reg', hr.REGS)
@pytest.mark.parametrize('h,w', hr.SHAPES)
def test_fused_route(h, w, reg):
    """dn.head_forward + dn.head_loss(...).backward(): coords, heat-maps, loss by the value bounds (printed as
    error / bound), the logit gradient by the yardstick."""
    _check(reg, h, w, ('ref', 'fused'))


@pytest.mark.parametrize('reg', hr.REGS)
@pytest.mark.parametrize('h,w', hr.SHAPES)
def test_loss_rows_and_head_bwd_route(h, w, reg):
    """dsnt_head_bwd by a second backward through the same graph, and dsnt_head_loss_rows + dsnt_head_bwd through the
    C ABI (per-row dist and reg_row as well), on the same inputs."""
    _check(reg, h, w, ('second', 'rows'))


@pytest.mark.parametrize('reg', hr.REGS)
@pytest.mark.parametrize('h,w', UNFUSED_SHAPES)
def test_unfused_public_route(h, w, reg):
    _check(reg, h, w, ('unfused',))


@pytest.mark.parametrize('h,w', [(64, 64), (28, 28), (16, 16)])
def test_census_on_device_heatmaps(h, w):
    """The JS branches the kernel takes on these inputs, counted from the heat-maps the device wrote."""
    import dsnt.nn as dn
    total = {}
    for regime in hr.REGIMES:
        x, t, _ = hr.make(regime, h, w)
        hm, _ = dn.head_forward(x.to(DEV))
        c = hr.census_counts(*hr.census(hm.cpu().reshape(hr.ROWS, -1).numpy(), t.numpy(), h, w, hr.sigma_of(h, w)))
        print('census %dx%d %-8s %s' % (h, w, regime, c))
        for k, n in c.items():
            total[k] = total.get(k, 0) + n
    print('census %dx%d total    %s' % (h, w, total))
    assert total['general'] >= 32 and total['mixed'] >= 32, total


@pytest.mark.parametrize('reg', ['js', 'kl'])
@pytest.mark.parametrize('h,w', [(64, 64), (28, 28)])
def test_misaligned_base_pointers(h, w, reg):
    """Logits, heat-maps and gradients one float off a 16-byte boundary: ROW_DISPATCH and dsnt_head_loss_grad drop to
    VEC == 1 on shapes that otherwise always run VEC == 4.  Same bounds; the aligned call beside it as a control."""
    _, bound = _bound(reg, h, w)
    bad = []
    for regime in hr.REGIMES:
        x, t, m = hr.make(regime, h, w)
        sigma = hr.sigma_of(h, w)
        o64 = hr.oracle(x, t, m, reg, sigma, 1.0)
        S = hr.scale_rows(o64['p'], o64['v'])
        for shift in (1, 0):
            for route, got in _hip_cabi(x, t, m, reg, sigma, 1.0, shift).items():
                fig = _figures(got, o64, S)
                print('%dx%d %s %-8s shift=%d %-8s %s' % (h, w, reg, regime, shift, route,
                                                          ' '.join('%s=%.3g' % kv for kv in fig.items())))
                if not fig['ratio'] <= bound:
                    bad.append((regime, shift, route, 'ratio', fig['ratio']))
                bad += [(regime, shift, route, k, v) for k, v in fig.items() if k != 'ratio' and not v <= 1.0]
    assert not bad, bad


@pytest.mark.parametrize('reg', hr.REGS)
@pytest.mark.parametrize('h,w', [(64, 64), (14, 14), (7, 7), (8, 512), (96, 96)])
def test_mask_edges(h, w, reg):
    """Peaked rows.  A row with mask 0 has a gradient of exactly 0.0 everywhere; an all-zero mask gives a loss of
    exactly 0 and an all-zero gradient through the clamp(sum, 1) denominator.  Both routes."""
    x, t, m = hr.make('peaked', h, w)
    assert 0 < int((m == 0).sum()) < m.numel()
    coeff, sigma = hr.coeff_of(reg), hr.sigma_of(h, w)
    off = (m.flatten() == 0).numpy()
    hip = _hip_public(x, t, m, reg, sigma, coeff, True)
    hip.update(_hip_cabi(x, t, m, reg, sigma, coeff))
    for route, got in hip.items():
        assert np.isfinite(got['g']).all(), route
        assert np.abs(got['g'][off]).max() == 0.0, route
        assert np.abs(got['g'][~off]).max() > 0.0, route
    zero = torch.zeros_like(m)
    hip = _hip_public(x, t, zero, reg, sigma, coeff, True)
    hip.update(_hip_cabi(x, t, zero, reg, sigma, coeff))
    for route, got in hip.items():
        assert np.abs(got['g']).max() == 0.0, route
        if 'loss' in got:
            assert got['loss'] == 0.0, route


@pytest.mark.parametrize('reg', hr.REGS)
@pytest.mark.parametrize('h,w', [(64, 64), (7, 7), (4, 1024), (96, 96)])
def test_single_row(h, w, reg):
    _, bound = _bound(reg, h, w)
    bad = []
    for regime in ('peaked', 'edge', 'onehot'):
        x, t, m = hr.make(regime, h, w, rows=1)
        coeff, sigma = hr.coeff_of(reg), hr.sigma_of(h, w)
        o64 = hr.oracle(x, t, None, reg, sigma, coeff)
        assert o64['dist'].min() > 1e-4
        S = hr.scale_rows(o64['p'], o64['v'])
        hip = _hip_public(x, t, None, reg, sigma, coeff, True)
        hip.update(_hip_cabi(x, t, None, reg, sigma, coeff))
        for route, got in hip.items():
            fig = _figures(got, o64, S)
            print('%dx%d %s %-8s rows=1 %-8s %s' % (h, w, reg, regime, route, ' '.join('%s=%.3g' % kv for kv in fig.items())))
            if not fig['ratio'] <= bound:
                bad.append((regime, route, 'ratio', fig['ratio']))
            bad += [(regime, route, k, v) for k, v in fig.items() if k != 'ratio' and not v <= 1.0]
    assert not bad, bad


@pytest.mark.parametrize('rows', [1, 3])
@pytest.mark.parametrize('h,w', [(7, 7), (5, 5)])
def test_upstream_gradient_on_odd_element_counts(h, w, rows):
    """An upstream gradient other than 1 rescales the fused gradient in place (dsnt_scale_by_scalar): 49 or 147 logits
    are not a multiple of four floats.  One rounding per element, so equal to the product bit for bit."""
    import dsnt.nn as dn
    x, t, _ = hr.make('peaked', h, w, rows=rows)

    def grad(up):
        ld = x.to(DEV).requires_grad_()
        hm, co = dn.head_forward(ld)
        loss = dn.head_loss(ld, hm.detach(), co.detach(), t.to(DEV), None, 'js', hr.sigma_of(h, w), 1.0)
        return torch.autograd.grad(loss * up, ld)[0]
    g1 = grad(1.0)
    assert float(g1.abs().max()) > 0
    assert torch.equal(grad(-0.75), g1 * -0.75)


def test_4096_rows_properties():
    """4096 peaked rows at 64x64, JS: finite; every row's gradient sums to 0 within 2^-24 (32 sum_i |p_i v_i| +
    256 |sum_i p_i v_i|); rows 1000..1063 equal the same 64 rows run alone, bit for bit (same denominator).

    The row-sum bound, by reasoning, independent of the number of rows: sum_i g_i = sum_i p_i v_i - s sum_i p_i with s
    the kernel's sum_j p_j v_j.  Each g_i is a rounded product with a rounded difference (2 ulp of |p_i v_i| + p_i |s|),
    s carries the error of a 16-per-thread chain and an 8-level tree (<= 24 ulp of sum |p v|), and the heat-map's row
    sum is within 1e-5 = 168 x 2^-24 of 1, which multiplies s."""
    import dsnt.nn as dn
    R, h, w, sigma = 4096, 64, 64, 2.0 / 64
    x, t, _ = hr.make('peaked', h, w, rows=R)
    den = dn.mask_denominator(None, 64, torch.device(DEV))

    def run(xs, ts):
        ld = xs.to(DEV).requires_grad_()
        hm, co = dn.head_forward(ld)
        loss = dn.head_loss(ld, hm.detach(), co.detach(), ts.to(DEV), None, 'js', sigma, 1.0, den)
        g, = torch.autograd.grad(loss, ld)
        return hm.detach(), g
    hm, g = run(x, t)
    assert torch.isfinite(g).all() and torch.isfinite(hm).all()
    hm_s, g_s = run(x[1000:1064], t[1000:1064])
    assert torch.equal(g[1000:1064], g_s) and torch.equal(hm[1000:1064], hm_s)
    o64 = hr.oracle(x, t, None, 'js', sigma, 1.0)
    v = o64['v'] * (R / 64.0)                         # the oracle averaged over 4096 rows, the device over 64
    pv = o64['p'] * v
    bound = hr.EPS24 * (32 * np.abs(pv).sum(-1) + 256 * np.abs(pv.sum(-1)))
    sums = np.abs(_f64(g, R, -1).sum(-1))
    print('4096 rows: worst |row sum| / bound = %.3g' % float((sums / bound).max()))
    assert (sums <= bound).all()
    # the same through S_r.  S_r holds max_i |p_i v_i|, not the sum over the hw pixels that the rounding errors of a row
    # sum add up over; sum_i |p_i v_i| <= hw max_i |p_i v_i| <= hw S_r and |sum p v| <= S_r / max p with max p >= 1 / hw,
    # so the factor that is rigorous for every row is (32 + 256) hw: it depends on the map, not on the number of rows
    S = hr.scale_rows(o64['p'], v)
    print('4096 rows: worst |row sum| / (2^-24 S_r) = %.3g' % float((sums / (hr.EPS24 * S)).max()))
    assert (sums <= hr.EPS24 * S * 288 * h * w).all()
