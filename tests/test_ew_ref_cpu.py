"""tests/ew_ref.py (the fp64 restatement of the element-wise kernels) pinned to the torch CPU operators, on the same
tie-heavy, NaN, -inf, ragged and guard inputs that tests/test_elementwise_edges_gpu.py feeds the HIP kernels.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ew_ref as R

POOL_SHAPES = [(1, 5), (7, 9), (2, 2), (16, 16), (12, 20)]


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2))))


def _same(a, b):
    """Equal, NaNs at the same places (signs of zero are compared by the GPU tests, bit for bit)."""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize('pool,hw', [(pl, hw) for pl in (2, 3) for hw in POOL_SHAPES if pl == 3 or (hw[0] % 2 == 0 and hw[1] % 2 == 0)])
@pytest.mark.parametrize('nan_tap', [None, 0, 1, 3, 8])
def test_pools_equal_aten(pool, hw, nan_tap):
    """Values, arg-max and the routed gradient == F.max_pool2d(return_indices=True) and its autograd on contiguous NCHW
    fp64: first maximum wins, the index starts at the first valid tap, NaN propagates, a -inf window keeps its first tap."""
    H, W = hw
    N, C = 3, 8
    x = R.tie_input(N, H, W, C, seed=H * 100 + W, pool=pool, nan_tap=nan_tap)
    y, k = (R.maxpool2 if pool == 2 else R.maxpool3s2)(x.astype(np.float64))
    xt = _nchw(x).double().requires_grad_()
    args = dict(kernel_size=2, stride=2) if pool == 2 else dict(kernel_size=3, stride=2, padding=1)
    yt, it = F.max_pool2d(xt, return_indices=True, **args)
    assert _same(np.transpose(y, (0, 3, 1, 2)), yt.detach().numpy())
    Ho, Wo = y.shape[1:3]
    oh, ow = np.arange(Ho)[None, :, None, None], np.arange(Wo)[None, None, :, None]
    kk = k.astype(np.int64)
    flat = ((2 * oh + kk // 2) * W + 2 * ow + kk % 2) if pool == 2 else ((2 * oh - 1 + kk // 3) * W + 2 * ow - 1 + kk % 3)
    assert np.array_equal(np.transpose(flat, (0, 3, 1, 2)), it.numpy())
    gy = R.int_grad(y.shape, seed=7)
    yt.backward(_nchw(gy).double())
    dx = R.maxpool2_bwd(gy, k) if pool == 2 else R.maxpool3s2_bwd(gy, k, H, W)
    assert np.array_equal(np.transpose(dx, (0, 3, 1, 2)), xt.grad.numpy())


@pytest.mark.parametrize('pool,hw', [(2, (12, 20)), (3, (1, 5)), (3, (7, 9)), (3, (16, 16))])
def test_tie_inputs_hold_ties(pool, hw):
    """At least a third of the windows of the inputs the GPU tie tests use hold their maximum more than once."""
    x = R.tie_input(3, hw[0], hw[1], 8, seed=hw[0] * 100 + hw[1], pool=pool, nan_tap=None)
    assert R.tie_share(x, pool) >= 1.0 / 3.0


@pytest.mark.parametrize('M,C', [(300, 80), (129, 8), (1000, 192), (2561, 128)])
@pytest.mark.parametrize('relu', [0, 1])
def test_batchnorm_equals_autograd(M, C, relu):
    """tile_sums -> statistics, bn_bwd_tile_sums -> coefficients, bn_apply == F.batch_norm (+ ReLU) and its autograd in fp64,
    outside the elements whose ReLU mask two correct programs may take differently."""
    x, gamma, beta, da = R.bn_case(M, C, seed=M + C)
    s1, s2, _, _ = R.tile_sums(x, M, C)
    mean, var = s1.sum(0) / M, s2.sum(0) / M - (s1.sum(0) / M) ** 2
    invstd = 1.0 / np.sqrt(var + 1e-5)
    scale = gamma.astype(np.float64) * invstd
    shift = beta.astype(np.float64) - mean * scale
    dead, und = R.relu_mask(x, scale, shift) if relu else (np.zeros(x.shape, bool), np.zeros(x.shape, bool))
    dz = np.where(dead, 0.0, da.astype(np.float64))
    d1, d2, _, _ = R.bn_bwd_tile_sums(dz, x, mean, invstd, M, C)
    coef = np.stack([d1.sum(0) / M, d2.sum(0) / M])
    dx, und2, _ = R.bn_apply(da, x, scale, shift, mean, invstd, coef, relu)
    assert np.array_equal(und, und2) and und.mean() <= 1e-3

    xt = torch.from_numpy(x).double().requires_grad_()
    gt, bt = torch.from_numpy(gamma).double().requires_grad_(), torch.from_numpy(beta).double().requires_grad_()
    yt = F.batch_norm(xt, None, None, gt, bt, True, 0.1, 1e-5)
    if relu:
        yt = F.relu(yt)
    yt.backward(torch.from_numpy(da).double())
    y = x * scale + shift
    if relu:
        y = np.maximum(y, 0.0)
        assert np.array_equal(dead[~und], (yt.detach().numpy() <= 0)[~und])
    assert np.abs(y - yt.detach().numpy()).max() <= 1e-12 * np.abs(y).max()
    want = xt.grad.numpy()
    assert np.abs(dx - want)[~und].max() <= 1e-11 * np.abs(want).max()
    assert np.abs(d2.sum(0) - gt.grad.numpy()).max() <= 1e-11 * np.abs(d2.sum(0)).max()
    assert np.abs(d1.sum(0) - bt.grad.numpy()).max() <= 1e-11 * max(1.0, np.abs(d1.sum(0)).max())


@pytest.mark.parametrize('M,C', [(163841, 64), (2561, 128), (350, 48), (100003, 48), (350, 80), (60003, 80)])
def test_undecidable_mask_share_of_the_gpu_cases(M, C):
    """The apply cases of the GPU module keep the undecidable-mask exclusion under 0.1 %, by the reference alone."""
    x, gamma, beta, _ = R.bn_case(M, C, seed=M + C)
    mu, is_, sc, sh = R.bn_vectors(x, gamma, beta)
    _, und = R.relu_mask(x, sc, sh)
    assert und.mean() <= 1e-3


def test_apply_and_sum_bounds_admit_plain_fp32():
    """The derived bars are no tighter than what a plain fp32 evaluation of the same expressions achieves against the fp64
    reference (torch CPU, fp32): they hold for it with nothing added."""
    M, C = 1000, 192
    x, gamma, beta, da = R.bn_case(M, C, seed=5)
    mu, is_, sc, sh = R.bn_vectors(x, gamma, beta)
    coef = (np.random.default_rng(1).standard_normal((2, C)) * 0.05).astype(np.float32)
    want, und, bound = R.bn_apply(da, x, sc, sh, mu, is_, coef, 0)
    t = {k: torch.from_numpy(v) for k, v in dict(x=x, da=da, mu=mu, is_=is_, sc=sc, c0=coef[0], c1=coef[1]).items()}
    got = (t['sc'] * (t['da'] - t['c0'] - (t['x'] - t['mu']) * t['is_'] * t['c1'])).double().numpy()
    assert (np.abs(got - want) <= bound).all()
    s1, s2, a1, a2 = R.tile_sums(x, M, C)
    n = R.tile_sum_ops(M, C)
    xt = torch.from_numpy(x)
    for t_ in range(s1.shape[0]):
        blk = xt[t_ * 128:(t_ + 1) * 128]
        assert (np.abs(blk.sum(0).double().numpy() - s1[t_]) <= R.gamma(n) * a1[t_]).all()
        assert (np.abs((blk * blk).sum(0).double().numpy() - s2[t_]) <= R.gamma(n) * a2[t_]).all()


def _h(v):
    return float(np.float32(v))


@pytest.mark.parametrize('wd', [0.0, 1e-4])
@pytest.mark.parametrize('gs', [1.0, 1.0 / 3.0])
def test_rmsprop_equals_torch(wd, gs):
    """Three steps == torch.optim.RMSprop in fp64 (grad_scale by scaling the gradient handed to torch); and ONE fp32 torch
    step from the same fp32 state stays inside bound_p / bound_sq."""
    n = 1003
    r = np.random.default_rng(11)
    p0 = r.standard_normal(n).astype(np.float32)
    grads = [(r.standard_normal(n) * (0.1 + i)).astype(np.float32) for i in range(3)]
    lr, alpha, eps = _h(2.5e-4), _h(0.99), _h(1e-8)
    pt = torch.from_numpy(p0).double().requires_grad_()
    opt = torch.optim.RMSprop([pt], lr=lr, alpha=alpha, eps=eps, weight_decay=_h(wd))
    p, sq = p0.astype(np.float64), np.zeros(n)
    for g in grads:
        pt.grad = torch.from_numpy(g).double() * _h(gs)
        opt.step()
        out = R.rmsprop_step(p, g, sq, lr, alpha, eps, wd, gs)
        p, sq = out['p'], out['sq']
        assert np.abs(p - pt.detach().numpy()).max() <= 1e-13
        assert np.abs(sq - opt.state[pt]['square_avg'].numpy()).max() <= 1e-13
    # fp32 torch, one step from an fp32 state with history
    p32, sq32 = p.astype(np.float32), sq.astype(np.float32)
    q = torch.from_numpy(p32.copy()).requires_grad_()
    o32 = torch.optim.RMSprop([q], lr=lr, alpha=alpha, eps=eps, weight_decay=_h(wd))
    q.grad = torch.from_numpy(grads[1]) * np.float32(gs)
    o32.step()                                     # creates the state
    o32.state[q]['square_avg'].copy_(torch.from_numpy(sq32))
    with torch.no_grad():
        q.copy_(torch.from_numpy(p32))
    q.grad = torch.from_numpy(grads[2]) * np.float32(gs)
    o32.step()
    out = R.rmsprop_step(p32, grads[2], sq32, lr, alpha, eps, wd, gs)
    assert (np.abs(q.detach().double().numpy() - out['p']) <= out['bound_p']).all()
    assert (np.abs(o32.state[q]['square_avg'].double().numpy() - out['sq']) <= out['bound_sq']).all()


@pytest.mark.parametrize('wd', [0.0, 1e-4])
@pytest.mark.parametrize('gs', [1.0, 0.5, 1.0 / 3.0])
@pytest.mark.parametrize('momentum', [0.9, 0.0])
def test_sgd_equals_torch(wd, gs, momentum):
    """Three steps (first_step 1, 0, 0) == torch.optim.SGD in fp64; momentum 0 never touches the buffer; the fp32 torch step
    stays inside the bounds."""
    n = 1003
    r = np.random.default_rng(12)
    p0 = r.standard_normal(n).astype(np.float32)
    grads = [(r.standard_normal(n) * (0.1 + i)).astype(np.float32) for i in range(3)]
    lr, mom = _h(0.2), _h(momentum)
    pt = torch.from_numpy(p0).double().requires_grad_()
    opt = torch.optim.SGD([pt], lr=lr, momentum=mom, weight_decay=_h(wd))
    p, buf = p0.astype(np.float64), (np.full(n, -777.0) if momentum == 0 else np.zeros(n))
    for i, g in enumerate(grads):
        pt.grad = torch.from_numpy(g).double() * _h(gs)
        opt.step()
        out = R.sgd_step(p, g, buf, lr, momentum, wd, gs, first_step=(i == 0))
        p, buf = out['p'], out['buf']
        assert np.abs(p - pt.detach().numpy()).max() <= 1e-13
        if momentum == 0:
            assert (buf == -777.0).all()
        else:
            assert np.abs(buf - opt.state[pt]['momentum_buffer'].numpy()).max() <= 1e-13
    if momentum != 0:
        p32, b32 = p.astype(np.float32), buf.astype(np.float32)
        q = torch.from_numpy(p32.copy()).requires_grad_()
        o32 = torch.optim.SGD([q], lr=lr, momentum=mom, weight_decay=_h(wd))
        q.grad = torch.from_numpy(grads[1]) * np.float32(gs)
        o32.step()
        o32.state[q]['momentum_buffer'].copy_(torch.from_numpy(b32))
        with torch.no_grad():
            q.copy_(torch.from_numpy(p32))
        q.grad = torch.from_numpy(grads[2]) * np.float32(gs)
        o32.step()
        out = R.sgd_step(p32, grads[2], b32, lr, momentum, wd, gs, first_step=False)
        assert (np.abs(q.detach().double().numpy() - out['p']) <= out['bound_p']).all()
        assert (np.abs(o32.state[q]['momentum_buffer'].double().numpy() - out['buf']) <= out['bound_buf']).all()


def test_guard_semantics():
    """A raised flag[0] blocks the step; a non-finite g * grad_scale (fp32: 3e38 * 2 overflows) is skipped, bits kept, and
    raises FLAG_GRAD in flag[1]; dsnt_nonfinite_flag promotes it."""
    n = 64
    r = np.random.default_rng(3)
    p, sq = r.standard_normal(n).astype(np.float32), np.abs(r.standard_normal(n)).astype(np.float32)
    g = r.standard_normal(n).astype(np.float32)
    for step in (lambda **k: R.rmsprop_step(p, g, sq, 1e-3, grad_scale=2.0, **k), lambda **k: R.sgd_step(p, g, sq, 0.1, grad_scale=2.0, **k)):
        out = step(flag=[1, 0])
        assert np.array_equal(out['p'], p) and out['flag'] == [1, 0]
        clean, free = step(flag=[0, 0]), step()
        assert clean['flag'] == [0, 0] and np.array_equal(clean['p'], free['p'])
    bad = g.copy()
    bad[[0, 5, 9, n - 1]] = [np.inf, -np.inf, np.nan, 3e38]
    for out, state in ((R.rmsprop_step(p, bad, sq, 1e-3, grad_scale=2.0, flag=[0, 0]), 'sq'),
                       (R.sgd_step(p, bad, sq, 0.1, grad_scale=2.0, flag=[0, 0]), 'buf')):
        assert out['flag'] == [0, R.FLAG_GRAD] and np.flatnonzero(out['skip']).tolist() == [0, 5, 9, n - 1]
        assert np.array_equal(out['p'][out['skip']], p[out['skip']]) and np.array_equal(out[state][out['skip']], sq[out['skip']])
        assert np.isfinite(out['p']).all() and (out['p'][~out['skip']] != p[~out['skip']]).all()
    assert R.sgd_step(p, bad, sq, 0.1, grad_scale=1.0, flag=[0, 0])['skip'].sum() == 3       # 3e38 itself is finite
    assert R.nonfinite_flag(g, [0, 0], R.FLAG_LOSS) == [0, 0]
    assert R.nonfinite_flag(bad, [0, 0], R.FLAG_LOSS) == [R.FLAG_LOSS, 0]
    assert R.nonfinite_flag(g, [0, R.FLAG_GRAD], R.FLAG_LOSS) == [R.FLAG_GRAD, R.FLAG_GRAD]


def test_launch_mirrors():
    """flat_grid / tile_cgs as the GPU module's premises use them."""
    assert R.flat_grid(1) == 1 and R.flat_grid(256 * 4096) == 4096 and R.flat_grid(2621443) == 4096 and R.flat_grid(4200) == 17
    assert R.tile_cgs(257, 32) == 32 and R.tile_cgs(257, 16) == 16 and R.tile_cgs(3, 20) == 20 and R.tile_cgs(3, 24) == 24
    assert R.tile_cgs(8, 48) == 16 and R.tile_grid_y(8, 48) == 3 and R.tile_cgs(2, 258) == 256 and R.tile_grid_y(2, 258) == 1
    assert R.apply_is_fixed(163841, 64) == (True, 4096) and R.apply_is_fixed(2561, 128, pro=True) == (True, 128)
    assert not R.apply_is_fixed(350, 48)[0] and not R.apply_is_fixed(60003, 80)[0]


# ---------------------------------------------------------------- the BatchNorm finalise oracle
def _finalize_case(M, C, seed):
    x, gamma, beta, da = R.bn_case(M, C, seed)
    s1, s2, _, _ = R.tile_sums(x, M, C)
    return x, gamma, beta, da, np.stack([s1, s2], 1)             # partial [tiles][2][C], fp64: the sums unrounded


@pytest.mark.parametrize('M,C', [(1, 8), (37, 20), (4133, 64)])
def test_bn_finalize_oracle_equals_batch_norm(M, C):
    """R.bn_finalize fed with R.tile_sums(x) == F.batch_norm(x.double(), training=True): the output through scale / shift and
    both running statistics after two calls (two inputs) with momentum 0.1 — two fp64 programs, 1e-12 relative.  momentum and
    eps are handed to torch as the fp32 values the ABI carries.  torch refuses one value per channel in training mode, so
    at M = 1 the reference is the definition: mean = x, var = 0 (unbias = 1), y = beta."""
    mom, eps = _h(0.1), _h(1e-5)
    rm, rv = np.linspace(-1, 1, C), np.linspace(0.5, 2, C)
    rmt, rvt = torch.from_numpy(rm.copy()), torch.from_numpy(rv.copy())
    for call in range(2):
        x, gamma, beta, _, part = _finalize_case(M, C, seed=M + C + call)
        o = R.bn_finalize(part, M, gamma, beta, rm, rv, 0.1, 1e-5, 1)
        scale = gamma.astype(np.float64) * o['invstd']
        y = x.astype(np.float64) * scale + (beta.astype(np.float64) - o['mean'] * scale)
        if M > 1:
            yt = F.batch_norm(torch.from_numpy(x).double(), rmt, rvt, torch.from_numpy(gamma).double(),
                              torch.from_numpy(beta).double(), True, mom, eps).numpy()
        else:
            yt = np.broadcast_to(beta.astype(np.float64), (1, C))
            rmt = (1 - mom) * rmt + mom * torch.from_numpy(x[0]).double()
            rvt = (1 - mom) * rvt
        assert np.abs(y - yt).max() <= 1e-12 * max(1.0, np.abs(yt).max())
        rm, rv = o['running_mean'], o['running_var']
        assert np.abs(rm - rmt.numpy()).max() <= 1e-12 * np.abs(rmt.numpy()).max()
        assert np.abs(rv - rvt.numpy()).max() <= 1e-12 * np.abs(rvt.numpy()).max()
        assert (o['bar_mean'] > 0).all() and (o['bar_invstd'] > 0).all()
    # eval mode: the running pair is the statistic, nothing moves
    e = R.bn_finalize(None, M, gamma, beta, rm, rv, 0.1, 1e-5, 0)
    assert np.array_equal(e['mean'], rm) and np.abs(e['invstd'] - 1 / np.sqrt(rv + eps)).max() <= 1e-15 * e['invstd'].max()
    assert 'running_mean' not in e and not e['dm'].any() and not e['bar_invstd_spread'].any()


@pytest.mark.parametrize('M,C', [(1, 8), (37, 20), (4133, 64)])
def test_bn_bwd_finalize_oracle_equals_autograd(M, C):
    """R.bn_bwd_finalize == autograd's dgamma / dbeta, and its two coefficients are the ones with which R.bn_apply reproduces
    x.grad (1e-12 relative; M = 1 by the definition: xhat = 0, dx = 0, dgamma = 0, dbeta = da).  Accumulation adds the old
    vectors; DSNT_BN_FROZEN zeroes the coefficients and nothing else."""
    x, gamma, beta, da, part = _finalize_case(M, C, seed=3 * M + C)
    f = R.bn_finalize(part, M, gamma, beta, None, None, 0.1, 1e-5, 1)
    d1, d2, _, _ = R.bn_bwd_tile_sums(da, x, f['mean'], f['invstd'], M, C)
    bpart = np.stack([d1, d2], 1)
    old_g, old_b = np.full(C, 0.25, np.float32), np.full(C, -0.5, np.float32)
    o = R.bn_bwd_finalize(bpart, M, 0, old_g, old_b)
    scale = gamma.astype(np.float64) * f['invstd']
    dx, _, _ = R.bn_apply(da, x, scale, beta - f['mean'] * scale, f['mean'], f['invstd'], o['coef'], 0)
    if M > 1:
        xt = torch.from_numpy(x).double().requires_grad_()
        gt, bt = torch.from_numpy(gamma).double().requires_grad_(), torch.from_numpy(beta).double().requires_grad_()
        F.batch_norm(xt, None, None, gt, bt, True, _h(0.1), _h(1e-5)).backward(torch.from_numpy(da).double())
        want_dx, want_dg, want_db = xt.grad.numpy(), gt.grad.numpy(), bt.grad.numpy()
    else:
        want_dx, want_dg, want_db = np.zeros((1, C)), np.zeros(C), da[0].astype(np.float64)
    ref = max(1.0, np.abs(want_dx).max())
    assert np.abs(dx - want_dx).max() <= 1e-12 * ref * max(1.0, float(f['invstd'].max()))
    assert np.abs(o['dgamma'] - want_dg).max() <= 1e-12 * max(1.0, np.abs(want_dg).max())
    assert np.abs(o['dbeta'] - want_db).max() <= 1e-12 * max(1.0, np.abs(want_db).max())
    a = R.bn_bwd_finalize(bpart, M, 1, old_g, old_b)
    assert np.array_equal(a['dgamma'], o['dgamma'] + 0.25) and np.array_equal(a['dbeta'], o['dbeta'] - 0.5)
    assert np.array_equal(a['coef'], o['coef']) and (a['bar_dgamma'] > o['bar_dgamma']).all()
    z = R.bn_bwd_finalize(bpart, M, R.BN_FROZEN | 1, old_g, None)
    assert not z['coef'].any() and not z['bar_coef'].any() and np.array_equal(z['dgamma'], a['dgamma']) and z['dbeta'] is None


def test_finalize_bars_admit_a_plain_fp64_combine_and_refuse_an_fp32_one():
    """The bars are no tighter than a left-to-right fp64 evaluation of the kernels' expressions achieves (numpy, another
    order than math.fsum), on producer, offset and cancelling partials; and on the cancelling partials a left-to-right fp32
    combine misses the mean bar by more than 10x."""
    for part, M in (R.partial_producer(65, 20, 1)[:2], R.partial_producer(257, 8, 2, rows=4, offset=300.0)[:2], R.partial_cancelling(1027, 20, 3)):
        o = R.bn_finalize(part, M, None, None, None, None, 0.1, 1e-5, 1)
        s = np.zeros((2, part.shape[2]))
        for t in range(part.shape[0]):
            s += part[t].astype(np.float64)
        mean = s[0] * (1.0 / M)
        var = np.maximum(s[1] * (1.0 / M) - mean * mean, 0.0)
        is_ = (1.0 / np.sqrt(var + float(np.float32(1e-5)))).astype(np.float32)
        assert (np.abs(mean.astype(np.float32).astype(np.float64) - o['mean']) <= o['bar_mean']).all()
        assert (np.abs(is_.astype(np.float64) - o['invstd']) <= o['bar_invstd']).all()
    f0, _ = R.combine_f32(part)
    assert (np.abs(f0 / M - o['mean']) >= 10 * o['bar_mean']).all()


def test_half_ulp32():
    """Half an fp32 ulp of the binade: powers of two open their binade, zero and the subnormals share the spacing 2^-149."""
    v = np.array([1.0, 1.5, 2.0, 0.75, -300.0, 2.0 ** -126, 2.0 ** -130, 0.0, -0.0])
    want = np.array([2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 2.0 ** -25, 2.0 ** -16, 2.0 ** -150, 2.0 ** -150, 2.0 ** -150, 2.0 ** -150])
    assert np.array_equal(R.half_ulp32(v), want)
    for x in (1.0, 1.5, 0.75, 300.0):
        assert R.half_ulp32(x) == 0.5 * float(np.spacing(np.float32(x)))


def test_prologue_mapping_mirror():
    """R.pro_mapping / R.pro_reads as the GPU module's premise table uses them: every element read once at every shape."""
    assert R.pro_mapping(20, 256) == [(40, 6, 16)] and R.pro_mapping(160, 256) == [(256, 1, 0), (64, 4, 0)]
    assert R.pro_mapping(160, 512) == [(320, 1, 192)] and R.pro_mapping(256, 256) == [(256, 1, 0)] * 2
    for C_, NT, tiles, want in ((20, 256, 97, [2]), (160, 256, 65, [5, 2]), (4, 512, 1025, [2]), (256, 512, 17, [2]), (64, 256, 1, [1])):
        cnt, trips = R.pro_reads(tiles, C_, NT)
        assert (cnt == 1).all() and trips == want
