"""Every fp16x3 entry point the engine launches, held to fp32 accuracy PER CHANNEL on operands with a production range.

The per-tensor bars of tests/test_conv_gpu.py and tests/test_bwd1_gpu.py measure errors against the whole output's scale on iid
data, where no channel is small.  fp16x3 (csrc/conv_split.h) loses relative precision exactly on small quantities: below
bound 2^-16 the low plane of an operand is an fp16 subnormal with the absolute precision bound 2^-38.  Here each kernel runs
under four operand profiles (tests/f16x3_util.py):
  * chan     A = relu(x gamma_c + beta_c), gamma_c log-uniform over [2^-14, 1], one dead and one constant channel;
  * wspread  per-output-channel weight scale log-uniform over [2^-14, 1] (weight gradients: the same spread on dY's channels);
  * grad     the gradient-like operand heavy-tailed (n^3), per-image scales over [2^-12, 1], one image entirely zero;
  * probe    exact operands whose results need every subnormal plane element (f16x3_util: a flush is a hard failure);
with bounds produced the way the engine produces them (weights: the prep launch; raw operands and gradients: dsnt_amax; BatchNorm
operands: the analytic bound at the launch's real M; the folded BatchNorm backward: dsnt_bn_bwd_finalize_bound), and — outside the
probe — never tighter than the measured production looseness: LOOSE_A (2^8) times the maximum of an A operand, LOOSE_G (2^2)
times that of a gradient operand (f16x3_util.LOOSE_LOG2).  Bars, per output channel over the batch (forward,
data gradient) and per output-channel row (weight gradient): err_c <= max(4 err32_c, 2e-6 scale_c), errors against fp64 torch on
the same fp32 inputs, err32_c torch fp32's own."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f16x3_util as U

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _geom(N, H, W, Cin, Cout, R, stride=1, pad=None, dil=1):
    from dsnt._lib import ConvGeom
    pad = (R - 1) // 2 if pad is None else pad
    Ho = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (R - 1) - 1) // stride + 1
    return ConvGeom(N, H, W, Cin, Ho, Wo, Cout, R, R, stride, pad, dil)


def _check(fails):
    assert not fails, fails


# -------------------------------------------------------------------------------------------------------- operand profiles
def _act(profile, tag, shape, pro):
    """The A operand of a forward-like launch, NHWC.  Returns (x, sc, sh, relu, act64, act32, gamma, beta): with `pro` the
    kernel forms act = relu?(x sc + sh) itself (sc, sh are the BatchNorm's scale / shift; gamma / beta give the analytic
    bound); without, x is the materialised operand."""
    r = U.rng(tag + profile)
    N, H, W, Cc = shape
    if profile == 'probe':
        v = np.where(np.arange(Cc) % 2 == 0, 1.0, 0.0)          # even channels 'res', odd channels 'pow2'
        n = N * H * W
        x = np.where(v > 0, U.probe_res(r, n * Cc).reshape(n, Cc), U.probe_pow2(r, n * Cc).reshape(n, Cc)).reshape(shape)
        x[0, 0, 0, 0] = U.PROBE_BOUND                           # a 'res' channel: fixes s = 2^13 (exact bound)
        U.assert_probe_exact(x)
        x = U.f32(x)
        sc, sh = (torch.ones(Cc), torch.zeros(Cc)) if pro else (None, None)
        act = torch.relu(x) if pro else x
        return x, sc, sh, int(pro), act.double(), act, None, None
    if profile == 'chan':
        gamma = U.log_spread(r, Cc, -14)
        gamma[:2] = 0.0
        beta = gamma * r.standard_normal(Cc) * 0.3
        beta[1] = 2.0 ** -9                                      # gamma = 0: a constant channel ... and a dead one
        x = r.standard_normal(shape)
    elif profile == 'wspread':
        gamma = r.uniform(0.5, 1.5, Cc)
        beta = r.standard_normal(Cc) * 0.3
        x = r.standard_normal(shape)
    else:                                                        # 'grad': the A operand of a data gradient
        x = U.heavy(r, shape)
        gamma = beta = None
    x = U.f32(x)
    if gamma is None:
        return x, None, None, 0, x.double(), x, None, None
    g32, b32 = U.f32(gamma), U.f32(beta)
    if pro:
        a64 = torch.relu(x.double() * g32.double() + b32.double())
        a32 = torch.relu(x * g32 + b32)
        return x, g32, b32, 1, a64, a32, g32, b32
    a = torch.relu(x * g32 + b32)
    return a, None, None, 0, a.double(), a, g32, b32


def _weights(profile, tag, Cout, R, Cin):
    """Weights [Cout][R][R][Cin].  The probe's: one non-zero per output channel — a power of two on a 'res' input channel for
    even o, a 'res' value on a 'pow2' channel for odd o (every output element is then ONE exact product)."""
    r = U.rng(tag + profile + 'w')
    if profile == 'probe':
        w = np.zeros((Cout, R * R, Cin))
        n = Cout
        taps = r.integers(0, R * R, n)
        ch = 2 * r.integers(0, Cin // 2, n) + (np.arange(n) % 2)
        vals = np.where(np.arange(n) % 2 == 0, U.probe_pow2(r, n), U.probe_res(r, n))
        w[np.arange(n), taps, ch] = vals
        w[1, taps[1], ch[1]] = U.PROBE_BOUND                     # times a power of two: still exact
        U.assert_probe_exact(w)
        return U.f32(w.reshape(Cout, R, R, Cin))
    w = r.standard_normal((Cout, R, R, Cin)) * (2.0 / (Cin * R * R)) ** 0.5
    if profile == 'wspread':
        w *= U.log_spread(r, Cout, -14).reshape(-1, 1, 1, 1)
    return U.f32(w)


def _a_bound(x, sc, sh, relu, act32, gamma, beta, M, profile, loose=U.LOOSE_A):
    """The A bound of a launch: exact for the probe; otherwise the engine's (analytic for a BatchNorm operand, dsnt_amax for
    a materialised one), never tighter than `loose` x max|A|."""
    if profile == 'probe':
        return U.dev_amax(act32.contiguous().to(DEV))
    loose = U.dev_amax(act32.contiguous().to(DEV), loose)
    if gamma is not None:
        return U.bmax(U.bn_bound(gamma, beta, M, DEV), loose)
    return loose


def _conv_refs(act64, act32, w, stride, pad, dil):
    w4 = _nchw(w)
    y64 = F.conv2d(_nchw(act64), w4.double(), None, stride=stride, padding=pad, dilation=dil).permute(0, 2, 3, 1)
    y32 = F.conv2d(_nchw(act32), w4, None, stride=stride, padding=pad, dilation=dil).permute(0, 2, 3, 1)
    return y64, y32


def _compare(name, profile, got, y64, y32, axis=-1):
    if profile == 'probe':
        return U.exact(name, got, y64)
    return U.per_channel(name, got, y64, y32, axis)


# ------------------------------------------------------------------------------------------------------------ forward-like
FWD_CASES = {
    # name: (N, H, W, Cin, Cout, k, stride, pad, dil) of dsnt_conv_fwd_f16x3_ex, and the kernel it reaches
    'generic': (2, 12, 12, 64, 64, 3, 1, 1, 1),       # implicit GEMM (W % 16 != 0: not the halo kernel)
    'generic_s2': (2, 16, 16, 64, 128, 3, 2, 1, 1),   # stride 2 (ResNet)
    'halo': (2, 8, 32, 64, 64, 3, 1, 1, 1),           # the LDS halo-tile kernel
    'gemm1': (4, 128, 128, 64, 64, 1, 1, 0, 1),       # >= 65536 rows: the streaming 1x1 kernel (csrc/gemm1.hip)
}
FWD_ROUTE = {'generic': 0, 'generic_s2': 0, 'halo': 2, 'gemm1': 1}       # dsnt_conv_f16x3_route(g, 0)


@pytest.mark.parametrize('profile', U.PROFILES)
@pytest.mark.parametrize('kind', list(FWD_CASES))
def test_conv_fwd_f16x3_ex(kind, profile):
    from dsnt import _lib
    from dsnt._lib import ptr, call
    N, H, W, Cin, Cout, k, stride, pad, dil = FWD_CASES[kind]
    g = _geom(N, H, W, Cin, Cout, k, stride, pad, dil)
    assert _lib.fn('dsnt_conv_f16x3_route')(C.byref(g), 0) == FWD_ROUTE[kind]
    tag = 'ex' + kind
    x, sc, sh, relu, a64, a32, gamma, beta = _act(profile, tag, (N, H, W, Cin), pro=True)
    w = _weights(profile, tag, Cout, k, Cin)
    M = N * g.Ho * g.Wo
    xd, wd = x.to(DEV), w.to(DEV)
    planes, wb = U.prep_weights(wd)
    ab = _a_bound(x, sc, sh, relu, a32, gamma, beta, N * H * W, profile)
    y = torch.full((N, g.Ho, g.Wo, Cout), float('nan'), device=DEV)
    stats = torch.zeros((M + 127) // 128, 2, Cout, device=DEV)
    scd, shd = (sc.to(DEV), sh.to(DEV)) if sc is not None else (None, None)
    call('dsnt_conv_fwd_f16x3_ex', ptr(xd), ptr(planes), wd.numel(), ptr(wb), ptr(ab), None, ptr(y), ptr(scd), ptr(shd), relu,
         None, None, ptr(stats), C.byref(g), None, None)
    torch.cuda.synchronize()
    y64, y32 = _conv_refs(a64, a32, w, stride, pad, dil)
    _check(_compare('fwd_ex/' + kind, profile, y, y64, y32))


STREAM_CASE = (2, 16, 32, 64, 64)


@pytest.mark.parametrize('profile', U.PROFILES)
@pytest.mark.parametrize('mode', ['plain', 'pro', 'bnb'])
def test_conv_fwd_f16x3_stream(mode, profile):
    """csrc/conv3s.hip: a raw operand, a BatchNorm+ReLU prologue, and the data-gradient form with the BatchNorm-backward
    epilogue (no ReLU mask: the output is the convolution itself)."""
    from dsnt import _lib
    from dsnt._lib import ptr, call, BnBwdEpilogue
    N, H, W, Cin, Cout = STREAM_CASE
    g = _geom(N, H, W, Cin, Cout, 3)
    assert _lib.fn('dsnt_conv_fwd_stream_ok')(C.byref(g)) == 1
    tag = 'st' + mode
    x, sc, sh, relu, a64, a32, gamma, beta = _act(profile, tag, (N, H, W, Cin), pro=mode == 'pro')
    w = _weights(profile, tag, Cout, 3, Cin)
    M = N * H * W
    xd, wd = x.contiguous().to(DEV), w.to(DEV)
    strm, wb = U.prep_weights(wd, stream_order=True)
    ab = _a_bound(x, sc, sh, relu, a32, gamma, beta, M, profile, U.LOOSE_G if mode == 'bnb' else U.LOOSE_A)
    y = torch.full((N, H, W, Cout), float('nan'), device=DEV)
    stats = torch.full((M // 128, 2, Cout), float('nan'), device=DEV)
    bnb = None
    if mode == 'bnb':
        r = U.rng(tag + 'bnb')
        keep = [U.f32(r.standard_normal(s)).to(DEV) for s in ((N, H, W, Cout), (Cout,), (Cout,), (Cout,))]
        istd = (keep[3].abs() + 0.5).contiguous()
        bnb = BnBwdEpilogue(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[1]), ptr(istd), 0)
    scd, shd = (sc.to(DEV), sh.to(DEV)) if sc is not None else (None, None)
    call('dsnt_conv_fwd_f16x3_stream', ptr(xd), ptr(strm), wd.numel(), ptr(wb), ptr(ab), None, ptr(y), ptr(scd), ptr(shd), relu,
         None, None, ptr(stats), C.byref(g), C.byref(bnb) if bnb is not None else None, None)
    torch.cuda.synchronize()
    y64, y32 = _conv_refs(a64, a32, w, 1, 1, 1)
    _check(_compare('stream/' + mode, profile, y, y64, y32))


def _bn_behind(profile, tag, shape):
    """The BatchNorm behind a data gradient, for the folded backward: its input y, scale (gamma invstd), mean, invstd and dz
    behind it.  dz correlates with xhat (a real gradient does), so that c1 sqrt(M) — the loose term of the bound — matters."""
    r = U.rng(tag + profile + 'bn')
    N, H, W, Cc = shape
    M = N * H * W
    mu = r.standard_normal(Cc) * 0.5
    std = np.abs(r.uniform(-1, 1, Cc)) + 0.5
    y = r.standard_normal(shape) * std + mu
    gamma = U.log_spread(r, Cc, -14) if profile == 'chan' else r.uniform(0.3, 1.3, Cc)
    if profile == 'probe':
        dz = _act('probe', tag, shape, pro=False)[0].double().numpy()
        scale, coef = np.ones(Cc), np.zeros(2 * Cc)
        return [U.f32(a) for a in (y, scale, mu, 1.0 / std, dz)] + [U.f32(coef), None]
    xhat = (y - mu) / std
    if profile == 'grad':
        dz = U.heavy(r, shape) + 0.5 * xhat * U.log_spread(r, N, -12).reshape(-1, 1, 1, 1)
        dz[1] = 0.0
    else:
        dz = r.standard_normal(shape) * 1e-3 + 2e-3 * xhat
    scale = gamma / std
    y32, mu32, is32, sc32, dz32 = (U.f32(a) for a in (y, mu, 1.0 / std, scale, dz))
    xh = (y32.double().reshape(M, Cc) - mu32.double()) * is32.double()
    d = dz32.double().reshape(M, Cc)
    partial = torch.stack([d.sum(0), (d * xh).sum(0)]).float().reshape(1, 2, Cc)
    return [y32, sc32, mu32, is32, dz32, None, partial]


def _apply64(y, scale, mu, istd, dz, coef, Cc):
    """fp64 and fp32 of dy = scale (dz - c0 - (y - mean) invstd c1) from the same fp32 inputs."""
    c0, c1 = coef[:Cc], coef[Cc:]
    d64 = scale.double() * (dz.double() - c0.double() - (y.double() - mu.double()) * istd.double() * c1.double())
    d32 = scale * (dz - c0 - (y - mu) * istd * c1)
    return d64, d32


def _finalize_bound(partial, M, Cc, scale, dz):
    """coef and the bound of dy as the engine leaves them (dsnt_bn_bwd_finalize_bound)."""
    from dsnt._lib import ptr, call
    coef = torch.empty(2 * Cc, device=DEV)
    dg, db = torch.empty(Cc, device=DEV), torch.empty(Cc, device=DEV)
    out = torch.zeros(64, device=DEV)
    pd, sd, dzd = partial.to(DEV), scale.to(DEV), dz.contiguous().to(DEV)
    dza = U.dev_amax(dzd)
    call('dsnt_bn_bwd_finalize_bound', ptr(pd), 1, M, Cc, ptr(dg), ptr(db), 0, ptr(coef), ptr(sd), ptr(dza), ptr(out))
    torch.cuda.synchronize()
    return coef.cpu(), out


@pytest.mark.parametrize('profile', U.PROFILES)
def test_conv_dgrad_f16x3_stream_apply(profile):
    """csrc/conv3s.hip MODE 4: the data gradient of a 3x3 convolution whose A operand is the BatchNorm backward of the layer
    behind, formed while it is staged; its bound is what dsnt_bn_bwd_finalize_bound leaves."""
    from dsnt._lib import ptr, call, BnBwdEpilogue, BnBwdApply, BnTail
    N, H, W, Cin, Cout = STREAM_CASE
    g = _geom(N, H, W, Cin, Cout, 3)
    M = N * H * W
    tag = 'ap'
    y, scale, mu, istd, dz, coef, partial = _bn_behind(profile, tag, (N, H, W, Cin))
    w = _weights(profile, tag, Cout, 3, Cin)
    if profile == 'probe':
        bound = U.dev_amax(dz.contiguous().to(DEV))
    else:
        coef, fb = _finalize_bound(partial, M, Cin, scale, dz)
    d64, d32 = _apply64(y, scale, mu, istd, dz, coef, Cin)
    if profile != 'probe':
        bound = U.bmax(fb, U.dev_amax(d32.contiguous().to(DEV), U.LOOSE_G))
    yd, scd, mud, isd, dzd, cfd = (t.contiguous().to(DEV) for t in (y, scale, mu, istd, dz, coef))
    wd = w.to(DEV)
    strm, wb = U.prep_weights(wd, stream_order=True)
    r = U.rng(tag + 'bnb')
    keep = [U.f32(r.standard_normal(s)).to(DEV) for s in ((N, H, W, Cout), (Cout,), (Cout,), (Cout,))]
    istd2 = (keep[3].abs() + 0.5).contiguous()
    bnb = BnBwdEpilogue(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[1]), ptr(istd2), 0)
    ap = BnBwdApply(ptr(yd), ptr(scd), ptr(mud), ptr(isd), ptr(cfd))
    out = torch.full((N, H, W, Cout), float('nan'), device=DEV)
    dyo = torch.full((N, H, W, Cin), float('nan'), device=DEV)
    stats = torch.full((M // 128, 2, Cout), float('nan'), device=DEV)
    amax = torch.zeros(64, device=DEV)
    tail = BnTail()
    tail.amax = amax.data_ptr()
    call('dsnt_conv_dgrad_f16x3_stream_apply', ptr(dzd), C.byref(ap), ptr(dyo), ptr(strm), wd.numel(), ptr(wb), ptr(bound),
         ptr(out), ptr(stats), 0, C.byref(g), C.byref(bnb), C.byref(tail))
    torch.cuda.synchronize()
    y64, y32 = _conv_refs(d64, d32, w, 1, 1, 1)
    _check(_compare('stream_apply', profile, out, y64, y32))


FWD1_CASE = (2, 128, 128, 64, 64)


@pytest.mark.parametrize('profile', U.PROFILES)
def test_conv1x1_fwd_f16x3(profile):
    from dsnt import _lib
    from dsnt._lib import ptr, call, BnTail
    N, H, W, Cin, Cout = FWD1_CASE
    g = _geom(N, H, W, Cin, Cout, 1)
    assert _lib.fn('dsnt_conv1x1_fwd_ok')(C.byref(g))
    M = N * H * W
    tag = 'f1'
    x, sc, sh, relu, a64, a32, gamma, beta = _act(profile, tag, (N, H, W, Cin), pro=True)
    w = _weights(profile, tag, Cout, 1, Cin)
    xd, wd = x.contiguous().to(DEV), w.to(DEV)
    planes, wb = U.prep_weights(wd)
    ab = _a_bound(x, sc, sh, relu, a32, gamma, beta, M, profile)
    scd, shd = (sc.to(DEV), sh.to(DEV)) if sc is not None else (None, None)
    rows = _lib.fn('dsnt_conv1x1_fwd_stats_rows')(C.byref(g), 0)
    y = torch.full((N, H, W, Cout), float('nan'), device=DEV)
    stats = torch.full((rows, 2, Cout), float('nan'), device=DEV)
    amax = torch.zeros(64, device=DEV)
    tl = BnTail()
    tl.amax = amax.data_ptr()
    call('dsnt_conv1x1_fwd_f16x3', ptr(xd), ptr(planes), wd.numel(), ptr(wb), ptr(ab), None, ptr(y), ptr(scd), ptr(shd), relu,
         None, ptr(stats), C.byref(g), C.byref(tl))
    torch.cuda.synchronize()
    y64, y32 = _conv_refs(a64, a32, w, 1, 0, 1)
    _check(_compare('fwd1', profile, y, y64, y32))


STEM_CASE = (2, 32)        # N, Ho: the space-to-depth stem, [N][Ho + 1][Ho + 1][16] -> [N][Ho][Ho][64]


@pytest.mark.parametrize('profile', U.PROFILES)
def test_stem4_fwd_f16x3(profile):
    from dsnt import _lib
    from dsnt._lib import ptr, call, ConvGeom, BnTail
    N, Ho = STEM_CASE
    Hi = Ho + 1
    g = ConvGeom(N, Hi, Hi, 16, Ho, Ho, 64, 4, 4, 1, 1, 1)
    assert _lib.fn('dsnt_stem4_fwd_ok')(C.byref(g)) == 1
    tag = 'sf'
    x, _, _, _, a64, a32, gamma, beta = _act(profile, tag, (N, Hi, Hi, 16), pro=False)
    w = _weights(profile, tag, 64, 4, 16)
    xd, wd = x.contiguous().to(DEV), w.to(DEV)
    planes, wb = U.prep_weights(wd)
    ab = U.dev_amax(xd) if profile == 'probe' else U.dev_amax(xd, U.LOOSE_A)
    rows = _lib.fn('dsnt_stem4_fwd_stats_rows')(C.byref(g))
    y = torch.full((N, Ho, Ho, 64), float('nan'), device=DEV)
    part = torch.full((rows, 2, 64), float('nan'), device=DEV)
    am = torch.zeros(64, device=DEV)
    tail = BnTail()
    tail.amax = am.data_ptr()
    call('dsnt_stem4_fwd_f16x3', ptr(xd), ptr(planes), wd.numel(), ptr(wb), ptr(ab), None, ptr(y), ptr(part), C.byref(g),
         C.byref(tail))
    torch.cuda.synchronize()
    y64, y32 = _conv_refs(a64, a32, w, 1, 1, 1)
    _check(_compare('stem4_fwd', profile, y, y64, y32))


# ------------------------------------------------------------------------------------------------------------ weight gradients
def _grad(profile, tag, shape, A=None):
    """dY [N][Ho][Wo][Cout] of a weight gradient.  The probe's: one non-zero per output channel o, at a pixel of image 0 (a
    'res' image of A) holding a power of two for even o, at a pixel of image 1 (a 'pow2' image) holding a 'res' value for odd o:
    every dW element is then one exact product."""
    r = U.rng(tag + profile + 'g')
    N, Ho, Wo, Cc = shape
    if profile == 'probe':
        d = np.zeros(shape)
        o = np.arange(Cc)
        img = o % 2
        pix = r.choice(Ho * Wo - 1, Cc, replace=Ho * Wo - 1 < Cc)        # distinct pixels: a data gradient's dx rows are one product too
        pix[1] = Ho * Wo - 1
        d[img, pix // Wo, pix % Wo, o] = np.where(img == 0, U.probe_pow2(r, Cc), U.probe_res(r, Cc))
        d[1, Ho - 1, Wo - 1, 1] = U.PROBE_BOUND              # fixes the gradient's s (times a power of two in A's image 1)
        U.assert_probe_exact(d)
        return U.f32(d)
    if profile == 'grad':
        return U.f32(U.heavy(r, shape) * 1e-3)
    d = r.standard_normal(shape) * 1e-3
    if profile == 'wspread':
        d *= U.log_spread(r, Cc, -14)
    return U.f32(d)


def _wgrad_act(profile, tag, shape, pro):
    """A operand of a weight gradient.  The probe's: image 0 all 'res' values, image 1 all powers of two."""
    if profile != 'probe':
        return _act('chan' if profile == 'chan' else 'wspread', tag, shape, pro)
    r = U.rng(tag + 'probe' + 'a')
    N, H, W, Cc = shape
    n = H * W * Cc
    x = np.stack([U.probe_res(r, n), U.probe_pow2(r, n)] + [U.probe_pow2(r, n) for _ in range(N - 2)]).reshape(shape)
    x[0, 0, 0, 0] = U.PROBE_BOUND
    U.assert_probe_exact(x)
    x = U.f32(x)
    sc, sh = (torch.ones(Cc), torch.zeros(Cc)) if pro else (None, None)
    act = torch.relu(x) if pro else x
    return x, sc, sh, int(pro), act.double(), act, None, None


def _wgrad_refs(a64, a32, gy, wshape, stride, pad, dil):
    dw64 = torch.nn.grad.conv2d_weight(_nchw(a64), wshape, _nchw(gy).double(), stride=stride, padding=pad, dilation=dil)
    dw32 = torch.nn.grad.conv2d_weight(_nchw(a32), wshape, _nchw(gy), stride=stride, padding=pad, dilation=dil)
    return dw64.permute(0, 2, 3, 1), dw32.permute(0, 2, 3, 1)


WGRAD_CASES = {
    # name: (N, H, W, Cin, Cout, k, stride, pad, dil) of dsnt_conv_wgrad_f16x3, and the kernel it reaches
    'wgrad3': (2, 16, 16, 64, 64, 3, 1, 1, 1),       # 3x3 / stride 1: the halo kernel (csrc/wgrad3.hip)
    'wgrad1': (2, 128, 128, 64, 64, 1, 1, 0, 1),     # 1x1 of >= 16384 rows (csrc/wgrad1.hip)
    'generic': (2, 16, 16, 64, 128, 3, 2, 1, 1),     # stride 2: the generic split kernel (csrc/conv_split6.hip)
    'stem4': (2, 33, 33, 16, 64, 4, 1, 1, 1),        # the space-to-depth stem (csrc/stem4.hip), a raw operand
}
WGRAD_ROUTE = {'wgrad3': 2, 'wgrad1': 3, 'generic': 0, 'stem4': 1}       # dsnt_conv_f16x3_route(g, 1)


@pytest.mark.parametrize('profile', U.PROFILES)
@pytest.mark.parametrize('kind', list(WGRAD_CASES))
def test_conv_wgrad_f16x3(kind, profile):
    from dsnt import _lib
    from dsnt._lib import ptr, call
    N, H, W, Cin, Cout, k, stride, pad, dil = WGRAD_CASES[kind]
    g = _geom(N, H, W, Cin, Cout, k, stride, pad, dil)
    assert _lib.fn('dsnt_conv_f16x3_route')(C.byref(g), 1) == WGRAD_ROUTE[kind]
    assert _lib.fn('dsnt_conv_wgrad_halo_ok')(C.byref(g)) == (kind == 'wgrad3')
    tag = 'wg' + kind
    pro = kind != 'stem4'
    x, sc, sh, relu, a64, a32, gamma, beta = _wgrad_act(profile, tag, (N, H, W, Cin), pro)
    gy = _grad(profile, tag, (N, g.Ho, g.Wo, Cout))
    xd, gyd = x.contiguous().to(DEV), gy.to(DEV)
    ab = _a_bound(x, sc, sh, relu, a32, gamma, beta, N * H * W, profile)
    gb = U.dev_amax(gyd) if profile == 'probe' else U.dev_amax(gyd, U.LOOSE_G)
    nws = max(_lib.fn('dsnt_conv_wgrad_f16x3_ws_floats')(C.byref(g), 0), _lib.fn('dsnt_conv_wgrad_ws_floats')(C.byref(g)))
    ws = torch.empty(nws, device=DEV)
    dw = torch.full((Cout, k, k, Cin), float('nan'), device=DEV)
    db = torch.full((Cout,), float('nan'), device=DEV)
    scd, shd = (sc.to(DEV), sh.to(DEV)) if sc is not None else (None, None)
    call('dsnt_conv_wgrad_f16x3', ptr(xd), ptr(scd), ptr(shd), relu, ptr(gyd), ptr(ws), ptr(dw), ptr(db), 0, ptr(ab), ptr(gb),
         C.byref(g))
    torch.cuda.synchronize()
    dw64, dw32 = _wgrad_refs(a64, a32, gy, (Cout, Cin, k, k), stride, pad, dil)
    fails = _compare('wgrad/' + kind, profile, dw, dw64, dw32, axis=0)
    db64, db32 = gy.double().sum((0, 1, 2)), gy.sum((0, 1, 2))
    if profile == 'probe':
        fails += U.exact('wgrad/%s/bias' % kind, db, db64)
    else:
        e, e32 = float((db.cpu().double() - db64).abs().max()), float((db32.double() - db64).abs().max())
        if not e <= max(4 * e32, 2e-6 * float(db64.abs().max())):
            fails.append(('bias', e, e32))
    _check(fails)


# ----------------------------------------------------------------------------------------------------- the 1x1 one-pass backward
BWD1_CASE = (2, 128, 128, 64, 64)


@pytest.mark.parametrize('profile', U.PROFILES)
def test_conv1x1_bwd_f16x3(profile):
    """csrc/bwd1.hip: the data gradient (masked by the ReLU of the BatchNorm in front) per input channel and the weight gradient
    per output-channel row, in one pass.  The 'grad' profile folds the BatchNorm backward of the layer behind into the launch
    (its bound from dsnt_bn_bwd_finalize_bound); the others take dY as it is."""
    from dsnt import _lib
    from dsnt._lib import ptr, call, ConvGeom, BnBwdEpilogue, BnBwdApply
    N, H, W, Cin, Cout = BWD1_CASE
    M = N * H * W
    g = ConvGeom(N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, 1)
    assert _lib.fn('dsnt_conv1x1_bwd_ok')(C.byref(g))
    tag = 'b1'
    x, sc, sh, relu, a64, a32, gamma, beta = _wgrad_act(profile, tag, (N, H, W, Cin), pro=True)
    mu, istd = torch.zeros(Cin), torch.ones(Cin)                  # (the BatchNorm-backward sums are not under test here)
    if profile == 'probe':
        # W^T [Cin][Cout]: row o of W is 'res' for even o (dY there is a power of two), a power of two for odd o
        r = U.rng(tag + 'probe' + 'w')
        w = np.stack([U.probe_res(r, Cin) if o % 2 == 0 else U.probe_pow2(r, Cin) for o in range(Cout)])
        w[0, 0] = U.PROBE_BOUND                                   # a 'res' row: times a power of two
        U.assert_probe_exact(w)
        w = U.f32(w)
        gy = _grad('probe', tag, (N, H, W, Cout))
        # distinct pixels per output channel, so that every dx element is one product
        flat = gy.reshape(M, Cout)
        assert int((flat != 0).sum(1).max()) <= 1
    else:
        w = _weights(profile, tag, Cout, 1, Cin).reshape(Cout, Cin)
        if profile != 'grad':
            gy = _grad(profile, tag, (N, H, W, Cout))
    apply = profile == 'grad'
    if apply:
        yb, ysc, ymu, yis, dz, _, partial = _bn_behind('grad', tag, (N, H, W, Cout))
        dz = dz * 1e-3
        partial = partial * 1e-3
        coef, fb = _finalize_bound(partial, M, Cout, ysc, dz)
        d64, d32 = _apply64(yb, ysc, ymu, yis, dz, coef, Cout)
        gb = U.bmax(fb, U.dev_amax(d32.contiguous().to(DEV), U.LOOSE_G))
        gy64, gy32 = d64.reshape(M, Cout), d32.reshape(M, Cout)
    else:
        gy64, gy32 = gy.double().reshape(M, Cout), gy.reshape(M, Cout)
        gb = U.dev_amax(gy.contiguous().to(DEV)) if profile == 'probe' else U.dev_amax(gy.contiguous().to(DEV), U.LOOSE_G)
    ab = _a_bound(x, sc, sh, relu, a32, gamma, beta, M, profile)
    # references: dx = (dY W) [z > 0], dW = dY^T act, db = sum dY
    z64 = x.double().reshape(M, Cin) * sc.double() + sh.double()
    z32 = x.reshape(M, Cin) * sc + sh
    dx64 = (gy64 @ w.double()) * (z64 > 0)
    dx32 = (gy32 @ w) * (z32 > 0)
    act64, act32 = a64.reshape(M, Cin), a32.reshape(M, Cin)
    dw64, dw32 = gy64.t() @ act64, gy32.t() @ act32
    db64, db32 = gy64.sum(0), gy32.sum(0)
    # device
    wdt = w.t().contiguous().to(DEV)
    planes, wb = U.prep_weights(wdt)
    xd, scd, shd, mud, isd = (t.contiguous().to(DEV) for t in (x, sc, sh, mu, istd))
    xs = BnBwdEpilogue(ptr(xd), ptr(scd), ptr(shd), ptr(mud), ptr(isd), relu)
    if apply:
        yd, ysd, ymd, yid, cfd, dzd = (t.contiguous().to(DEV) for t in (yb, ysc, ymu, yis, coef, dz))
        ap = BnBwdApply(ptr(yd), ptr(ysd), ptr(ymd), ptr(yid), ptr(cfd))
        dyd, apref = dzd, C.byref(ap)
    else:
        dyd, apref = gy.contiguous().to(DEV), None
    splits = _lib.fn('dsnt_conv1x1_bwd_splits')(C.byref(g), 0)
    ws = torch.full((_lib.fn('dsnt_conv1x1_bwd_ws_floats')(C.byref(g), 0),), float('nan'), device=DEV)
    stats = torch.full((splits, 2, Cin), float('nan'), device=DEV)
    dx = torch.full((M, Cin), float('nan'), device=DEV)
    call('dsnt_conv1x1_bwd_f16x3', C.byref(xs), ptr(dyd), apref, ptr(planes), wdt.numel(), ptr(wb), ptr(ab), ptr(gb), ptr(dx),
         ptr(stats), ptr(ws), None, 0, C.byref(g))
    dw, db = torch.zeros(Cout, Cin, device=DEV), torch.zeros(Cout, device=DEV)
    table = torch.tensor([[ws.data_ptr(), dw.data_ptr(), db.data_ptr(), splits, Cout * Cin, Cout, 0]], dtype=torch.int64).to(DEV)
    call('dsnt_wgrad_reduce_all', ptr(table), 1, (Cout * Cin // 4 + (Cout + 3) // 4 + 63) // 64)
    torch.cuda.synchronize()
    fails = _compare('bwd1/dx', profile, dx, dx64, dx32, axis=-1)
    fails += _compare('bwd1/dw', profile, dw, dw64, dw32, axis=0)
    if profile == 'probe':
        fails += U.exact('bwd1/db', db, db64)
    _check(fails)


@pytest.fixture(scope='module', autouse=True)
def _report():
    """Prints, when the module finishes, each kernel's worst per-channel err_c / err32_c and err_c / bar_c (informational)."""
    yield
    for name, rec in sorted(U.REPORT.items()):
        print('F16X3_RANGE %-26s %s' % (name, U.report_line(rec)))
