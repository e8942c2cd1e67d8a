"""Operands and launches of tests/test_shortcut_fused_gpu.py: conv3 of a Bottleneck with a projection shortcut, and that
shortcut (hourglass.py:25,44-48), as the pair of existing forward launches and as the one fused launch
(dsnt_conv1x1_fwd_ds_f16x3), through the C ABI, on the same operands and bounds."""
import ctypes as C

import torch

import f16x3_util as U

DEV = 'cuda:0'
SITES = [(64, 128), (128, 256)]         # (Cin = planes, Cout) of layer1 and layer3 of the stem


def geom(M, Cin, Cout):
    from dsnt._lib import ConvGeom
    assert M % 32 == 0
    return ConvGeom(1, M // 32, 32, Cin, M // 32, 32, Cout, 1, 1, 1, 0, 1)


def workgroups(Cin, Cout):
    """W: the workgroups (= statistics rows) a launch of this shape takes once it has stages for all of them."""
    from dsnt import _lib
    g = geom(1 << 17, Cin, Cout)
    return _lib.fn('dsnt_conv1x1_fwd_stats_rows')(C.byref(g), 0)


_cache = {}


def operands(Cin, Cout, M):
    """CPU fp32 operands of one site at M rows (computed once per shape): y2 seen through bn3 + ReLU, the raw block input x,
    both weights and biases."""
    key = (Cin, Cout, M)
    if key in _cache:
        return _cache[key]
    r = U.rng('dsfuse%d_%d_%d' % key)
    o = {}
    o['y2'] = U.f32(r.standard_normal((M, Cin)))
    o['x'] = U.f32(r.standard_normal((M, Cin)) * 1.7 + 0.2)
    o['gamma'] = U.f32(r.uniform(0.5, 1.5, Cin))
    o['beta'] = U.f32(r.standard_normal(Cin) * 0.3)
    y64 = o['y2'].double()
    o['mu'] = y64.mean(0).float()
    o['istd'] = (1.0 / (y64.var(0, unbiased=False) + 1e-5).sqrt()).float()
    o['sc'] = o['gamma'] * o['istd']
    o['sh'] = o['beta'] - o['mu'] * o['sc']
    o['w3'] = U.f32(r.standard_normal((Cout, Cin)) * (2.0 / Cin) ** 0.5)
    o['wd'] = U.f32(r.standard_normal((Cout, Cin)) * (2.0 / Cin) ** 0.5 * 0.25)
    o['b3'] = U.f32(r.standard_normal(Cout) * 0.1)
    o['bd'] = U.f32(r.standard_normal(Cout) * 0.1)
    _cache[key] = o
    return o


def _bn_a_bound(o, M):
    act32 = torch.relu(o['y2'] * o['sc'] + o['sh'])
    return U.bmax(U.bn_bound(o['gamma'], o['beta'], M, DEV), U.dev_amax(act32.to(DEV), U.LOOSE_A))


def forward(Cin, Cout, M, flags=0):
    """(pair, fused): out, statistics rows, both bound slots of the two existing launches and of the fused one.
    flags: DSNT_CONV_SHARE_CHIP (2) on the conv3 launch of the pair and on the fused launch — the same plan for both."""
    from dsnt import _lib
    from dsnt._lib import ptr, call, BnTail
    o = operands(Cin, Cout, M)
    g = geom(M, Cin, Cout)
    assert _lib.fn('dsnt_conv1x1_fwd_ok')(C.byref(g))
    d = {k: v.to(DEV) for k, v in o.items()}
    p3, wb3 = U.prep_weights(d['w3'])
    pd, wbd = U.prep_weights(d['wd'])
    ab3, abd = _bn_a_bound(o, M), U.dev_amax(d['x'], U.LOOSE_A)
    rows = _lib.fn('dsnt_conv1x1_fwd_stats_rows')(C.byref(g), flags)
    asc, ash = d['gamma'][:1].expand(Cout).contiguous(), d['beta'][:1].expand(Cout).contiguous()
    n = d['w3'].numel()

    def outputs():
        y = torch.full((M, Cout), float('nan'), device=DEV)
        stats = torch.full((rows, 2, Cout), float('nan'), device=DEV)
        amax, amax_bn = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
        tl = BnTail()
        tl.amax, tl.amax_bn, tl.amax_scale, tl.amax_shift, tl.amax_relu = (amax.data_ptr(), amax_bn.data_ptr(), asc.data_ptr(),
                                                                            ash.data_ptr(), 1)
        return y, stats, amax, amax_bn, tl

    skip = torch.full((M, Cout), float('nan'), device=DEV)
    call('dsnt_conv1x1_fwd_f16x3', ptr(d['x']), ptr(pd), n, ptr(wbd), ptr(abd), ptr(d['bd']), ptr(skip), None, None, 0, None, None,
         C.byref(g), None)
    y, stats, amax, amax_bn, tl = outputs()
    call('dsnt_conv1x1_fwd_f16x3', ptr(d['y2']), ptr(p3), n, ptr(wb3), ptr(ab3), ptr(d['b3']), ptr(y), ptr(d['sc']), ptr(d['sh']), 1 | flags,
         ptr(skip), ptr(stats), C.byref(g), C.byref(tl))
    pair = dict(out=y, stats=stats, amax=amax, amax_bn=amax_bn)
    y, stats, amax, amax_bn, tl = outputs()
    call('dsnt_conv1x1_fwd_ds_f16x3', ptr(d['y2']), ptr(d['x']), ptr(p3), ptr(pd), n, ptr(wb3), ptr(wbd), ptr(ab3), ptr(abd),
         ptr(d['b3']), ptr(d['bd']), ptr(y), ptr(d['sc']), ptr(d['sh']), 1 | flags, ptr(stats), C.byref(g), C.byref(g), C.byref(tl))
    torch.cuda.synchronize()
    return pair, dict(out=y, stats=stats, amax=amax, amax_bn=amax_bn), rows


def forward_refs(Cin, Cout, M):
    """(fp64, fp32) out = conv3(relu(bn3(y2))) + b3 + ds(x) + b_ds."""
    o = operands(Cin, Cout, M)
    a32 = torch.relu(o['y2'] * o['sc'] + o['sh'])
    a64 = torch.relu(o['y2'].double() * o['sc'].double() + o['sh'].double())
    r64 = a64 @ o['w3'].double().t() + o['b3'].double() + o['x'].double() @ o['wd'].double().t() + o['bd'].double()
    r32 = a32 @ o['w3'].t() + o['b3'] + (o['x'] @ o['wd'].t() + o['bd'])
    return r64, r32
