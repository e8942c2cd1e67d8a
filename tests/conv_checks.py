"""The checking code of the kernel-level convolution tests (tests/test_conv_gpu.py, tests/test_bwd1_gpu.py), shared with
tests/test_plan_edges_gpu.py: one function per kernel family, each the whole comparison of that family against fp64 through the
C ABI — operands, launches, every assertion — for one case.  A function returns the figures it measured (maximum errors next to
the scales its bars are relative to), so that a caller can report them; the bars themselves live here and nowhere else.
At the end: conv_f32_edge, the comparison of tests/test_conv_f32_edges_gpu.py for the fp32 family of csrc/conv_f32.hip, and
conv_split_edge, that of tests/test_conv_split_edges_gpu.py for the tiled bf16x6 / fp16x3 kernels of csrc/conv_split6.hip, on
the same operands, guards and bars."""
import ctypes as C

import torch
import torch.nn.functional as F

from dsnt import synthetic


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def geom(N, H, W, Cin, Cout, R, S, stride, pad, dil):
    from dsnt._lib import ConvGeom
    Ho = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (S - 1) - 1) // stride + 1
    return ConvGeom(N, H, W, Cin, Ho, Wo, Cout, R, S, stride, pad, dil)


def conv_f16x3_vs_fp32_accuracy(case, pro, loose, flags=0):
    """fp16x3 forward (dsnt_conv_fwd_f16x3_ex) with bias, residual and statistics partial (one row per 128 output rows): 2e-5 of
    the output scale vs torch fp32, an fp64 check that its error is of fp32 size, column sums of the partial.
    flags: DSNT_CONV_SHARE_CHIP (2) for the launch on half of the chip."""
    import math
    from dsnt._lib import ptr, call
    N, H, W, Cin, Cout, k, stride, pad, dil = case
    dev = torch.device('cuda:0')
    tag = 'c' + '_'.join(map(str, case))
    x = synthetic.tensor(tag + 'x', (N, Cin, H, W), seed=1)
    w = synthetic.tensor(tag + 'w', (Cout, Cin, k, k), seed=1, scale=(2.0 / (Cin * k * k)) ** 0.5)
    b = synthetic.tensor(tag + 'b', (Cout,), seed=1, scale=0.1)
    sc = synthetic.tensor(tag + 's', (Cin,), seed=1, kind='uniform').abs() + 0.5
    sh = synthetic.tensor(tag + 'h', (Cin,), seed=1, scale=0.3)
    g = geom(N, H, W, Cin, Cout, k, k, stride, pad, dil)
    act = F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) if pro else x
    y32 = F.conv2d(act, w, b, stride=stride, padding=pad, dilation=dil)
    y64 = F.conv2d(act.double(), w.double(), b.double(), stride=stride, padding=pad, dilation=dil)
    res = synthetic.tensor(tag + 'r', tuple(y32.shape), seed=1)
    xd = nhwc(x).to(dev)
    wd = w.permute(0, 2, 3, 1).contiguous().to(dev)
    wb, ab = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    call('dsnt_amax', ptr(wd), wd.numel(), ptr(wb))
    assert wb.max().item() == wd.abs().max().item()
    planes = torch.empty(2 * wd.numel(), dtype=torch.float16, device=dev)
    call('dsnt_split_f16x2', ptr(wd), ptr(planes), wd.numel(), wd.numel(), ptr(wb))
    # the two planes carry the scaled weights to ~2^-23 of the largest
    s_w = 2.0 ** (13 - math.floor(math.log2(wb.max().item())))
    back = planes.view(2, -1).double().sum(0) / s_w
    assert (back - wd.reshape(-1).double()).abs().max().item() <= 2.0 ** -22 * wd.abs().max().item()
    ab[7] = act.abs().max().item() * loose            # any slot may hold the maximum
    bd, scd, shd, resd = b.to(dev), sc.to(dev), sh.to(dev), nhwc(res).to(dev)
    y = torch.empty(N, g.Ho, g.Wo, Cout, device=dev)
    M = N * g.Ho * g.Wo
    stats = torch.zeros((M + 127) // 128, 2, Cout, device=dev)
    call('dsnt_conv_fwd_f16x3_ex', ptr(xd), ptr(planes), wd.numel(), ptr(wb), ptr(ab), ptr(bd), ptr(y),
         ptr(scd) if pro else None, ptr(shd) if pro else None, 1 | flags, ptr(resd), None, ptr(stats), C.byref(g), None, None)
    got = y.cpu().permute(0, 3, 1, 2)
    scale = y32.abs().max().item()
    e32bar = (got - (y32 + res)).abs().max().item()
    assert e32bar <= 2e-5 * scale
    err16 = (got.double() - (y64 + res.double())).abs().max().item()
    err32 = ((y32 + res).double() - (y64 + res.double())).abs().max().item()
    assert err16 <= max(4 * err32, 2e-6 * scale), (err16, err32)
    yd = (y32 + res).permute(0, 2, 3, 1).reshape(M, Cout).double()
    s = stats.cpu().double().sum(0)
    es = (s[0] - yd.sum(0)).abs().max().item()
    assert es <= 1e-4 * max(1.0, yd.sum(0).abs().max().item())
    return dict(err_vs_fp32=e32bar, err16=err16, err32=err32, scale=scale, stats_err=es,
                stats_scale=max(1.0, yd.sum(0).abs().max().item()))


def wgrad_halo_f16x3(case, pro, relu):
    """The halo weight gradient (csrc/wgrad3.hip) vs fp64 autograd and its slab plan: plain call, slabs only + the table-driven
    reduction (the same bits), DSNT_WGRAD_SHARE_CHIP, accumulate."""
    from dsnt import _lib
    from dsnt._lib import ptr, call
    N, H, W, Cin, Cout = case
    dev = torch.device('cuda:0')
    tag = 'h' + '_'.join(map(str, case))
    g = geom(N, H, W, Cin, Cout, 3, 3, 1, 1, 1)
    assert _lib.fn('dsnt_conv_wgrad_halo_ok')(C.byref(g)) == 1
    x = synthetic.tensor(tag + 'x', (N, Cin, H, W), seed=1)
    sc = synthetic.tensor(tag + 's', (Cin,), seed=1, kind='uniform').abs() + 0.5
    sh = synthetic.tensor(tag + 'h', (Cin,), seed=1, scale=0.3)
    act = x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1) if pro else x
    act = (F.relu(act) if relu else act).double()
    w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(act, w, b, padding=1)
    gy = synthetic.tensor(tag + 'g', tuple(y.shape), seed=2) * 1e-4
    y.backward(gy.double())
    xd, gyd, scd, shd = nhwc(x).to(dev), nhwc(gy).to(dev), sc.to(dev), sh.to(dev)
    ab, gb = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    ab.fill_(act.abs().max().item() * 16.0)
    call('dsnt_amax', ptr(gyd), gyd.numel(), ptr(gb))
    nws = _lib.fn('dsnt_conv_wgrad_f16x3_ws_floats')(C.byref(g), 0)
    splits = _lib.fn('dsnt_conv_wgrad_f16x3_splits')(C.byref(g), 0)
    assert nws == splits * Cout * (9 * Cin + 1)
    ws = torch.full((nws,), float('nan'), device=dev)
    dw16, dw32 = torch.empty(Cout, 3, 3, Cin, device=dev), torch.empty(Cout, 3, 3, Cin, device=dev)
    db16, db32 = torch.empty(Cout, device=dev), torch.empty(Cout, device=dev)
    args = (ptr(xd), ptr(scd) if pro else None, ptr(shd) if pro else None, relu, ptr(gyd))
    call('dsnt_conv_wgrad_f16x3', *args, ptr(ws), ptr(dw16), ptr(db16), 0, ptr(ab), ptr(gb), C.byref(g))
    assert bool(torch.isfinite(ws).all()), 'a slab element was never written'
    ws32 = torch.empty(_lib.fn('dsnt_conv_wgrad_ws_floats')(C.byref(g)), device=dev)
    call('dsnt_conv_wgrad', *args, ptr(ws32), ptr(dw32), ptr(db32), 0, C.byref(g))
    ref = w.grad.permute(0, 2, 3, 1)
    scale = ref.abs().max().item()
    e16 = (dw16.cpu().double() - ref).abs().max().item()
    e32 = (dw32.cpu().double() - ref).abs().max().item()
    assert e16 <= 3e-5 * scale and e16 <= max(4 * e32, 2e-6 * scale), (e16, e32)
    eb = (db16.cpu().double() - b.grad).abs().max().item()
    assert eb <= 3e-5 * b.grad.abs().max().item()
    # slabs only + the table-driven reduction: the same bits; accumulate adds
    ws2 = torch.empty(nws, device=dev)
    dw2, db2 = torch.zeros_like(dw16), torch.zeros_like(db16)
    call('dsnt_conv_wgrad_f16x3', *args, ptr(ws2), None, None, 0, ptr(ab), ptr(gb), C.byref(g))
    assert torch.equal(ws, ws2)
    # DSNT_WGRAD_SHARE_CHIP (bit 1): four-wave workgroups of 32 input channels that leave half of every CU to the
    # other streams, over its own plan of (at most as many) slabs: every slab element written, the same gradient
    nws_s = _lib.fn('dsnt_conv_wgrad_f16x3_ws_floats')(C.byref(g), 2)
    splits_s = _lib.fn('dsnt_conv_wgrad_f16x3_splits')(C.byref(g), 2)
    assert nws_s == splits_s * Cout * (9 * Cin + 1) and splits_s <= splits
    ws3 = torch.full((nws_s,), float('nan'), device=dev)
    dw3, db3 = torch.empty_like(dw16), torch.empty_like(db16)
    call('dsnt_conv_wgrad_f16x3', *args, ptr(ws3), ptr(dw3), ptr(db3), 2, ptr(ab), ptr(gb), C.byref(g))
    assert bool(torch.isfinite(ws3).all())
    e3 = (dw3.cpu().double() - ref).abs().max().item()
    assert e3 <= 3e-5 * scale and e3 <= max(4 * e32, 2e-6 * scale), (e3, e32)
    assert (db3.cpu().double() - b.grad).abs().max().item() <= 3e-5 * b.grad.abs().max().item()
    if splits_s == splits:
        assert torch.equal(ws, ws3)      # same slabs: the two workgroup shapes add in the same order, bit for bit
    table = torch.tensor([[ws2.data_ptr(), dw2.data_ptr(), db2.data_ptr(), splits, Cout * 9 * Cin, Cout, 0]],
                         dtype=torch.int64).to(dev)
    call('dsnt_wgrad_reduce_all', ptr(table), 1, (Cout * 9 * Cin // 4 + (Cout + 3) // 4 + 63) // 64)
    assert torch.equal(dw2, dw16) and torch.equal(db2, db16)
    call('dsnt_conv_wgrad_f16x3', *args, ptr(ws), ptr(dw16), ptr(db16), 1, ptr(ab), ptr(gb), C.byref(g))
    assert (dw16.cpu().double() - 2 * ref).abs().max().item() <= 6e-5 * scale
    return dict(e16=e16, e32=e32, e_share=e3, scale=scale, bias_err=eb, bias_scale=b.grad.abs().max().item(),
                splits=splits, splits_share=splits_s)


def wgrad_1x1_f16x3(case, pro, relu):
    """The four-wave 1x1 weight gradient (csrc/wgrad1.hip) vs fp64: every slab element written, slabs-only + table-driven
    reduction bit-identical to the reduction inside the call, and the DSNT_WGRAD_SHARE_CHIP launch over its own plan."""
    from dsnt import _lib
    from dsnt._lib import ptr, call
    N, H, W, Cin, Cout = case
    dev = torch.device('cuda:0')
    tag = 'w1' + '_'.join(map(str, case))
    g = geom(N, H, W, Cin, Cout, 1, 1, 1, 0, 1)
    x = synthetic.tensor(tag + 'x', (N, Cin, H, W), seed=1)
    sc = synthetic.tensor(tag + 's', (Cin,), seed=1, kind='uniform').abs() + 0.5
    sh = synthetic.tensor(tag + 'h', (Cin,), seed=1, scale=0.3)
    act = x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1) if pro else x
    act = (F.relu(act) if relu else act).double()
    gy = synthetic.tensor(tag + 'g', (N, Cout, H, W), seed=2) * 1e-4
    a2 = act.permute(0, 2, 3, 1).reshape(-1, Cin)
    g2 = gy.double().permute(0, 2, 3, 1).reshape(-1, Cout)
    ref = (g2.t() @ a2).view(Cout, 1, 1, Cin)
    bref = g2.sum(0)
    xd, gyd, scd, shd = nhwc(x).to(dev), nhwc(gy).to(dev), sc.to(dev), sh.to(dev)
    ab, gb = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    ab.fill_(act.abs().max().item() * 16.0)
    call('dsnt_amax', ptr(gyd), gyd.numel(), ptr(gb))
    nws = _lib.fn('dsnt_conv_wgrad_f16x3_ws_floats')(C.byref(g), 0)
    splits = _lib.fn('dsnt_conv_wgrad_f16x3_splits')(C.byref(g), 0)
    assert nws == splits * Cout * (Cin + 1)
    ws = torch.full((nws,), float('nan'), device=dev)
    dw16, dw32 = torch.empty(Cout, 1, 1, Cin, device=dev), torch.empty(Cout, 1, 1, Cin, device=dev)
    db16, db32 = torch.empty(Cout, device=dev), torch.empty(Cout, device=dev)
    args = (ptr(xd), ptr(scd) if pro else None, ptr(shd) if pro else None, relu, ptr(gyd))
    call('dsnt_conv_wgrad_f16x3', *args, ptr(ws), ptr(dw16), ptr(db16), 0, ptr(ab), ptr(gb), C.byref(g))
    assert bool(torch.isfinite(ws).all()), 'a slab element was never written'
    ws32 = torch.empty(_lib.fn('dsnt_conv_wgrad_ws_floats')(C.byref(g)), device=dev)
    call('dsnt_conv_wgrad', *args, ptr(ws32), ptr(dw32), ptr(db32), 0, C.byref(g))
    scale = ref.abs().max().item()
    e16 = (dw16.cpu().double() - ref).abs().max().item()
    e32 = (dw32.cpu().double() - ref).abs().max().item()
    assert e16 <= 3e-5 * scale and e16 <= max(4 * e32, 2e-6 * scale), (e16, e32)
    eb = (db16.cpu().double() - bref).abs().max().item()
    assert eb <= 3e-5 * bref.abs().max().item()
    ws2 = torch.empty(nws, device=dev)
    dw2, db2 = torch.zeros_like(dw16), torch.zeros_like(db16)
    call('dsnt_conv_wgrad_f16x3', *args, ptr(ws2), None, None, 0, ptr(ab), ptr(gb), C.byref(g))      # slabs only
    assert torch.equal(ws, ws2)
    table = torch.tensor([[ws2.data_ptr(), dw2.data_ptr(), db2.data_ptr(), splits, Cout * Cin, Cout, 0]],
                         dtype=torch.int64).to(dev)
    call('dsnt_wgrad_reduce_all', ptr(table), 1, (Cout * Cin // 4 + (Cout + 3) // 4 + 63) // 64)
    assert torch.equal(dw2, dw16) and torch.equal(db2, db16)
    # DSNT_WGRAD_SHARE_CHIP: half as many (longer) slabs on half the CUs — its own plan, the same gradient
    nws_s = _lib.fn('dsnt_conv_wgrad_f16x3_ws_floats')(C.byref(g), 2)
    splits_s = _lib.fn('dsnt_conv_wgrad_f16x3_splits')(C.byref(g), 2)
    assert nws_s == splits_s * Cout * (Cin + 1) and splits_s <= splits
    ws3 = torch.full((nws_s,), float('nan'), device=dev)
    dw3, db3 = torch.empty_like(dw16), torch.empty_like(db16)
    call('dsnt_conv_wgrad_f16x3', *args, ptr(ws3), ptr(dw3), ptr(db3), 2, ptr(ab), ptr(gb), C.byref(g))
    assert bool(torch.isfinite(ws3).all())
    e3 = (dw3.cpu().double() - ref).abs().max().item()
    assert e3 <= 3e-5 * scale and e3 <= max(4 * e32, 2e-6 * scale), (e3, e32)
    assert (db3.cpu().double() - bref).abs().max().item() <= 3e-5 * bref.abs().max().item()
    return dict(e16=e16, e32=e32, e_share=e3, scale=scale, bias_err=eb, bias_scale=bref.abs().max().item(),
                splits=splits, splits_share=splits_s)


def wgrad_reduction_in_the_call(fields, pro):
    """dsnt_conv_wgrad_f16x3 on a route the two functions above do not reach (fields: the twelve of dsnt_conv_geom; the stem kernel
    of csrc/stem4.hip, the implicit GEMM of csrc/wgrad_gemm.hip): dw and dbias of the call equal, bit for bit, the table-driven
    reduction of a slabs-only call, and accumulate bit 0 adds.  Bars: those of the route's own accuracy test (stem 4e-6 / 8e-6 of
    the gradient's scale, stem_weight_gradient_on_its_own_kernel; otherwise 3e-5 / 6e-5, wgrad_halo_f16x3)."""
    from dsnt import _lib
    from dsnt._lib import ptr, call, ConvGeom
    N, H, W, Cin, Ho, Wo, Cout, R, S, stride, pad, dil = fields
    dev = torch.device('cuda:0')
    g = ConvGeom(*fields)
    route = _lib.fn('dsnt_conv_f16x3_route')(C.byref(g), 1)
    assert route in (0, 1) and (route == 0 or not pro)
    bar = 4e-6 if route == 1 else 3e-5
    tag = 'wr' + '_'.join(map(str, fields))
    x = synthetic.tensor(tag + 'x', (N, Cin, H, W), seed=1)
    sc = synthetic.tensor(tag + 's', (Cin,), seed=1, kind='uniform').abs() + 0.5
    sh = synthetic.tensor(tag + 'h', (Cin,), seed=1, scale=0.3)
    act = F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) if pro else x
    gy = synthetic.tensor(tag + 'g', (N, Cout, Ho, Wo), seed=2) * 1e-2
    ref = torch.nn.grad.conv2d_weight(act.double(), (Cout, Cin, R, S), gy.double(), stride=stride, padding=pad,
                                      dilation=dil).permute(0, 2, 3, 1)
    bref = gy.double().sum((0, 2, 3))
    scale, bscale = ref.abs().max().item(), bref.abs().max().item()
    if route == 1:
        bscale = max(bscale, gy.abs().sum().item() * 1e-3)
    xd, gyd, scd, shd = nhwc(x).to(dev), nhwc(gy).to(dev), sc.to(dev), sh.to(dev)
    ab, gb = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    ab.fill_(act.abs().max().item())
    call('dsnt_amax', ptr(gyd), gyd.numel(), ptr(gb))
    K = R * S * Cin
    nws = _lib.fn('dsnt_conv_wgrad_f16x3_ws_floats')(C.byref(g), 0)
    splits = _lib.fn('dsnt_conv_wgrad_f16x3_splits')(C.byref(g), 0)
    assert splits > 0 and nws == splits * Cout * (K + 1)
    ws, ws2 = torch.full((nws,), float('nan'), device=dev), torch.full((nws,), float('nan'), device=dev)
    dw, db = torch.empty(Cout, R, S, Cin, device=dev), torch.empty(Cout, device=dev)
    dw2, db2 = torch.zeros_like(dw), torch.zeros_like(db)
    args = (ptr(xd), ptr(scd) if pro else None, ptr(shd) if pro else None, 1, ptr(gyd))
    call('dsnt_conv_wgrad_f16x3', *args, ptr(ws), ptr(dw), ptr(db), 0, ptr(ab), ptr(gb), C.byref(g))
    assert bool(torch.isfinite(ws).all()), 'a slab element was never written'
    e = (dw.cpu().double() - ref).abs().max().item()
    eb = (db.cpu().double() - bref).abs().max().item()
    print('wgrad_reduction_in_the_call', fields, 'pro=%d' % pro, 'route', route, 'splits', splits, 'err', e, 'scale', scale,
          'bias err', eb, 'bias scale', bscale)
    assert e <= bar * scale and eb <= bar * bscale
    # slabs only + the table-driven reduction: the same bits
    call('dsnt_conv_wgrad_f16x3', *args, ptr(ws2), None, None, 0, ptr(ab), ptr(gb), C.byref(g))
    assert torch.equal(ws, ws2)
    table = torch.tensor([[ws2.data_ptr(), dw2.data_ptr(), db2.data_ptr(), splits, Cout * K, Cout, 0]], dtype=torch.int64).to(dev)
    call('dsnt_wgrad_reduce_all', ptr(table), 1, (Cout * K // 4 + (Cout + 3) // 4 + 63) // 64)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)
    # accumulate (bit 0) adds
    call('dsnt_conv_wgrad_f16x3', *args, ptr(ws), ptr(dw), ptr(db), 1, ptr(ab), ptr(gb), C.byref(g))
    e2 = (dw.cpu().double() - 2 * ref).abs().max().item()
    print('wgrad_reduction_in_the_call', fields, 'accumulate err', e2)
    assert e2 <= 2 * bar * scale
    assert (db.cpu().double() - 2 * bref).abs().max().item() <= 2 * bar * bscale
    return dict(err=e, err_accumulate=e2, scale=scale, bias_err=eb, splits=splits, route=route)


def conv3_stream_kernel(case, mode):
    """dsnt_conv_fwd_f16x3_stream (csrc/conv3s.hip) against dsnt_conv_fwd_f16x3_ex on the same operands and against torch fp64;
    mode: plain, pro, pro_res, res, bnb, pro_norelu, bnb_norelu."""
    from dsnt import _lib
    from dsnt._lib import ptr, call, BnBwdEpilogue
    N, H, W, Cin, Cout = case
    dev = torch.device('cuda:0')
    tag = 's3' + '_'.join(map(str, case))
    g = geom(N, H, W, Cin, Cout, 3, 3, 1, 1, 1)
    assert _lib.fn('dsnt_conv_fwd_stream_ok')(C.byref(g)) == 1
    M = N * H * W
    x = synthetic.tensor(tag + 'x', (N, Cin, H, W), seed=1)
    w = synthetic.tensor(tag + 'w', (Cout, Cin, 3, 3), seed=1, scale=(2.0 / (Cin * 9)) ** 0.5)
    b = synthetic.tensor(tag + 'b', (Cout,), seed=1, scale=0.1)
    sc = synthetic.tensor(tag + 's', (Cin,), seed=1, kind='uniform').abs() + 0.5
    sh = synthetic.tensor(tag + 'h', (Cin,), seed=1, scale=0.3)
    res = synthetic.tensor(tag + 'r', (N, Cout, H, W), seed=1)
    relu = 0 if mode.endswith('_norelu') else 1
    mode = mode.replace('_norelu', '')
    pro = mode in ('pro', 'pro_res')
    xd = nhwc(x).to(dev)
    wd = w.permute(0, 2, 3, 1).contiguous().to(dev)
    n = wd.numel()
    plain = torch.empty(2 * n, dtype=torch.float16, device=dev)
    strm = torch.full((2 * n,), float('nan'), dtype=torch.float16, device=dev)
    wb, wb2 = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    table = torch.tensor([[wd.data_ptr(), plain.data_ptr(), wb.data_ptr(), n, n, 0, 0],
                          [wd.data_ptr(), strm.data_ptr(), wb2.data_ptr(), n, n, Cout, Cin]], dtype=torch.int64).to(dev)
    call('dsnt_f16_prep_weights', ptr(table), 2, 7)
    assert torch.equal(wb, wb2)
    want = plain.view(2, Cout, 9, Cin // 16, 16).permute(0, 3, 2, 1, 4).contiguous().view(-1)
    assert torch.equal(want.view(torch.int16), strm.view(torch.int16))
    bd, scd, shd, resd = b.to(dev), sc.to(dev), sh.to(dev), nhwc(res).to(dev)
    tiles = M // 128
    if mode == 'bnb':
        # the launch as a data gradient: A = a gradient tensor, epilogue = ReLU mask of bn(xin) + the two BN-backward sums
        xin = nhwc(synthetic.tensor(tag + 'xin', (N, Cout, H, W), seed=3)).to(dev)
        mean = synthetic.tensor(tag + 'm', (Cout,), seed=4, scale=0.2).to(dev)
        invstd = (synthetic.tensor(tag + 'i', (Cout,), seed=5, kind='uniform').abs() + 0.5).to(dev)
        bsc = (synthetic.tensor(tag + 'bs', (Cout,), seed=6, kind='uniform') + 0.2).to(dev)
        bsh = synthetic.tensor(tag + 'bh', (Cout,), seed=7, scale=0.3).to(dev)
        bnb = BnBwdEpilogue(ptr(xin), ptr(bsc), ptr(bsh), ptr(mean), ptr(invstd), relu)
    ab = torch.zeros(64, device=dev)
    act = x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1) if pro else x
    if pro and relu:
        act = F.relu(act)
    ab[11] = act.abs().max().item() * 3.0
    outs = []
    for fn, planes in (('dsnt_conv_fwd_f16x3_ex', plain), ('dsnt_conv_fwd_f16x3_stream', strm)):
        y = torch.full((N, H, W, Cout), float('nan'), device=dev)
        stats = torch.full((tiles, 2, Cout), float('nan'), device=dev)
        amax = torch.zeros(64, device=dev)
        tail = _lib.BnTail()
        if mode != 'bnb':
            tail.amax = amax.data_ptr()
        call(fn, ptr(xd), ptr(planes), n, ptr(wb), ptr(ab), None if mode == 'bnb' else ptr(bd), ptr(y),
             ptr(scd) if pro else None, ptr(shd) if pro else None, relu,
             ptr(resd) if mode in ('res', 'pro_res') else None, None, ptr(stats), C.byref(g),
             C.byref(bnb) if mode == 'bnb' else None, C.byref(tail))
        outs.append((y, stats, amax))
    if mode == 'pro':       # DSNT_CONV_SHARE_CHIP (bit 1 of in_relu): fewer persistent workgroups, the same result bit for bit
        y2 = torch.full((N, H, W, Cout), float('nan'), device=dev)
        st2 = torch.full((tiles, 2, Cout), float('nan'), device=dev)
        call('dsnt_conv_fwd_f16x3_stream', ptr(xd), ptr(strm), n, ptr(wb), ptr(ab), ptr(bd), ptr(y2), ptr(scd), ptr(shd), relu | 2,
             None, None, ptr(st2), C.byref(g), None, None)
        assert torch.equal(y2, outs[1][0]) and torch.equal(st2, outs[1][1])
    torch.cuda.synchronize()
    (y0, st0, am0), (y1, st1, am1) = outs
    assert not bool(torch.isnan(y1).any()) and not bool(torch.isnan(st1).any())
    scale = y0.abs().max().item()
    # Cout 128 on 32-pixel-wide patches runs on v_mfma_f32_16x16x32_f16 (csrc/conv3s_mf.hip): an MFMA sums BOTH K-steps of a
    # pair, so the same products are added in another association — fp32 rounding of the 1152..3456-term sums, not bit identity
    mf16 = Cout == 128 and W % 32 == 0 and H % 4 == 0 and M // 128 > 128
    d01 = (y0 - y1).abs().max().item()
    if mode in ('plain', 'pro', 'bnb') and H % 8 == 0 and not mf16:   # (H % 8 != 0: _ex runs the implicit-GEMM kernel, K order (tap, channel))
        assert torch.equal(y0, y1)
    else:
        assert d01 <= (5e-7 if H % 8 == 0 else 2e-6) * scale
        if mode == 'bnb':        # the ReLU mask comes from the residual operand, not from the sums: the same zeros
            assert torch.equal(y0 == 0, y1 == 0)
    if mode == 'bnb':
        assert float((y1 == 0).float().mean()) > (0.2 if relu else -1.0)
    else:
        assert am1.max().item() == y1.abs().max().item()
    # statistics: other tiles, other order — the column sums agree to fp32 rounding of a 128-term sum
    for k in range(2):
        a0, a1 = st0[:, k].double().sum(0), st1[:, k].double().sum(0)
        assert (a0 - a1).abs().max().item() <= 2e-6 * max(1.0, st0[:, k].double().abs().sum(0).max().item())
    figs = dict(diff_vs_ex=d01, scale=scale)
    if mode != 'bnb':
        y64 = F.conv2d(act.double(), w.double(), b.double(), padding=1)
        if mode in ('res', 'pro_res'):
            y64 = y64 + res.double()
        y32 = F.conv2d(act, w, b, padding=1) + (res if mode in ('res', 'pro_res') else 0)
        got = y1.cpu().permute(0, 3, 1, 2).double()
        err16, err32 = (got - y64).abs().max().item(), (y32.double() - y64).abs().max().item()
        assert err16 <= max(4 * err32, 2e-6 * y64.abs().max().item()), (err16, err32)
        cols = y1.double().reshape(M, Cout)
        assert (st1[:, 0].double().sum(0) - cols.sum(0)).abs().max().item() <= 1e-4 * max(1.0, cols.sum(0).abs().max().item())
        assert (st1[:, 1].double().sum(0) - (cols * cols).sum(0)).abs().max().item() <= 1e-4 * (cols * cols).sum(0).max().item()
        figs.update(err16=err16, err32=err32, scale64=y64.abs().max().item())
    return figs


def conv3_stream_dgrad_apply(case, relu, big_mean):
    """dsnt_conv_dgrad_f16x3_stream_apply (csrc/conv3s.hip MODE 4) against the two launches it replaces — dsnt_bn_act_bwd_apply,
    then dsnt_conv_fwd_f16x3_stream on its output — and its dy_out against fp64."""
    from dsnt import _lib
    from dsnt._lib import ptr, call, BnBwdEpilogue, BnBwdApply
    N, H, W, Cin, Cout = case            # of the data-gradient launch: Cin = channels of dL/dy, Cout = channels of dL/dx
    dev = torch.device('cuda:0')
    tag = 's4' + '_'.join(map(str, case)) + str(relu) + str(big_mean)
    g = geom(N, H, W, Cin, Cout, 3, 3, 1, 1, 1)
    M = N * H * W
    w = synthetic.tensor(tag + 'w', (Cout, Cin, 3, 3), seed=1, scale=(2.0 / (Cin * 9)) ** 0.5)
    wd = w.permute(0, 2, 3, 1).contiguous().to(dev)
    n = wd.numel()
    strm = torch.empty(2 * n, dtype=torch.float16, device=dev)
    wb = torch.zeros(64, device=dev)
    table = torch.tensor([[wd.data_ptr(), strm.data_ptr(), wb.data_ptr(), n, n, Cout, Cin]], dtype=torch.int64).to(dev)
    call('dsnt_f16_prep_weights', ptr(table), 1, 7)
    # the BatchNorm behind the convolution: its input y, its vectors, the reduced coefficients; dz behind it (ReLU-masked)
    mu = synthetic.tensor(tag + 'mu', (Cin,), seed=2, scale=20.0 if big_mean else 0.5).to(dev)
    std = (synthetic.tensor(tag + 'sd', (Cin,), seed=3, kind='uniform').abs() + 0.5).to(dev)
    yin = (nhwc(synthetic.tensor(tag + 'y', (N, Cin, H, W), seed=4)).to(dev) * std + mu).contiguous()
    dz = nhwc(synthetic.tensor(tag + 'dz', (N, Cin, H, W), seed=5)).to(dev)
    dz = (dz * (nhwc(synthetic.tensor(tag + 'mk', (N, Cin, H, W), seed=6)).to(dev) > 0)).contiguous()
    invstd = (1.0 / std).contiguous()
    gamma = (synthetic.tensor(tag + 'ga', (Cin,), seed=7, kind='uniform') + 0.3).to(dev)
    scale = (gamma * invstd).contiguous()
    shift = torch.zeros(Cin, device=dev)
    xhat = (yin.view(M, Cin) - mu) * invstd
    coef = torch.cat([dz.view(M, Cin).mean(0), (dz.view(M, Cin) * xhat).mean(0)]).contiguous()
    # the BatchNorm in front of the convolution (the epilogue)
    xin = nhwc(synthetic.tensor(tag + 'xin', (N, Cout, H, W), seed=8)).to(dev)
    mean = synthetic.tensor(tag + 'm', (Cout,), seed=9, scale=0.2).to(dev)
    istd = (synthetic.tensor(tag + 'i', (Cout,), seed=10, kind='uniform').abs() + 0.5).to(dev)
    bsc = (synthetic.tensor(tag + 'bs', (Cout,), seed=11, kind='uniform') + 0.2).to(dev)
    bsh = synthetic.tensor(tag + 'bh', (Cout,), seed=12, scale=0.3).to(dev)
    bnb = BnBwdEpilogue(ptr(xin), ptr(bsc), ptr(bsh), ptr(mean), ptr(istd), relu)
    tiles = M // 128
    # reference: the apply launch, then the stream kernel on its output
    dy = torch.full((N, H, W, Cin), float('nan'), device=dev)
    call('dsnt_bn_act_bwd_apply', ptr(dz), ptr(yin), ptr(scale), ptr(shift), ptr(mu), ptr(invstd), ptr(coef), 0, ptr(dy), 0, M, Cin)
    dy64 = (scale.double() * (dz.view(M, Cin).double() - coef[:Cin].double() -
                              (yin.view(M, Cin).double() - mu.double()) * invstd.double() * coef[Cin:].double())).view(N, H, W, Cin)
    ab = torch.zeros(64, device=dev)
    ab[5] = float(dy64.abs().max()) * 2.5
    outs = []
    for fold, flags in ((False, 0), (True, 0), (True, 2)):
        out = torch.full((N, H, W, Cout), float('nan'), device=dev)
        stats = torch.full((tiles, 2, Cout), float('nan'), device=dev)
        amax = torch.zeros(64, device=dev)
        tail = _lib.BnTail()
        tail.amax = amax.data_ptr()
        dyo = torch.full((N, H, W, Cin), float('nan'), device=dev)
        if fold:
            ap = BnBwdApply(ptr(yin), ptr(scale), ptr(mu), ptr(invstd), ptr(coef))
            call('dsnt_conv_dgrad_f16x3_stream_apply', ptr(dz), C.byref(ap), ptr(dyo), ptr(strm), n, ptr(wb), ptr(ab), ptr(out),
                 ptr(stats), flags, C.byref(g), C.byref(bnb), C.byref(tail))
        else:
            call('dsnt_conv_fwd_f16x3_stream', ptr(dy), ptr(strm), n, ptr(wb), ptr(ab), None, ptr(out), None, None, 0, None, None,
                 ptr(stats), C.byref(g), C.byref(bnb), C.byref(tail))
        outs.append((out, stats, amax, dyo))
    torch.cuda.synchronize()
    (o0, s0, a0, _), (o1, s1, a1, d1), (o2, s2, a2, d2) = outs
    assert torch.equal(o1, o2) and torch.equal(d1, d2) and torch.equal(a1.max(), a2.max())      # the share flag changes no bit
    assert not bool(torch.isnan(d1).any()) and not bool(torch.isnan(o1).any()) and not bool(torch.isnan(s1).any())
    # dy_out against fp64, held to the apply kernel's own distance (x 4) plus the affine form's conditioning
    sc_dy = float(dy64.abs().max())
    e_ref, e_new = float((dy.double() - dy64).abs().max()), float((d1.double() - dy64).abs().max())
    cond = float((mu.abs() * invstd).max())
    assert e_new <= max(4 * e_ref, 2e-7 * (1 + cond) * sc_dy), (e_new, e_ref, cond)
    # the convolution's output: same mask, values to the rounding of dy carried through 9 Cin products
    so = float(o0.abs().max())
    tol = (4e-7 * (1 + cond)) * so
    d01 = (o0 - o1).abs().max().item()
    assert d01 <= tol, (d01, tol)
    if relu:
        assert float((o1 == 0).float().mean()) > 0.2 and float(((o0 == 0) != (o1 == 0)).float().mean()) <= 1e-5
    assert abs(a0.max().item() - a1.max().item()) <= tol
    for k in range(2):
        b0, b1 = s0[:, k].double().sum(0), s1[:, k].double().sum(0)
        assert (b0 - b1).abs().max().item() <= 4e-6 * (1 + cond) * max(1.0, s0[:, k].double().abs().sum(0).max().item())
    return dict(dy_err=e_new, dy_err_apply=e_ref, dy_bar=max(4 * e_ref, 2e-7 * (1 + cond) * sc_dy), out_diff=d01, out_bar=tol)


# ---------------------------------------------------------------- the 1x1 one-pass backward and the LDS-staged forward

def _bound(value, dev):
    return torch.full((64,), float(value), device=dev)


def _bwd1_reference(x, sc, sh, mu, istd, relu, dy, w):
    """fp64: dz_out, the two BatchNorm-backward sums, dW, db for y = conv1x1(relu?(x * sc + sh)) given dL/dy."""
    z = x * sc + sh
    act = torch.relu(z) if relu else z
    dx = dy @ w                                   # [M, Cin]
    if relu:
        dx = dx * (z > 0)
    xhat = (x - mu) * istd
    return dx, dx.sum(0), (dx * xhat).sum(0), dy.t() @ act, dy.sum(0), z


def conv1x1_backward_in_one_pass(case, mode, relu):
    """dsnt_conv1x1_bwd_f16x3 (csrc/bwd1.hip) against fp64; mode: apply, given, raw, raw_acc."""
    from dsnt import _lib
    from dsnt._lib import ptr, call, ConvGeom, BnBwdEpilogue, BnBwdApply
    N, H, W, Cin, Cout = case
    dev = torch.device('cuda:0')
    tag = 'b1' + '_'.join(map(str, case)) + mode
    M = N * H * W
    g = ConvGeom(N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, 1)
    assert _lib.fn('dsnt_conv1x1_bwd_ok')(C.byref(g))
    x = synthetic.tensor(tag + 'x', (M, Cin), seed=1)
    gamma = synthetic.tensor(tag + 'ga', (Cin,), seed=1, kind='uniform').abs() + 0.5
    beta = synthetic.tensor(tag + 'be', (Cin,), seed=1, scale=0.3)
    mu = x.double().mean(0).float()
    istd = (1.0 / (x.double().var(0, unbiased=False) + 1e-5).sqrt()).float()
    sc = gamma * istd
    sh = beta - mu * sc
    raw = mode.startswith('raw')           # no BatchNorm in front of the convolution: act(x) = x, dL/dx written as it is
    if raw:
        sc, sh, mu, istd = torch.ones(Cin), torch.zeros(Cin), torch.zeros(Cin), torch.zeros(Cin)
    w = synthetic.tensor(tag + 'w', (Cout, Cin), seed=2) * 0.05
    if mode == 'apply':
        # dY = y_scale (dz - c0 - (y - y_mean) y_invstd c1): the BatchNorm backward of the layer behind, folded in
        y = synthetic.tensor(tag + 'y', (M, Cout), seed=3)
        dz = synthetic.tensor(tag + 'dz', (M, Cout), seed=4) * 1e-3
        dz = dz * (synthetic.tensor(tag + 'mk', (M, Cout), seed=5) > 0)          # masked, as a data-gradient epilogue leaves it
        y_mean = y.double().mean(0).float()
        y_istd = (1.0 / (y.double().var(0, unbiased=False) + 1e-5).sqrt()).float()
        y_scale = (synthetic.tensor(tag + 'yg', (Cout,), seed=6, kind='uniform').abs() + 0.5) * y_istd
        yhat = (y.double() - y_mean.double()) * y_istd.double()
        coef = torch.stack([dz.double().mean(0), (dz.double() * yhat).mean(0)]).float()
        dy64 = y_scale.double() * (dz.double() - coef[0].double() - yhat * coef[1].double())
    else:
        dy = synthetic.tensor(tag + 'dy', (M, Cout), seed=4) * 1e-3
        dy64 = dy.double()
    ref_dz, ref_s1, ref_s2, ref_dw, ref_db, z64 = _bwd1_reference(x.double(), sc.double(), sh.double(), mu.double(), istd.double(),
                                                                   relu, dy64, w.double())
    # device side
    xd, scd, shd, mud, isd = (t.to(dev) for t in (x, sc, sh, mu, istd))
    wdt = w.t().contiguous().to(dev)                                  # the data gradient's filter [Cin][Cout]
    wb = torch.zeros(64, device=dev)
    call('dsnt_amax', ptr(wdt), wdt.numel(), ptr(wb))
    planes = torch.empty(2 * wdt.numel(), dtype=torch.float16, device=dev)
    call('dsnt_split_f16x2', ptr(wdt), ptr(planes), wdt.numel(), wdt.numel(), ptr(wb))
    act_max = (torch.relu(z64) if relu else z64).abs().max().item()
    ab = _bound(act_max * 3.0, dev)
    gb = _bound(dy64.abs().max().item() * 5.0, dev)                  # loose, as the analytic bound of the engine is
    xs = BnBwdEpilogue(ptr(xd), None, None, None, None, 0) if raw else BnBwdEpilogue(ptr(xd), ptr(scd), ptr(shd), ptr(mud), ptr(isd), relu)
    flags = 1 if mode == 'raw_acc' else 0
    prev = synthetic.tensor(tag + 'pv', (M, Cin), seed=7) * 1e-3 if flags else None
    if mode == 'apply':
        yd, dzd = y.to(dev), dz.to(dev)
        ysd, ymd, yid, cfd = y_scale.to(dev), y_mean.to(dev), y_istd.to(dev), coef.contiguous().to(dev)
        ap = BnBwdApply(ptr(yd), ptr(ysd), ptr(ymd), ptr(yid), ptr(cfd))
        dyd, apref = dzd, C.byref(ap)
    else:
        dyd, apref = dy.to(dev), None
    splits = _lib.fn('dsnt_conv1x1_bwd_splits')(C.byref(g), 0)
    nws = _lib.fn('dsnt_conv1x1_bwd_ws_floats')(C.byref(g), 0)
    assert nws == splits * Cout * (Cin + 1) and 0 < splits <= 512
    ws = torch.full((nws,), float('nan'), device=dev)
    stats = torch.full((splits, 2, Cin), float('nan'), device=dev)
    dz_out = prev.to(dev) if flags else torch.full((M, Cin), float('nan'), device=dev)
    if flags:
        ref_dz = ref_dz + prev.double()
    amax = torch.zeros(64, device=dev)
    call('dsnt_conv1x1_bwd_f16x3', C.byref(xs), ptr(dyd), apref, ptr(planes), wdt.numel(), ptr(wb), ptr(ab), ptr(gb),
         ptr(dz_out), None if raw else ptr(stats), ptr(ws), ptr(amax), flags, C.byref(g))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws).all()) and bool(torch.isfinite(dz_out).all())
    assert raw or bool(torch.isfinite(stats).all())
    # data gradient (elements whose pre-activation sits at the kink may take either side)
    got = dz_out.cpu().double()
    sure = (z64.abs() > 1e-5) if relu else torch.ones_like(z64, dtype=torch.bool)
    scale = ref_dz.abs().max().item()
    e = ((got - ref_dz) * sure).abs().max().item()
    assert e <= 2e-6 * scale, (e, scale)
    assert abs(amax.max().item() - dz_out.abs().max().item()) == 0.0
    # the BatchNorm-backward sums: one partial row per workgroup
    if not raw:
        s = stats.cpu().double().sum(0)
        unsure1 = ((got.abs() + ref_dz.abs()) * ~sure).sum(0)
        assert ((s[0] - ref_s1).abs() <= 1e-5 * ref_dz.abs().sum(0) + unsure1 + 1e-12).all()
        xhat = ((x.double() - mu.double()) * istd.double()).abs()
        assert ((s[1] - ref_s2).abs() <= 1e-5 * (ref_dz.abs() * xhat).sum(0) + unsure1 * xhat.max() + 1e-12).all()
    # weight and bias gradient through the table-driven slab reduction
    dw, db = torch.zeros(Cout, Cin, device=dev), torch.zeros(Cout, device=dev)
    table = torch.tensor([[ws.data_ptr(), dw.data_ptr(), db.data_ptr(), splits, Cout * Cin, Cout, 0]],
                         dtype=torch.int64).to(dev)
    call('dsnt_wgrad_reduce_all', ptr(table), 1, (Cout * Cin // 4 + (Cout + 3) // 4 + 63) // 64)
    ew = (dw.cpu().double() - ref_dw).abs().max().item()
    assert ew <= 3e-6 * ref_dw.abs().max().item(), (ew, ref_dw.abs().max().item())
    eb = (db.cpu().double() - ref_db).abs().max().item()
    assert eb <= 3e-6 * max(ref_db.abs().max().item(), dy64.abs().sum(0).max().item() * 1e-2), eb
    # a second launch writes the same bits (fixed summation order, no atomics on the results)
    ws2, stats2 = torch.empty_like(ws), torch.empty_like(stats)
    dz2 = prev.to(dev) if flags else torch.empty_like(dz_out)
    call('dsnt_conv1x1_bwd_f16x3', C.byref(xs), ptr(dyd), apref, ptr(planes), wdt.numel(), ptr(wb), ptr(ab), ptr(gb),
         ptr(dz2), None if raw else ptr(stats2), ptr(ws2), None, flags, C.byref(g))
    assert torch.equal(ws, ws2) and (raw or torch.equal(stats, stats2)) and torch.equal(dz_out, dz2)
    return dict(dz_err=e, dz_scale=scale, dw_err=ew, dw_scale=ref_dw.abs().max().item(), splits=splits)


def conv1x1_forward_lds_staged(case, pro, res):
    """dsnt_conv1x1_fwd_f16x3 (csrc/fwd1.hip) against fp64 and against dsnt_conv_fwd_f16x3_ex on the same operands: output,
    one-row-per-workgroup statistics, both operand-bound outputs, bit-reproducible; DSNT_CONV_SHARE_CHIP changes no value."""
    from dsnt import _lib
    from dsnt._lib import ptr, call, ConvGeom, BnTail
    N, H, W, Cin, Cout = case
    dev = torch.device('cuda:0')
    tag = 'f1' + '_'.join(map(str, case))
    M = N * H * W
    g = ConvGeom(N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, 1)
    assert _lib.fn('dsnt_conv1x1_fwd_ok')(C.byref(g))
    x = synthetic.tensor(tag + 'x', (M, Cin), seed=1)
    sc = synthetic.tensor(tag + 's', (Cin,), seed=1, kind='uniform').abs() + 0.5
    sh = synthetic.tensor(tag + 'h', (Cin,), seed=1, scale=0.3)
    w = synthetic.tensor(tag + 'w', (Cout, Cin), seed=2) * 0.05
    b = synthetic.tensor(tag + 'b', (Cout,), seed=2, scale=0.1)
    r = synthetic.tensor(tag + 'r', (M, Cout), seed=3)
    act = torch.relu(x.double() * sc.double() + sh.double()) if pro else x.double()
    ref = act @ w.double().t() + b.double() + (r.double() if res else 0.0)
    xd, scd, shd, wd, bd, rd = (t.to(dev) for t in (x, sc, sh, w, b, r))
    wb = torch.zeros(64, device=dev)
    call('dsnt_amax', ptr(wd), wd.numel(), ptr(wb))
    planes = torch.empty(2 * wd.numel(), dtype=torch.float16, device=dev)
    call('dsnt_split_f16x2', ptr(wd), ptr(planes), wd.numel(), wd.numel(), ptr(wb))
    ab = torch.full((64,), act.abs().max().item() * 3.0, device=dev)
    asc = (synthetic.tensor(tag + 'as', (Cout,), seed=4, kind='uniform').abs() + 0.5).to(dev)
    ash = synthetic.tensor(tag + 'ah', (Cout,), seed=4, scale=0.2).to(dev)

    def run(flags, name='dsnt_conv1x1_fwd_f16x3'):
        y = torch.full((M, Cout), float('nan'), device=dev)
        amax, amax_bn = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
        tl = BnTail()
        tl.amax, tl.amax_bn, tl.amax_scale, tl.amax_shift, tl.amax_relu = (amax.data_ptr(), amax_bn.data_ptr(), asc.data_ptr(),
                                                                            ash.data_ptr(), 1)
        common = (ptr(xd), ptr(planes), wd.numel(), ptr(wb), ptr(ab), ptr(bd), ptr(y), ptr(scd) if pro else None,
                  ptr(shd) if pro else None, 1 | flags, ptr(rd) if res else None)
        if name == 'dsnt_conv1x1_fwd_f16x3':
            rows = _lib.fn('dsnt_conv1x1_fwd_stats_rows')(C.byref(g), flags)
            stats = torch.full((rows, 2, Cout), float('nan'), device=dev)
            call(name, *common, ptr(stats), C.byref(g), C.byref(tl))
        else:
            rows = (M + 127) // 128
            stats = torch.full((rows, 2, Cout), float('nan'), device=dev)
            call(name, *common, None, ptr(stats), C.byref(g), None, C.byref(tl))
        torch.cuda.synchronize()
        return y, stats, amax, amax_bn, rows

    y, stats, amax, amax_bn, rows = run(0)
    assert 0 < rows <= 512 and bool(torch.isfinite(y).all()) and bool(torch.isfinite(stats).all())
    scale = ref.abs().max().item()
    e = (y.cpu().double() - ref).abs().max().item()
    assert e <= 2e-6 * scale, (e, scale)
    s = stats.cpu().double().sum(0)
    assert ((s[0] - ref.sum(0)).abs() <= 1e-5 * ref.abs().sum(0)).all()
    assert ((s[1] - (ref * ref).sum(0)).abs() <= 1e-5 * (ref * ref).sum(0)).all()
    assert float(amax.max()) == float(y.abs().max())
    want_bn = torch.relu(y * asc + ash).abs().max()
    assert abs(float(amax_bn.max()) - float(want_bn)) <= 1e-6 * float(want_bn)
    # the first streaming kernel on the same operands
    y0, stats0, amax0, _, _ = run(0, 'dsnt_conv_fwd_f16x3_ex')
    assert (y - y0).abs().max().item() <= 2e-6 * scale
    assert ((stats.double().sum(0) - stats0.double().sum(0)).abs() <= 1e-5 * stats0.double().abs().sum(0) + 1e-6).all()
    # bit-reproducible, and the share flag (fewer workgroups, other statistics rows) changes no output value
    y2, stats2, _, _, _ = run(0)
    assert torch.equal(y, y2) and torch.equal(stats, stats2)
    y3, stats3, _, _, rows3 = run(2)
    assert torch.equal(y, y3) and rows3 <= rows
    assert ((stats3.double().sum(0) - stats.double().sum(0)).abs() <= 1e-5 * stats.double().abs().sum(0) + 1e-6).all()
    return dict(err=e, scale=scale, rows=rows, rows_share=rows3)


# ---------------------------------------------------------------- the stem's space-to-depth convolution (csrc/stem4.hip)

def _stem_tag(prefix, N, Ho, Wo):
    return prefix + ('%d_%d' % (N, Ho) if Wo == Ho else '%d_%d_%d' % (N, Ho, Wo))


def stem_forward_on_its_halo_kernel(N, Ho, Wo, with_bias):
    """dsnt_stem4_fwd_f16x3 — a 4x4 / stride 1 / pad 1 convolution of the 16-channel [N][Ho + 1][Wo + 1] image, 64 output channels —
    against the tiled fp16x3 kernel on the same operands (bit-identical outputs), against torch in fp64, with its statistics and
    the bound of its output; refusals."""
    from dsnt import _lib
    from dsnt._lib import ptr, ConvGeom, BnTail
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    Hi, Wi = Ho + 1, Wo + 1
    g = ConvGeom(N, Hi, Wi, 16, Ho, Wo, 64, 4, 4, 1, 1, 1)
    assert _lib.fn('dsnt_stem4_fwd_ok')(C.byref(g)) == 1
    tag = _stem_tag('stem', N, Ho, Wo)
    x = synthetic.tensor(tag + 'x', (N, Hi, Wi, 16), seed=1).to(dev)
    w = (synthetic.tensor(tag + 'w', (64, 4, 4, 16), seed=2) * 0.1).to(dev)
    b = synthetic.tensor(tag + 'b', (64,), seed=3).to(dev) if with_bias else None
    wb, ab = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    planes = torch.empty(2 * w.numel(), dtype=torch.float16, device=dev)
    assert _lib.fn('dsnt_amax')(ptr(w), w.numel(), ptr(wb), st) == 0
    assert _lib.fn('dsnt_amax')(ptr(x), x.numel(), ptr(ab), st) == 0
    assert _lib.fn('dsnt_split_f16x2')(ptr(w), ptr(planes), w.numel(), w.numel(), ptr(wb), st) == 0
    M = N * Ho * Wo
    rows = _lib.fn('dsnt_stem4_fwd_stats_rows')(C.byref(g))
    assert 0 < rows <= N * (Ho // 4) * (Wo // 32)
    y = torch.full((N, Ho, Wo, 64), float('nan'), device=dev)
    part = torch.full((rows, 2, 64), float('nan'), device=dev)
    am = torch.zeros(64, device=dev)
    tail = BnTail()
    tail.amax = am.data_ptr()
    assert _lib.fn('dsnt_stem4_fwd_f16x3')(ptr(x), ptr(planes), w.numel(), ptr(wb), ptr(ab), ptr(b), ptr(y), ptr(part), C.byref(g),
                                           C.byref(tail), st) == 0
    # the tiled kernel on the same planes and bounds
    y_t = torch.empty_like(y)
    part_t = torch.empty((M + 127) // 128, 2, 64, device=dev)
    assert _lib.fn('dsnt_conv_fwd_f16x3_ex')(ptr(x), ptr(planes), w.numel(), ptr(wb), ptr(ab), ptr(b), ptr(y_t), None, None, 0, None, None,
                                             ptr(part_t), C.byref(g), None, None, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, y_t)
    ref = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2),
                                     None if b is None else b.double(), stride=1, padding=1).permute(0, 2, 3, 1)
    assert ref.shape == y.shape
    e = (y.double() - ref).abs().max().item()
    assert e <= 2e-6 * max(1.0, ref.abs().max().item())
    s1, s2 = part[:, 0].double().sum(0), part[:, 1].double().sum(0)
    yd = y.double().reshape(-1, 64)
    assert (s1 - yd.sum(0)).abs().max().item() <= 1e-5 * max(1.0, yd.abs().sum(0).max().item())
    assert (s2 - (yd * yd).sum(0)).abs().max().item() <= 1e-5 * (yd * yd).sum(0).max().item()
    assert am.max().item() == y.abs().max().item()
    # without statistics / bound; refusals
    y2 = torch.empty_like(y)
    assert _lib.fn('dsnt_stem4_fwd_f16x3')(ptr(x), ptr(planes), w.numel(), ptr(wb), ptr(ab), ptr(b), ptr(y2), None, C.byref(g), None, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(y2, y)
    bad = ConvGeom(N, Hi, Wi, 16, Ho, Wo, 128, 4, 4, 1, 1, 1)
    assert _lib.fn('dsnt_stem4_fwd_ok')(C.byref(bad)) == 0
    bad3 = ConvGeom(N, Ho, Wo, 16, Ho, Wo, 64, 3, 3, 1, 1, 1)
    assert _lib.fn('dsnt_stem4_fwd_ok')(C.byref(bad3)) == 0
    assert _lib.fn('dsnt_stem4_fwd_f16x3')(ptr(x), ptr(planes), w.numel(), ptr(wb), ptr(ab), ptr(b), ptr(y2), None, C.byref(bad3), None, st) != 0
    return dict(err=e, scale=max(1.0, ref.abs().max().item()), rows=rows)


def stem_weight_gradient_on_its_own_kernel(N, Ho, Wo):
    """The weight gradient of the same convolution (stem4_wgrad_kernel, reached through dsnt_conv_wgrad_f16x3) against torch in
    fp64, with and without the in-call reduction, accumulating, and the refusal of a BatchNorm prologue."""
    from dsnt import _lib
    from dsnt._lib import ptr, ConvGeom
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    Hi, Wi = Ho + 1, Wo + 1
    g = ConvGeom(N, Hi, Wi, 16, Ho, Wo, 64, 4, 4, 1, 1, 1)
    tag = _stem_tag('stemw', N, Ho, Wo)
    x = synthetic.tensor(tag + 'x', (N, Hi, Wi, 16), seed=1).to(dev)
    gy = (synthetic.tensor(tag + 'g', (N, Ho, Wo, 64), seed=2) * 1e-2).to(dev)
    ab, gb = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    assert _lib.fn('dsnt_amax')(ptr(x), x.numel(), ptr(ab), st) == 0
    assert _lib.fn('dsnt_amax')(ptr(gy), gy.numel(), ptr(gb), st) == 0
    splits = _lib.fn('dsnt_conv_wgrad_f16x3_splits')(C.byref(g), 0)
    nws = _lib.fn('dsnt_conv_wgrad_f16x3_ws_floats')(C.byref(g), 0)
    assert 0 < splits <= N * (Ho // 4) * (Wo // 32) and nws == splits * (64 * 256 + 64)
    assert _lib.fn('dsnt_conv_wgrad_ws_floats')(C.byref(g)) >= nws
    ws = torch.full((nws,), float('nan'), device=dev)
    dw, db = torch.empty(64, 4, 4, 16, device=dev), torch.empty(64, device=dev)
    wg = _lib.fn('dsnt_conv_wgrad_f16x3')
    assert wg(ptr(x), None, None, 0, ptr(gy), ptr(ws), ptr(dw), ptr(db), 0, ptr(ab), ptr(gb), C.byref(g), st) == 0
    torch.cuda.synchronize()
    ref = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (64, 16, 4, 4), gy.double().permute(0, 3, 1, 2),
                                      stride=1, padding=1).permute(0, 2, 3, 1)
    refb = gy.double().sum((0, 1, 2))
    assert not torch.isnan(ws).any()
    e = (dw.double() - ref).abs().max().item()
    assert e <= 4e-6 * ref.abs().max().item()
    assert (db.double() - refb).abs().max().item() <= 4e-6 * max(refb.abs().max().item(), gy.abs().sum().item() * 1e-3)
    # the slabs alone add up to the same gradient (what the engine's one reduction per bucket does), and accumulate adds
    slabs = ws[:splits * 64 * 256].view(splits, 64, 4, 4, 16).double().sum(0)
    assert (slabs - ref).abs().max().item() <= 4e-6 * ref.abs().max().item()
    assert wg(ptr(x), None, None, 0, ptr(gy), ptr(ws), ptr(dw), ptr(db), 1, ptr(ab), ptr(gb), C.byref(g), st) == 0
    torch.cuda.synchronize()
    assert (dw.double() - 2 * ref).abs().max().item() <= 8e-6 * ref.abs().max().item()
    sc, sh = torch.ones(16, device=dev), torch.zeros(16, device=dev)
    assert wg(ptr(x), ptr(sc), ptr(sh), 0, ptr(gy), ptr(ws), None, None, 0, ptr(ab), ptr(gb), C.byref(g), st) != 0
    return dict(err=e, scale=ref.abs().max().item(), splits=splits)


# ---------------------------------------------------------------- the fp32 family at its plan edges (csrc/conv_f32.hip, conv_epilogue.h)

SENT = -777.0               # what output buffers hold before a launch: no output of these cases comes near it
FRONT = 64                  # sentinel floats in front of a buffer (256 bytes: the buffer keeps its 16-byte alignment)
F32_BAR = 2e-5              # outputs, of max |reference|: the project's fp32 bar (tests/test_conv_gpu.py)
SUM_BAR = 1e-5              # per-tile column sums, of the column's sum of absolute values (test_native_strided_data_gradient)
ULP = 2.0 ** -23            # amax_bn: one fmaf on the stored value, rounded once (2^-24 of the result), against fp64
CONV_F32_MODES = ('fwd', 'pro_relu', 'pro_norelu', 'inplace', 'bnb_relu', 'bnb_norelu')


class Guarded:
    """rows x cols floats on the device, a block of sentinels in front and `guard_rows` rows of them behind; the payload starts
    as sentinels too (or as `init`).  The kernels address y and the statistics with a pitch of exactly Cout, so a column past
    Cout of row m IS column 0.. of row m + 1: an overrun shows as a wrong value there, and in the rows behind for the last row."""

    def __init__(self, rows, cols, dev, init=None, guard_rows=128):
        self.n = rows * cols
        self.buf = torch.full((FRONT + self.n + guard_rows * cols,), SENT, device=dev)
        self.t = self.buf[FRONT:FRONT + self.n].view(rows, cols)
        if init is not None:
            self.t.copy_(init)

    def intact(self):
        return bool((self.buf[:FRONT] == SENT).all()) and bool((self.buf[FRONT + self.n:] == SENT).all())


def _f32_same(a, b):
    """Two launches' outputs (Guarded buffers, guards included, and bound slots) hold the same bits."""
    return all(torch.equal(p.buf if isinstance(p, Guarded) else p, q.buf if isinstance(q, Guarded) else q) for p, q in zip(a, b))


_f32_cache = {}


def _fields(case):
    """(N, H, W, Cin, Cout, R, S, stride, pad, dil) of a CONV_F32 case (nine fields, a k x k filter) or a CONV_SPLIT case (ten)."""
    return tuple(case) if len(case) == 10 else tuple(case[:5]) + (case[5],) + tuple(case[5:])


def _f32_operands(case):
    """Host operands of one case and its fp64 convolutions (computed once per case, shared by its modes, never written to)."""
    if case not in _f32_cache:
        _f32_cache.clear()              # the cases come in order: one at a time is enough
        N, H, W, Cin, Cout, R, S, stride, pad, dil = _fields(case)
        tag = ('f32e' if len(case) == 9 else 'spl') + '_'.join(map(str, case))
        g = geom(N, H, W, Cin, Cout, R, S, stride, pad, dil)
        M = N * g.Ho * g.Wo
        o = dict(g=g, M=M, tag=tag)
        o['x'] = synthetic.tensor(tag + 'x', (N, Cin, H, W), seed=1)
        o['w'] = synthetic.tensor(tag + 'w', (Cout, Cin, R, S), seed=1, scale=(2.0 / (Cin * R * S)) ** 0.5)
        o['b'] = synthetic.tensor(tag + 'b', (Cout,), seed=1, scale=0.1)
        o['sc'] = synthetic.tensor(tag + 's', (Cin,), seed=1, kind='uniform').abs() + 0.5
        o['sh'] = synthetic.tensor(tag + 'h', (Cin,), seed=1, scale=0.3)
        o['r1'] = synthetic.tensor(tag + 'r1', (M, Cout), seed=2)
        o['r2'] = synthetic.tensor(tag + 'r2', (M, Cout), seed=3)
        o['asc'] = synthetic.tensor(tag + 'as', (Cout,), seed=4, kind='uniform') + 0.25        # both signs
        o['ash'] = synthetic.tensor(tag + 'ah', (Cout,), seed=4, scale=0.5)
        o['conv'] = {}
        _f32_cache[case] = o
    return _f32_cache[case]


def _f32_conv64(o, case, sc=None, sh=None, relu=0, dtype=torch.float64):
    """F.conv2d in fp64 (or wholly in `dtype`) on relu?(x * sc + sh) or on x, as [M][Cout]; the three forms on the case's own
    vectors are kept."""
    N, H, W, Cin, Cout, R, S, stride, pad, dil = _fields(case)
    key = None if sc is None else relu if sc is o['sc'] else -1
    if key != -1:
        key = (key, dtype)
    if key in o['conv']:
        return o['conv'][key]
    a = o['x'].to(dtype)
    if sc is not None:
        a = a * sc.to(dtype).view(1, -1, 1, 1) + sh.to(dtype).view(1, -1, 1, 1)
        a = F.relu(a) if relu else a
    y = F.conv2d(a, o['w'].to(dtype), None, stride=stride, padding=pad, dilation=dil).permute(0, 2, 3, 1).reshape(o['M'], Cout)
    if key != -1:
        o['conv'][key] = y
    return y


def _f32_tile_sums(got, weight, bm, tiles, tile_of=None):
    """fp64 per-tile column sums of got * weight and of |got * weight|; tile_of: the tile index of every row (int64), without it
    tiles of bm consecutive rows (the last one short)."""
    M, Cc = got.shape
    if tile_of is None:
        tile_of = torch.arange(M) // bm
    v = got * weight
    return (torch.zeros(tiles, Cc, dtype=torch.float64).index_add_(0, tile_of, v),
            torch.zeros(tiles, Cc, dtype=torch.float64).index_add_(0, tile_of, v.abs()))


def _f32_check_stats(st, got, second, bm, tiles, what, tile_of=None):
    """The statistics rows [tiles][2][Cout] of a launch against fp64 sums over the launch's OWN output `got`: row 0 the column
    sums, row 1 the sums of got * second; every element overwritten, nothing behind them touched.  tile_of: see _f32_tile_sums."""
    assert st.intact(), '%s: statistics written outside [tiles][2][Cout]' % what
    s = st.t.cpu().double().view(tiles, 2, -1)
    assert bool((s != SENT).all()), '%s: %d statistics elements never written' % (what, int((s == SENT).sum()))
    worst = 0.0
    for row, wgt in ((0, torch.ones_like(got)), (1, second)):
        want, mag = _f32_tile_sums(got, wgt, bm, tiles, tile_of)
        err = (s[:, row] - want).abs()
        bad = ~(err <= SUM_BAR * mag)
        assert not bool(bad.any()), '%s: statistics row %d: %d elements off, worst %.3e of the column\'s sum of absolute values' % (
            what, row, int(bad.sum()), float((err / mag.clamp_min(1e-300))[bad].max()))
        worst = max(worst, float((err / mag.clamp_min(1e-300)).max()))
    return worst


def _out_bounds(relu, am, amb, ascd, ashd):
    """A dsnt_out_bounds asking for amax and, with amb, for amax_bn under amax_relu = relu."""
    from dsnt._lib import BnTail
    t = BnTail()
    t.amax = am.data_ptr()
    if amb is not None:
        t.amax_bn, t.amax_scale, t.amax_shift, t.amax_relu = amb.data_ptr(), ascd.data_ptr(), ashd.data_ptr(), relu
    return t


def _bnb_operands(tag, M, Cout):
    """Host operands of a BatchNorm-backward epilogue over [M][Cout]: the BatchNorm's input, scale (both signs, away from zero),
    shift, mean, invstd, and the fp64 pre-activation z = x * scale + shift — none of it within 1e-3 of the kink."""
    xin = synthetic.tensor(tag + 'xin', (M, Cout), seed=5)
    bsc = synthetic.tensor(tag + 'bs', (Cout,), seed=6, kind='uniform')
    bsc = torch.sign(bsc) * (bsc.abs() + 0.5)                              # both signs, away from zero
    bsh = synthetic.tensor(tag + 'bh', (Cout,), seed=7, scale=0.3)
    bmu = synthetic.tensor(tag + 'bm', (Cout,), seed=8, scale=0.2)
    bis = synthetic.tensor(tag + 'bi', (Cout,), seed=9, kind='uniform').abs() + 0.5
    z = xin.double() * bsc.double() + bsh.double()
    near = z.abs() < 1e-3           # two fp32 evaluations may disagree about a pre-activation at the kink: move those away
    xin = (xin.double() + torch.where(near, torch.sign(z) * torch.sign(bsc.double()) * 4e-3 / bsc.double().abs(),
                                      torch.zeros_like(z))).float()
    z = xin.double() * bsc.double() + bsh.double()
    assert float(z.abs().min()) >= 1e-3
    return xin, bsc, bsh, bmu, bis, z


def conv_f32_edge(case, mode):
    """One case of tests/plan_edge_cases.py CONV_F32 in one mode, against torch fp64 on the CPU, through the C ABI.  Every launch
    writes into sentinel-filled buffers with guards and runs twice into fresh ones (the same bits).  Modes:
      fwd / pro_relu / pro_norelu   bias, res1, res2 and statistics; without / with in_scale, in_shift (in_relu 1 / 0).  Through
                    dsnt_conv_fwd (where the case is small enough: the K-split kernel) and through dsnt_conv_fwd_ex with a
                    dsnt_out_bounds (always a tile kernel), amax_relu 1 and 0: y against the reference; amax == max |y| as floats;
                    amax_bn against relu?(y s + h) of the device's y; statistics against fp64 sums of the device's y.  With a
                    prologue, where dsnt_conv_fwd_pro_ok accepts the case: dsnt_conv_fwd_pro on dsnt_bn_stats partials leaves the
                    vectors and running statistics of dsnt_bn_finalize and the bits of the launch on those vectors.
      inplace       res1 == y (the accumulating data gradient): no bias, no second residual.
      bnb_relu / bnb_norelu   the case as a data-gradient launch with the BatchNorm-backward epilogue (dsnt_conv_fwd_ex, without
                    and with amax): dz against the reference, zero exactly where the fp64 pre-activation is <= 0, the two sums
                    against fp64 sums over the device's dz."""
    from dsnt import _lib
    from dsnt._lib import ptr, call, BnTail, BnPrologue, BnBwdEpilogue
    assert mode in CONV_F32_MODES
    N, H, W, Cin, Cout, k, stride, pad, dil = case
    dev = torch.device('cuda:0')
    o = _f32_operands(case)
    g, M = o['g'], o['M']
    bm = _lib.fn('dsnt_conv_fwd_bm')(C.byref(g))
    tiles = (M + bm - 1) // bm
    xd = nhwc(o['x']).to(dev)
    wd = o['w'].permute(0, 2, 3, 1).contiguous().to(dev)          # OHWI
    figs = {}

    bounds = _out_bounds

    if mode.startswith('bnb'):
        relu = 1 if mode == 'bnb_relu' else 0
        xin, bsc, bsh, bmu, bis, z = _bnb_operands('f32e' + '_'.join(map(str, case)), M, Cout)
        conv = _f32_conv64(o, case)
        ref = torch.where(z > 0, conv, torch.zeros_like(conv)) if relu else conv
        scale = float(ref.abs().max())
        xhat = (xin.double() - bmu.double()) * bis.double()
        xind, vecs = xin.to(dev), [t.to(dev) for t in (bsc, bsh, bmu, bis)]
        bnb = BnBwdEpilogue(ptr(xind), *[ptr(v) for v in vecs], relu)
        for with_amax in (False, True):
            what = '%s %s amax=%d' % (case, mode, with_amax)
            outs = []
            for _ in range(2):
                dz, st, am = Guarded(M, Cout, dev), Guarded(tiles * 2, Cout, dev, guard_rows=4), torch.zeros(64, device=dev)
                t = bounds(0, am, None, None, None)
                call('dsnt_conv_fwd_ex', ptr(xd), ptr(wd), None, ptr(dz.t), None, None, 0, None, None, ptr(st.t), C.byref(g),
                     C.byref(bnb), C.byref(t) if with_amax else None)
                torch.cuda.synchronize()
                outs.append((dz, st, am))
            dz, st, am = outs[0]
            assert dz.intact(), what + ': dz written outside M x Cout'
            got = dz.t.cpu().double()
            err = float((got - ref).abs().max())
            figs['err amax=%d' % with_amax] = err
            assert err <= F32_BAR * scale, (what, err, scale)
            zeros = got == 0
            if relu:
                assert torch.equal(zeros, z <= 0), what + ': the mask differs from the fp64 pre-activation\'s in %d places' % int((zeros != (z <= 0)).sum())
                assert float(zeros.double().mean()) > 0.2          # the mask really is on
            else:
                assert int(zeros.sum()) == 0, what + ': relu = 0 and %d zeros' % int(zeros.sum())
            figs['sums amax=%d' % with_amax] = _f32_check_stats(st, got, xhat, bm, tiles, what)
            if with_amax:
                assert float(am.max()) == float(dz.t.abs().max()), what
            assert _f32_same(outs[0], outs[1]), what + ': two launches differ'
        figs['scale'] = scale
        return figs

    inplace = mode == 'inplace'
    pro = mode.startswith('pro')
    in_relu = 1 if mode == 'pro_relu' else 0
    bd = None if inplace else o['b'].to(dev)
    r1d = o['r1'].to(dev)
    r2d = None if inplace else o['r2'].to(dev)
    ascd, ashd = o['asc'].to(dev), o['ash'].to(dev)
    extra = o['r1'].double() if inplace else o['b'].double() + o['r1'].double() + o['r2'].double()

    def launch(vec, tail_relu, prologue=None):
        """tail_relu None: no dsnt_out_bounds (dsnt_conv_fwd); 0 / 1: amax and amax_bn with that amax_relu (dsnt_conv_fwd_ex);
        prologue: a function (y, st, tail) -> the launch itself, for dsnt_conv_fwd_pro."""
        y = Guarded(M, Cout, dev, init=r1d if inplace else None)
        st = Guarded(tiles * 2, Cout, dev, guard_rows=4)
        am, amb = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
        t = None if tail_relu is None else bounds(tail_relu, am, amb, ascd, ashd)
        res1 = y.t if inplace else r1d
        if prologue is not None:
            prologue(y, st, res1, None if t is None else C.byref(t))
        elif t is None:
            call('dsnt_conv_fwd', ptr(xd), ptr(wd), ptr(bd), ptr(y.t), ptr(vec[0]) if vec else None, ptr(vec[1]) if vec else None,
                 in_relu, ptr(res1), ptr(r2d), ptr(st.t), C.byref(g))
        else:
            call('dsnt_conv_fwd_ex', ptr(xd), ptr(wd), ptr(bd), ptr(y.t), ptr(vec[0]) if vec else None, ptr(vec[1]) if vec else None,
                 in_relu, ptr(res1), ptr(r2d), ptr(st.t), C.byref(g), None, C.byref(t))
        torch.cuda.synchronize()
        return y, st, am, amb

    def check(out, ref, tail_relu, what):
        y, st, am, amb = out
        assert y.intact(), what + ': y written outside M x Cout'
        got = y.t.cpu().double()
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max())
        assert err <= F32_BAR * scale, (what, err, scale)
        s = _f32_check_stats(st, got, got, bm, tiles, what)
        if tail_relu is not None:
            assert float(am.max()) == float(y.t.abs().max()), (what, float(am.max()), float(y.t.abs().max()))
            v = got * o['asc'].double() + o['ash'].double()
            want = float((v.clamp_min(0.0) if tail_relu else v).abs().max())
            assert want > 0 and abs(float(amb.max()) - want) <= ULP * want, (what, float(amb.max()), want)
        return dict(err=err, scale=scale, sums=s)

    vec = (o['sc'].to(dev), o['sh'].to(dev)) if pro else None
    ref = _f32_conv64(o, case, o['sc'] if pro else None, o['sh'] if pro else None, in_relu) + extra
    for tail_relu in (None, 1, 0):
        what = '%s %s bounds=%s' % (case, mode, tail_relu)
        a, b = launch(vec, tail_relu), launch(vec, tail_relu)
        r = check(a, ref, tail_relu, what)
        figs['err bounds=%s' % tail_relu], figs['sums bounds=%s' % tail_relu], figs['scale'] = r['err'], r['sums'], r['scale']
        assert _f32_same(a, b), what + ': two launches differ'

    # the BatchNorm of the A operand finalised in the launch's own prologue
    rows = N * H * W
    tiles_in = (rows + 127) // 128
    if pro and _lib.fn('dsnt_conv_fwd_pro_ok')(C.byref(g), tiles_in, Cin) == 1:
        tag = 'f32e' + '_'.join(map(str, case))
        part = torch.empty(tiles_in, 2, Cin, device=dev)
        call('dsnt_bn_stats', ptr(xd), ptr(part), rows, Cin)
        gamma = (synthetic.tensor(tag + 'ga', (Cin,), seed=10, kind='uniform') + 1.5).to(dev)
        beta = synthetic.tensor(tag + 'be', (Cin,), seed=11, scale=0.2).to(dev)
        rm0 = synthetic.tensor(tag + 'rm', (Cin,), seed=12, scale=0.3).to(dev)
        rv0 = (synthetic.tensor(tag + 'rv', (Cin,), seed=13, kind='uniform').abs() + 0.5).to(dev)
        v_ref, rm_ref, rv_ref = [torch.full((Cin,), float('nan'), device=dev) for _ in range(4)], rm0.clone(), rv0.clone()
        call('dsnt_bn_finalize', ptr(part), tiles_in, rows, Cin, ptr(gamma), ptr(beta), ptr(rm_ref), ptr(rv_ref), 0.1, 1e-5, 1,
             *[ptr(t_) for t_ in v_ref])
        torch.cuda.synchronize()
        ref_bn = _f32_conv64(o, case, v_ref[2].cpu(), v_ref[3].cpu(), in_relu) + extra
        for tail_relu in (None, 1):
            what = '%s %s prologue bounds=%s' % (case, mode, tail_relu)
            sep = launch((v_ref[2], v_ref[3]), tail_relu)
            figs['err separate bounds=%s' % tail_relu] = check(sep, ref_bn, tail_relu, what + ' (separately finalised)')['err']
            fused = []
            for _ in range(2):
                v, rm, rv = [torch.full((Cin,), float('nan'), device=dev) for _ in range(4)], rm0.clone(), rv0.clone()
                bp = BnPrologue(ptr(part), tiles_in, Cin, rows, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), 0.1, 1e-5, *[ptr(t_) for t_ in v])

                def prologue(y, st, res1, t):
                    call('dsnt_conv_fwd_pro', ptr(xd), ptr(wd), ptr(bd), ptr(y.t), C.byref(bp), in_relu, ptr(res1), ptr(r2d), ptr(st.t),
                         C.byref(g), t)
                out = launch(None, tail_relu, prologue)
                for name, a_, b_ in zip(('mean', 'invstd', 'scale', 'shift', 'running_mean', 'running_var'), v + [rm, rv],
                                        v_ref + [rm_ref, rv_ref]):
                    assert torch.equal(a_, b_), '%s: %s differs from dsnt_bn_finalize\'s by %.3e' % (what, name, float((a_ - b_).abs().max()))
                fused.append(out)
            assert _f32_same(fused[0], sep), what + ': not the bits of the launch on separately finalised vectors'
            assert _f32_same(fused[0], fused[1]), what + ': two launches differ'
    return figs


# ---------------------------------------------------------------- the tiled split-precision kernels at their plan edges (csrc/conv_split6.hip)

CONV_SPLIT_PATHS = ('bf16x6', 'f16x3')
PLANE_GAP = 8               # elements between the end of a weight plane and the next one, for the cases at an odd index
A_SLOT = 7                  # the slot of the 64 that holds the A operand's bound: any may


def split_weight_planes(wd, path, gap, dev):
    """The OHWI weights `wd` as the planes a split-precision launch reads: (planes, plane_stride, w_bound).  bf16x6: three bf16
    planes of dsnt_split_bf16x3, copied `numel + gap` apart; fp16x3: dsnt_amax, then dsnt_split_f16x2 with that stride.  What
    lies between the planes is NaN."""
    from dsnt._lib import ptr, call
    n = wd.numel()
    stride = n + gap
    if path == 'bf16x6':
        tight = torch.empty(3 * n, dtype=torch.bfloat16, device=dev)
        call('dsnt_split_bf16x3', ptr(wd), ptr(tight), n)
        assert torch.equal(tight.view(3, n).float().sum(0), wd.reshape(-1))            # the split is exact
        planes = torch.full((3 * stride,), float('nan'), dtype=torch.bfloat16, device=dev)
        planes.view(3, stride)[:, :n] = tight.view(3, n)
        wb = None
    else:
        wb = torch.zeros(64, device=dev)
        call('dsnt_amax', ptr(wd), n, ptr(wb))
        assert wb.max().item() == wd.abs().max().item()
        planes = torch.full((2 * stride,), float('nan'), dtype=torch.float16, device=dev)
        call('dsnt_split_f16x2', ptr(wd), ptr(planes), n, stride, ptr(wb))
    v = planes.view(-1, stride)
    assert bool(torch.isfinite(v[:, :n]).all()) and bool(torch.isnan(v[:, n:]).all())
    return planes, stride, wb


def split_launch(path, xd, planes, stride, wb, ab, bias, y, sc, sh, in_relu, res1, res2, st, g, bnb=None, tail=None, check=True):
    """dsnt_conv_fwd_bf16x6_ex / dsnt_conv_fwd_f16x3_ex (ab: the A operand's bound) on the current stream; the return code."""
    from dsnt import _lib
    from dsnt._lib import ptr
    common = (ptr(bias), ptr(y), ptr(sc), ptr(sh), in_relu, ptr(res1), ptr(res2), ptr(st), C.byref(g),
              None if bnb is None else C.byref(bnb), None if tail is None else C.byref(tail), _lib.stream_ptr())
    if path == 'bf16x6':
        rc = _lib.fn('dsnt_conv_fwd_bf16x6_ex')(ptr(xd), ptr(planes), stride, *common)
    else:
        rc = _lib.fn('dsnt_conv_fwd_f16x3_ex')(ptr(xd), ptr(planes), stride, ptr(wb), ptr(ab), *common)
    assert rc == 0 or not check, (rc, _lib.fn('dsnt_last_error')())
    return rc


def split_tile_of(case, halo):
    """The statistics tile of every output row: 128 consecutive rows, or — the halo kernel — the 8 x 16 patch of pixels
    [8 th, 8 th + 8) x [16 tw, 16 tw + 16) of image img, tile (img * (H / 8) + th) * (W / 16) + tw."""
    N, H, W = case[:3]
    if not halo:
        return None
    m = torch.arange(N * H * W)
    img, oh, ow = m // (H * W), m % (H * W) // W, m % W
    return (img * (H // 8) + oh // 8) * (W // 16) + ow // 16


def conv_split_edge(case, path, mode):
    """One case of tests/plan_edge_cases.py CONV_SPLIT on one path (bf16x6: dsnt_conv_fwd_bf16x6_ex; f16x3: dsnt_conv_fwd_f16x3_ex
    with the weight bound of dsnt_amax and the A operand's bound in slot A_SLOT) in one mode of CONV_F32_MODES, against torch fp64
    on the CPU.  As conv_f32_edge: sentinel-filled guarded buffers, every launch twice into fresh ones (the same bits).
      fwd / pro_relu / pro_norelu   bias, res1, res2, statistics; without a dsnt_out_bounds, then with amax + amax_bn at amax_relu 1
                    and 0.  fp16x3: the A bound exact; in fwd and pro_relu also 64 times loose.
      inplace       res1 == y, no bias, no second residual.
      bnb_relu / bnb_norelu   the BatchNorm-backward epilogue without and with amax: dz is zero exactly where the fp64
                    pre-activation is <= 0 (relu 1) and where every tap of the output pixel lies in the padding — nowhere else.
    Outputs: F32_BAR of max |reference|, and an error of fp32 size — at most max(4 err32, 2e-6 scale), err32 the error of torch's
    fp32 CPU convolution (masked with the fp64 mask in the bnb modes) on the same operands.  Statistics: per tile (the halo
    kernel's are 8 x 16 patches), SUM_BAR against fp64 sums over the device's own output.  amax exact, amax_bn within ULP."""
    from dsnt import _lib
    from dsnt._lib import BnBwdEpilogue
    import plan_edge_cases as E
    assert mode in CONV_F32_MODES and path in CONV_SPLIT_PATHS
    N, H, W, Cin, Cout, R, S, stride_, pad, dil = case
    dev = torch.device('cuda:0')
    o = _f32_operands(case)
    g, M = o['g'], o['M']
    f16 = path == 'f16x3'
    halo = _lib.fn('dsnt_conv_f16x3_route')(C.byref(g), 0) == 2
    tiles = (M + 127) // 128
    tile_of = split_tile_of(case, halo)
    xd = nhwc(o['x']).to(dev)
    wd = o['w'].permute(0, 2, 3, 1).contiguous().to(dev)          # OHWI
    planes, stride, wb = split_weight_planes(wd, path, PLANE_GAP if E.CONV_SPLIT.index(case) % 2 else 0, dev)
    figs = dict(err_max=0.0, sums_max=0.0)

    def a_bound(value, loose=1.0):
        if not f16:
            return None
        ab = torch.zeros(64, device=dev)
        ab[A_SLOT] = value * loose
        return ab

    def outputs(got, ref, ref32, what):
        """y or dz against fp64, at the project's bar and at fp32 size."""
        assert bool((got != SENT).all()), '%s: %d output elements never written' % (what, int((got == SENT).sum()))
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max())
        err32 = float((ref32.double() - ref).abs().max())
        figs.update(scale=scale, err32=err32, err_max=max(figs['err_max'], err))
        assert err <= F32_BAR * scale, (what, err, scale)
        assert err <= max(4 * err32, 2e-6 * scale), (what, err, err32, scale)
        return err

    if mode.startswith('bnb'):
        relu = 1 if mode == 'bnb_relu' else 0
        xin, bsc, bsh, bmu, bis, z = _bnb_operands(o['tag'], M, Cout)
        conv, conv32 = _f32_conv64(o, case), _f32_conv64(o, case, dtype=torch.float32)
        ref = torch.where(z > 0, conv, torch.zeros_like(conv)) if relu else conv
        ref32 = torch.where(z > 0, conv32, torch.zeros_like(conv32)) if relu else conv32
        # output pixels whose every tap lies in the padding (Ho > H): this launch has no bias, their sums are exactly zero
        taps = F.conv2d(torch.ones(N, 1, H, W, dtype=torch.float64), torch.ones(1, 1, R, S, dtype=torch.float64), None, stride=stride_,
                        padding=pad, dilation=dil)
        pad_only = (taps.reshape(M, 1) == 0).expand(M, Cout)
        assert bool((conv[pad_only] == 0).all()) and int((conv == 0).sum()) == int(pad_only.sum())
        xhat = (xin.double() - bmu.double()) * bis.double()
        xind, vecs = xin.to(dev), [t.to(dev) for t in (bsc, bsh, bmu, bis)]
        bnb = BnBwdEpilogue(xind.data_ptr(), *[v.data_ptr() for v in vecs], relu)
        ab = a_bound(float(o['x'].abs().max()))
        for with_amax in (False, True):
            what = '%s %s %s amax=%d' % (case, path, mode, with_amax)
            outs = []
            for _ in range(2):
                dz, st, am = Guarded(M, Cout, dev), Guarded(tiles * 2, Cout, dev, guard_rows=4), torch.zeros(64, device=dev)
                t = _out_bounds(0, am, None, None, None)
                split_launch(path, xd, planes, stride, wb, ab, None, dz.t, None, None, 0, None, None, st.t, g, bnb, t if with_amax else None)
                torch.cuda.synchronize()
                outs.append((dz, st, am))
            dz, st, am = outs[0]
            assert dz.intact(), what + ': dz written outside M x Cout'
            got = dz.t.cpu().double()
            figs['err amax=%d' % with_amax] = outputs(got, ref, ref32, what)
            zeros = got == 0
            if relu:
                want0 = (z <= 0) | pad_only
                assert torch.equal(zeros, want0), what + ': the mask differs from the fp64 pre-activation\'s in %d places' % int((zeros != want0).sum())
                assert float((z <= 0).double().mean()) > 0.2          # the mask really is on
            else:
                assert torch.equal(zeros, pad_only), what + ': relu = 0 and %d zeros' % int((zeros != pad_only).sum())
            figs['sums amax=%d' % with_amax] = _f32_check_stats(st, got, xhat, 128, tiles, what, tile_of)
            figs['sums_max'] = max(figs['sums_max'], figs['sums amax=%d' % with_amax])
            if with_amax:
                assert float(am.max()) == float(dz.t.abs().max()), what
            assert _f32_same(outs[0], outs[1]), what + ': two launches differ'
        return figs

    inplace = mode == 'inplace'
    pro = mode.startswith('pro')
    in_relu = 1 if mode == 'pro_relu' else 0
    bd = None if inplace else o['b'].to(dev)
    r1d = o['r1'].to(dev)
    r2d = None if inplace else o['r2'].to(dev)
    ascd, ashd = o['asc'].to(dev), o['ash'].to(dev)
    scd, shd = (o['sc'].to(dev), o['sh'].to(dev)) if pro else (None, None)
    vec = (o['sc'], o['sh']) if pro else (None, None)
    conv, conv32 = _f32_conv64(o, case, *vec, in_relu), _f32_conv64(o, case, *vec, in_relu, dtype=torch.float32)
    if inplace:
        ref, ref32 = conv + o['r1'].double(), conv32 + o['r1']
    else:
        ref, ref32 = conv + (o['b'].double() + o['r1'].double() + o['r2'].double()), conv32 + o['b'] + o['r1'] + o['r2']
    act = o['x'].double()
    if pro:
        act = act * o['sc'].double().view(1, -1, 1, 1) + o['sh'].double().view(1, -1, 1, 1)
        act = F.relu(act) if in_relu else act
    act_max = float(act.abs().max())

    def launch(ab, tail_relu):
        y = Guarded(M, Cout, dev, init=r1d if inplace else None)
        st = Guarded(tiles * 2, Cout, dev, guard_rows=4)
        am, amb = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
        t = None if tail_relu is None else _out_bounds(tail_relu, am, amb, ascd, ashd)
        split_launch(path, xd, planes, stride, wb, ab, bd, y.t, scd, shd, in_relu, y.t if inplace else r1d, r2d, st.t, g, None, t)
        torch.cuda.synchronize()
        return y, st, am, amb

    for loose in ((1.0, 64.0) if f16 and mode in ('fwd', 'pro_relu') else (1.0,)):
        ab = a_bound(act_max, loose)
        for tail_relu in (None, 1, 0):
            what = '%s %s %s bounds=%s bound x %g' % (case, path, mode, tail_relu, loose)
            key = 'bounds=%s%s' % (tail_relu, '' if loose == 1.0 else ' loose')
            a, b = launch(ab, tail_relu), launch(ab, tail_relu)
            y, st, am, amb = a
            assert y.intact(), what + ': y written outside M x Cout'
            got = y.t.cpu().double()
            figs['err ' + key] = outputs(got, ref, ref32, what)
            figs['sums ' + key] = _f32_check_stats(st, got, got, 128, tiles, what, tile_of)
            figs['sums_max'] = max(figs['sums_max'], figs['sums ' + key])
            if tail_relu is not None:
                assert float(am.max()) == float(y.t.abs().max()), (what, float(am.max()), float(y.t.abs().max()))
                v = got * o['asc'].double() + o['ash'].double()
                want = float((v.clamp_min(0.0) if tail_relu else v).abs().max())
                assert want > 0 and abs(float(amb.max()) - want) <= ULP * want, (what, float(amb.max()), want)
            assert _f32_same(a, b), what + ': two launches differ'
    return figs
